// conv3d_grad.hip - the gradient kernels of the 3x3x3 convolution csd_conv3d_block (stride 1, zero padding 1, channels-last fp32):
//   csd_conv3d_wgrad         dW[co][ci][kd][kh][kw] = sum over b, voxel v of dy[b, v, co] * a[b, v + tap, ci]
//   csd_conv3d_dgrad_scale   the per-sample power of two that makes csd_conv3d_block's split-fp16 data gradient scale invariant
//
// Weight gradient, CSD_PREC_F16X3: v_mfma_f32_32x32x16_bf16 with split-bf16 operands, the arithmetic of wgrad_bf16.hip restated:
//     hi = x with the low 16 bits cleared (a bf16), lo = bf16(x - hi) (x - hi is exact in fp32; rounded to nearest even)
//     dy * a ~= hi*hi + hi*lo + lo*hi   -> 3 MFMAs, fp32 accumulate, ~2^-16 relative error per product
// bf16 rather than fp16 halves: gradients span the whole fp32 exponent range (a loss averaged over 1e5 voxels lives below 6e-5).
//   * the contraction index is the VOXEL.  A workgroup (4 waves) owns one 32 cout x 32 cin tile and walks the bricks of one K split:
//     the forward kernel's 128-voxel bricks (4 x 8 x 4, or 8 x 8 x 2 where W < 3) of ONE sample.  Per brick the dy brick [128][32] and the
//     halo patch of a [<= 400][32] are staged in LDS as [voxel][channel] dwords, split ONCE while staging: (hi bf16 << 16) | lo bf16.  A
//     voxel outside the volume (padding, ragged brick) and a channel beyond Cin / Cout are staged as 0 and contribute exactly 0: masked,
//     never clamped, and never read from memory.
//   * a lane gathers its 8 K values (8 voxels of its channel) at any tap offset with 8 ds_read_b32 (bank = channel) and two v_perm per
//     pair give the hi and the lo operand.  8 K steps of 16 voxels per brick.
//   * 32 x 32 x 27 taps = 432 accumulators are too many for one wave: the taps are split over the waves, 7 / 7 / 7 / 6, on the shared
//     patch (112 accumulator registers per wave).  No cross-wave reduction.
//   * split K: a split is a run of bricks of one sample, and the number of splits per sample depends on the volume and the channel
//     counts only - never on B - so a sample's partial sums do not depend on its neighbours or its place in the batch.  Partials
//     [split][tap][Cout][Cin] are summed in fp64 in split order by a second kernel that writes dw [Cout][Cin][27].  No atomics; the
//     result is bitwise repeatable and independent of launch order.
// CSD_PREC_F32 (the exact yardstick, untuned, like conv3d_direct_kernel): one thread per (tap, co, ci), one fp32 fmaf chain over the
// voxels of its split in voxel order, the same partial layout and reduction.  It also serves CSD_PREC_F16X3 where min(Cin, Cout) < 8
// (the 1- / 2-channel stem and head: an MFMA tile would be >= 75 % padding).
#include <string.h>

#include <algorithm>

#include "common.h"

namespace csd {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef float v4f_t __attribute__((ext_vector_type(4)));

#define W3_THREADS 256
#define W3_TAPS 27
#define W3_WTAPS 7                // taps per wave (wave 3: 6)
#define W3_NPIX 128               // voxels per brick
#define W3_THIN 8                 // min(Cin, Cout) below this: the fp32 kernel in both precisions
#define W3_WG_PER_SAMPLE 256      // MFMA: workgroups per sample the split count aims at
#define W3_F32_MIN_CHUNK 1024     // fp32: voxels per split at least
#define W3_F32_MAX_SPLITS 64      // fp32: splits per sample at most

struct Wgrad3dArgs {
  const float* a;
  const float* dy;
  float* partial;
  int B, D, H, W, Cin, Cout;
  int nbd, nbh, nbw, nbricks;     // bricks of one sample
  int nsplit, per_split;          // splits per sample; bricks (MFMA) or voxels (fp32) per split
  int n_ci, n_co;
};

__device__ __forceinline__ unsigned split_bf16(float v) {      // (hi bf16 << 16) | lo bf16
  const unsigned hb = __float_as_uint(v) & 0xffff0000u;
  unsigned lb = __float_as_uint(v - __uint_as_float(hb));     // exact
  lb += 0x7fffu + ((lb >> 16) & 1u);                           // round to nearest even (|lo| < 2^-7 |hi|: never overflows to inf)
  return hb | (lb >> 16);
}

template <int TD, int TH, int TW, bool VEC>
__global__ __launch_bounds__(W3_THREADS, 2) void conv3d_wgrad_bf16_kernel(const Wgrad3dArgs k) {
  constexpr int PD = TD + 2, PH = TH + 2, PW = TW + 2, NPATCH = PD * PH * PW;
  static_assert(TD * TH * TW == W3_NPIX && 16 % TW == 0 && (16 / TW) <= TH && TH % (8 / TW) == 0, "brick");
  extern __shared__ __attribute__((aligned(16))) unsigned smem_w3[];
  unsigned* const dyb = smem_w3;                       // [128][32]
  unsigned* const patch = smem_w3 + W3_NPIX * 32;      // [NPATCH][32]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 31, kg = lane >> 5;

  unsigned wid = blockIdx.x;
  const int ty = (int)(wid % (unsigned)k.n_ci); wid /= (unsigned)k.n_ci;
  const int tz = (int)(wid % (unsigned)k.n_co); wid /= (unsigned)k.n_co;
  const int split = (int)wid;                          // b * nsplit + c
  const int b = split / k.nsplit, c = split - b * k.nsplit;
  const int br_begin = c * k.per_split;
  const int br_end = min(br_begin + k.per_split, k.nbricks);
  const size_t vox = (size_t)k.D * k.H * k.W;
  const float* const a_s = k.a + (size_t)b * vox * k.Cin;
  const float* const dy_s = k.dy + (size_t)b * vox * k.Cout;
  const int ci0 = ty * 32, co0 = tz * 32;

  // this wave's taps and their patch offsets (scalar)
  const int tap0 = wave * W3_WTAPS;
  const int ntap = min(W3_WTAPS, W3_TAPS - tap0);
  int toff[W3_WTAPS];
#pragma unroll
  for (int i = 0; i < W3_WTAPS; ++i) {
    const int t = min(tap0 + i, W3_TAPS - 1);
    toff[i] = (((t / 9) * PH + (t / 3) % 3) * PW + t % 3) * 32;
  }
  // voxel j of a lane's 8: (tw, th) offsets inside the brick are compile-time constants (8 voxels never wrap TH)
  floatx16 acc[W3_WTAPS];
#pragma unroll
  for (int i = 0; i < W3_WTAPS; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // staging: VEC: slot e = channel quad e & 7 of voxel e >> 3 (one 16-byte load); else channel e & 31 of voxel e >> 5
  constexpr int CPV = VEC ? 8 : 32;                    // slots per voxel
  auto load_slot = [&](const float* src, int C, int cbase, int sv, int e, float (&v)[4]) {
    // sv: voxel index inside the sample or -1
    if (VEC) {
      const int ch = cbase + 4 * (e & 7);
      v[0] = v[1] = v[2] = v[3] = 0.f;
      if (sv >= 0 && ch < C) {
        const v4f_t q = *(const __attribute__((address_space(1))) v4f_t*)(src + (size_t)sv * C + ch);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      }
    } else {
      const int ch = cbase + (e & 31);
      v[0] = (sv >= 0 && ch < C) ? src[(size_t)sv * C + ch] : 0.f;
    }
  };
  auto store_slot = [&](unsigned* dst, int e, const float (&v)[4]) {
    if (VEC) {
      uintx4 q;
      q.x = split_bf16(v[0]); q.y = split_bf16(v[1]); q.z = split_bf16(v[2]); q.w = split_bf16(v[3]);
      *reinterpret_cast<uintx4*>(dst + (e >> 3) * 32 + 4 * (e & 7)) = q;
    } else {
      dst[e] = split_bf16(v[0]);
    }
  };

  for (int br = br_begin; br < br_end; ++br) {
    int r = br;
    const int bw = r % k.nbw; r /= k.nbw;
    const int bh = r % k.nbh;
    const int bd = r / k.nbh;
    const int d0 = bd * TD, h0 = bh * TH, w0 = bw * TW;
    if (br != br_begin) __syncthreads();               // every wave is done with the previous brick
    // ---- dy brick ----
    constexpr int NDY = W3_NPIX * CPV;
    for (int e0 = tid; e0 < NDY; e0 += W3_THREADS * 4) {
      float v[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * W3_THREADS;
        const int p = e / CPV;
        const int tw = p % TW, th = (p / TW) % TH, td = p / (TW * TH);
        const int d = d0 + td, h = h0 + th, x = w0 + tw;
        const int sv = (e < NDY && d < k.D && h < k.H && x < k.W) ? (d * k.H + h) * k.W + x : -1;
        load_slot(dy_s, k.Cout, co0, sv, e, v[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * W3_THREADS;
        if (e < NDY) store_slot(dyb, e, v[u]);
      }
    }
    // ---- halo patch of a ----
    constexpr int NPA = NPATCH * CPV;
    for (int e0 = tid; e0 < NPA; e0 += W3_THREADS * 4) {
      float v[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * W3_THREADS;
        const int p = e / CPV;
        const int pw = p % PW, ph = (p / PW) % PH, pd = p / (PW * PH);
        const int d = d0 - 1 + pd, h = h0 - 1 + ph, x = w0 - 1 + pw;
        const int sv = (e < NPA && d >= 0 && d < k.D && h >= 0 && h < k.H && x >= 0 && x < k.W) ? (d * k.H + h) * k.W + x : -1;
        load_slot(a_s, k.Cin, ci0, sv, e, v[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * W3_THREADS;
        if (e < NPA) store_slot(patch, e, v[u]);
      }
    }
    __syncthreads();

    // ---- 8 K steps of 16 voxels; lane half kg takes voxels 16 s + 8 kg + j ----
#pragma unroll 1
    for (int s = 0; s < W3_NPIX / 16; ++s) {
      const int v0 = 16 * s + 8 * kg;
      const int row0 = v0 / TW;                         // (th, td) of voxel v0; tw = 0
      const int pbase = (((row0 / TH) * PH + row0 % TH) * PW) * 32 + m;
      unsigned aw[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) aw[j] = dyb[(v0 + j) * 32 + m];
      uintx4 ah, al;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ah[j] = __builtin_amdgcn_perm(aw[2 * j + 1], aw[2 * j], 0x07060302u);
        al[j] = __builtin_amdgcn_perm(aw[2 * j + 1], aw[2 * j], 0x05040100u);
      }
      const bf16x8 Ah = __builtin_bit_cast(bf16x8, ah), Al = __builtin_bit_cast(bf16x8, al);
#pragma unroll
      for (int i = 0; i < W3_WTAPS; ++i) {
        if (i < ntap) {
          unsigned xw[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) xw[j] = patch[pbase + toff[i] + ((j / TW) * PW + j % TW) * 32];
          uintx4 bh, bl;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            bh[j] = __builtin_amdgcn_perm(xw[2 * j + 1], xw[2 * j], 0x07060302u);
            bl[j] = __builtin_amdgcn_perm(xw[2 * j + 1], xw[2 * j], 0x05040100u);
          }
          const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh), Bl = __builtin_bit_cast(bf16x8, bl);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh, acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl, acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh, acc[i], 0, 0, 0);
        }
      }
    }
  }

  // ---- partial [split][tap][Cout][Cin]: lane = cin (128 B per half wave) ----
  const int ci = ci0 + m;
#pragma unroll
  for (int i = 0; i < W3_WTAPS; ++i) {
    if (i < ntap) {
      float* dst = k.partial + ((size_t)split * W3_TAPS + (tap0 + i)) * k.Cout * k.Cin;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * kg;
        if (co < k.Cout && ci < k.Cin) dst[(size_t)co * k.Cin + ci] = acc[i][r];
      }
    }
  }
}

// ---- the fp32 yardstick: one thread per (tap, co, ci), one fmaf chain over the voxels of the split in voxel order -----------------------
__global__ __launch_bounds__(W3_THREADS) void conv3d_wgrad_f32_kernel(const Wgrad3dArgs k) {
  const int nw = W3_TAPS * k.Cout * k.Cin;
  const unsigned nblk = (unsigned)(nw + W3_THREADS - 1) / W3_THREADS;
  const int split = (int)(blockIdx.x / nblk);
  const int idx = (int)(blockIdx.x % nblk) * W3_THREADS + threadIdx.x;
  if (idx >= nw) return;
  const int b = split / k.nsplit, c = split - b * k.nsplit;
  const int ci = idx % k.Cin;
  const int co = (idx / k.Cin) % k.Cout;
  const int tap = idx / (k.Cin * k.Cout);
  const int kd = tap / 9 - 1, kh = (tap / 3) % 3 - 1, kw = tap % 3 - 1;
  const int vox = k.D * k.H * k.W;
  const int v_begin = c * k.per_split;
  const int v_end = min(v_begin + k.per_split, vox);
  const float* a_s = k.a + (size_t)b * vox * k.Cin + ci;
  const float* dy_s = k.dy + (size_t)b * vox * k.Cout + co;
  float acc = 0.f;
  for (int v = v_begin; v < v_end; ++v) {
    const int x = v % k.W, h = (v / k.W) % k.H, d = v / (k.W * k.H);
    const int dd = d + kd, hh = h + kh, xx = x + kw;
    if (dd < 0 || dd >= k.D || hh < 0 || hh >= k.H || xx < 0 || xx >= k.W) continue;       // zero padding: contributes exactly 0
    acc = fmaf(dy_s[(size_t)v * k.Cout], a_s[(size_t)((dd * k.H + hh) * k.W + xx) * k.Cin], acc);
  }
  k.partial[(size_t)split * nw + idx] = acc;
}

// dw[co][ci][tap] = sum over splits (split order, fp64) of partial[split][tap][co][ci]; beta = 1: added to what dw holds, in one fp32
// addition of the value beta = 0 stores
// (ci_off, Cin_dw: the Cin channels are the slice ci_off .. ci_off + Cin of a weight with Cin_dw input channels - one source of a
// two-source layer; the whole weight: 0, Cin)
__global__ void conv3d_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int nsplits, int Cin, int Cout,
                                           int beta, int ci_off, int Cin_dw) {
  const int nw = W3_TAPS * Cout * Cin;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nw) return;
  double s = 0.0;
  for (int i = 0; i < nsplits; ++i) s += (double)partial[(size_t)i * nw + idx];
  const int ci = idx % Cin;
  const int co = (idx / Cin) % Cout;
  const int tap = idx / (Cin * Cout);
  float* dst = dw + ((size_t)co * Cin_dw + ci_off + ci) * W3_TAPS + tap;
  const float v = (float)s;
  *dst = beta ? *dst + v : v;
}

// the stem's data gradient at the network boundary (common.h): one thread per (b, input channel, voxel)
__global__ __launch_bounds__(W3_THREADS) void conv3d_stem_dx_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                    float* __restrict__ dx, int B, int nx, int Cin, int Cout, int D, int H,
                                                                    int W, float scale) {
  const size_t vox = (size_t)D * H * W;
  const size_t total = (size_t)B * nx * vox;
  const size_t idx = (size_t)blockIdx.x * W3_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int vi = (int)(idx % vox);
  const size_t r = idx / vox;
  const int ci = (int)(r % nx);
  const size_t b = r / nx;
  const int x = vi % W, h = (vi / W) % H, d = vi / (W * H);
  float acc = 0.f;
  for (int tap = 0; tap < W3_TAPS; ++tap) {            // y[v] reads x[v + off(tap)]: x[u] feeds y[u - off(tap)]
    const int dd = d - (tap / 9 - 1), hh = h - ((tap / 3) % 3 - 1), xx = x - (tap % 3 - 1);
    if (dd < 0 || dd >= D || hh < 0 || hh >= H || xx < 0 || xx >= W) continue;
    const float* p = dy + (b * vox + ((size_t)dd * H + hh) * W + xx) * Cout;
    const float* wp = w + (size_t)ci * W3_TAPS + tap;
    for (int co = 0; co < Cout; ++co) acc = fmaf(p[co], wp[(size_t)co * Cin * W3_TAPS], acc);
  }
  dx[idx] = acc * scale;
}

bool wgrad3d_use_mfma(int Cin, int Cout, int precision) { return precision == CSD_PREC_F16X3 && std::min(Cin, Cout) >= W3_THIN; }

// the K splits of one sample: a function of the volume and the channel counts only (never of B)
void wgrad3d_plan(Wgrad3dArgs* a, int precision) {
  const int vox = a->D * a->H * a->W;
  a->n_ci = cdiv(a->Cin, 32);
  a->n_co = cdiv(a->Cout, 32);
  if (wgrad3d_use_mfma(a->Cin, a->Cout, precision)) {
    const int TD = a->W >= 3 ? 4 : 8, TH = 8, TW = a->W >= 3 ? 4 : 2;
    a->nbd = cdiv(a->D, TD); a->nbh = cdiv(a->H, TH); a->nbw = cdiv(a->W, TW);
    a->nbricks = a->nbd * a->nbh * a->nbw;
    const int want = std::min(a->nbricks, std::max(1, W3_WG_PER_SAMPLE / (a->n_ci * a->n_co)));
    a->per_split = cdiv(a->nbricks, want);
    a->nsplit = cdiv(a->nbricks, a->per_split);
  } else {
    a->per_split = std::max(W3_F32_MIN_CHUNK, cdiv(vox, W3_F32_MAX_SPLITS));
    a->nsplit = cdiv(vox, a->per_split);
  }
}

bool wgrad3d_shape_ok(int B, int Cin, int Cout, int D, int H, int W) {
  if (B < 1 || D < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return false;
  const size_t vox = (size_t)D * H * W;
  if (vox >= ((size_t)1 << 28) || vox * (size_t)std::max(Cin, Cout) * sizeof(float) >= ((size_t)1 << 31)) return false;
  return (size_t)Cin * Cout * W3_TAPS < ((size_t)1 << 28) && (size_t)B < ((size_t)1 << 20);
}

template <int TD, int TH, int TW, bool VEC>
int wgrad3d_mfma_launch(const Wgrad3dArgs& a, unsigned nblocks, hipStream_t s) {
  constexpr size_t lds = (size_t)(W3_NPIX + (TD + 2) * (TH + 2) * (TW + 2)) * 32 * sizeof(unsigned);
  CSD_SET_MAX_LDS_ONCE((conv3d_wgrad_bf16_kernel<TD, TH, TW, VEC>));
  hipLaunchKernelGGL((conv3d_wgrad_bf16_kernel<TD, TH, TW, VEC>), dim3(nblocks), dim3(W3_THREADS), lds, s, a);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

// ---- data gradient: per-sample power of two ---------------------------------------------------------------------------------------------
#define DG_CHUNKS 128
__global__ __launch_bounds__(256) void absmax_partial_kernel(const float* __restrict__ x, float* __restrict__ part, int64_t per) {
  __shared__ float red[256];
  const int b = blockIdx.y;
  const float* p = x + (size_t)b * per;
  float mx = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) mx = fmaxf(mx, fabsf(p[i]));
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = red[0];
}

// rowscale[b] = 2^(4 - floor(log2 max|x_b|)) (max|x_b * rowscale| in [16, 32)); 1 for an all-zero or non-finite sample.
// nscale[b][c] = rowscale[b], nshift[b][c] = 0: the prologue operands of csd_conv3d_block (an exact multiply in its staging)
__global__ void dgrad_scale_finalize_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ rowscale,
                                            float* __restrict__ nscale, float* __restrict__ nshift, int C) {
  const int b = blockIdx.x;
  float mx = 0.f;
  for (int i = 0; i < nchunk; ++i) mx = fmaxf(mx, part[(size_t)b * nchunk + i]);
  float sc = 1.f;
  if (mx > 0.f && mx < __uint_as_float(0x7f800000u)) {
    int e;
    frexpf(mx, &e);                                   // mx = f * 2^e, f in [0.5, 1): floor(log2 mx) = e - 1
    int sh = 5 - e;
    sh = sh > 126 ? 126 : (sh < -126 ? -126 : sh);
    sc = __uint_as_float((unsigned)(sh + 127) << 23);
  }
  if (threadIdx.x == 0) rowscale[b] = sc;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    nscale[(size_t)b * C + c] = sc;
    nshift[(size_t)b * C + c] = 0.f;
  }
}

}  // namespace

int conv3d_stem_dx_launch(const float* dy, const float* w, float* dx, int B, int nx, int Cin, int Cout, int D, int H, int W, float scale,
                          hipStream_t s) {
  CSD_REQUIRE(dy && w && dx && B >= 1 && nx >= 1 && nx <= Cin && Cout >= 1 && D >= 1 && H >= 1 && W >= 1, "conv3d_stem_dx: bad arguments");
  const size_t total = (size_t)B * nx * D * H * W;
  const size_t nb = cdiv64(total, W3_THREADS);
  CSD_REQUIRE(nb < ((size_t)1 << 31) && (size_t)D * H * W < ((size_t)1 << 28), "conv3d_stem_dx: %zu outputs exceed the kernel's grid", total);
  hipLaunchKernelGGL(conv3d_stem_dx_kernel, dim3((unsigned)nb), dim3(W3_THREADS), 0, s, dy, w, dx, B, nx, Cin, Cout, D, H, W, scale);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}
}  // namespace csd

using namespace csd;

extern "C" size_t csd_conv3d_wgrad_scratch_bytes(int B, int Cin, int Cout, int D, int H, int W, int precision) {
  if (!wgrad3d_shape_ok(B, Cin, Cout, D, H, W) || (precision != CSD_PREC_F16X3 && precision != CSD_PREC_F32)) return 0;
  Wgrad3dArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.D = D; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  wgrad3d_plan(&a, precision);
  return scratch_aligned_bytes((size_t)B * a.nsplit * W3_TAPS * Cin * Cout * sizeof(float));
}

extern "C" int csd_conv3d_wgrad(const float* a_in, const float* dy, float* dw, int B, int Cin, int Cout, int D, int H, int W, int precision,
                                void* scratch, void* stream) {
  return conv3d_wgrad_beta(a_in, dy, dw, B, Cin, Cout, D, H, W, precision, scratch, stream, 0);
}

int csd::conv3d_wgrad_beta(const float* a_in, const float* dy, float* dw, int B, int Cin, int Cout, int D, int H, int W, int precision,
                           void* scratch, void* stream, int beta, int ci_off, int Cin_dw) {
  if (Cin_dw <= 0) Cin_dw = Cin;
  CSD_REQUIRE(ci_off >= 0 && ci_off + Cin <= Cin_dw, "conv3d_wgrad: input channels %d .. %d are no slice of %d", ci_off, ci_off + Cin, Cin_dw);
  CSD_REQUIRE(a_in && dy && dw && scratch, "conv3d_wgrad: null argument");
  CSD_REQUIRE(precision == CSD_PREC_F16X3 || precision == CSD_PREC_F32,
              "conv3d_wgrad: precision must be fp16x3 (CSD_PREC_F16X3: split bf16) or fp32 (CSD_PREC_F32)");
  CSD_REQUIRE(wgrad3d_shape_ok(B, Cin, Cout, D, H, W), "conv3d_wgrad: bad shape B=%d %dx%dx%d C=%d->%d", B, D, H, W, Cin, Cout);
  hipStream_t s = (hipStream_t)stream;
  Wgrad3dArgs a;
  memset(&a, 0, sizeof(a));
  a.a = a_in; a.dy = dy;
  a.partial = scratch_aligned<float>(scratch);
  a.B = B; a.D = D; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
  wgrad3d_plan(&a, precision);
  const size_t nsplits = (size_t)B * a.nsplit;
  const int nw = W3_TAPS * Cin * Cout;
  if (wgrad3d_use_mfma(Cin, Cout, precision)) {
    const size_t nblocks = nsplits * a.n_ci * a.n_co;
    CSD_REQUIRE(nblocks < ((size_t)1 << 31), "conv3d_wgrad: %zu workgroups exceed the grid", nblocks);
    const bool vec = Cin % 4 == 0 && Cout % 4 == 0;
    int rc;
    if (W >= 3) rc = vec ? wgrad3d_mfma_launch<4, 8, 4, true>(a, (unsigned)nblocks, s) : wgrad3d_mfma_launch<4, 8, 4, false>(a, (unsigned)nblocks, s);
    else rc = vec ? wgrad3d_mfma_launch<8, 8, 2, true>(a, (unsigned)nblocks, s) : wgrad3d_mfma_launch<8, 8, 2, false>(a, (unsigned)nblocks, s);
    if (rc) return rc;
  } else {
    const size_t nblocks = nsplits * (size_t)cdiv(nw, W3_THREADS);
    CSD_REQUIRE(nblocks < ((size_t)1 << 31), "conv3d_wgrad: %zu workgroups exceed the grid", nblocks);
    hipLaunchKernelGGL(conv3d_wgrad_f32_kernel, dim3((unsigned)nblocks), dim3(W3_THREADS), 0, s, a);
    CSD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(conv3d_wgrad_reduce_kernel, dim3((unsigned)cdiv(nw, 256)), dim3(256), 0, s, a.partial, dw, (int)nsplits, Cin, Cout, beta, ci_off, Cin_dw);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

extern "C" size_t csd_conv3d_dgrad_scale_scratch_bytes(int B) {
  return B < 1 ? 0 : scratch_aligned_bytes((size_t)B * DG_CHUNKS * sizeof(float));
}

extern "C" int csd_conv3d_dgrad_scale(const float* dy, float* rowscale, float* nscale, float* nshift, int B, int64_t per_sample, int C,
                                      void* scratch, void* stream) {
  CSD_REQUIRE(dy && rowscale && nscale && nshift && scratch, "conv3d_dgrad_scale: null argument");
  CSD_REQUIRE(B >= 1 && B < 65536 && per_sample >= 1 && C >= 1, "conv3d_dgrad_scale: bad shape B=%d per_sample=%lld C=%d", B,
              (long long)per_sample, C);
  hipStream_t s = (hipStream_t)stream;
  float* part = scratch_aligned<float>(scratch);
  const int nchunk = (int)std::min<int64_t>(DG_CHUNKS, cdiv64(per_sample, 256 * 8));
  hipLaunchKernelGGL(absmax_partial_kernel, dim3((unsigned)nchunk, (unsigned)B), dim3(256), 0, s, dy, part, per_sample);
  CSD_LAUNCH_CHECK();
  hipLaunchKernelGGL(dgrad_scale_finalize_kernel, dim3((unsigned)B), dim3(64), 0, s, part, nchunk, rowscale, nscale, nshift, C);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}
