// conv3d.hip - the 3-D operators of the ddpm3D score networks (reference models/ddpm3D.py, models/layers.py:119-132,607-675 with dim = 3):
// a 3x3x3 stride-1 pad-1 convolution with the ResnetBlock prologue / epilogue fused, 2x2x2 average pooling, nearest x2 upsampling and the
// GroupNorm statistics as per-(sample, channel) scale / shift.  Activations are channels-last fp32 [B, D, H, W, C].
//
// csd_conv3d_block as an implicit GEMM on the gfx950 fp16 matrix cores (v_mfma_f32_32x32x16_f16, fp32 accumulate) in the F16X3
// arithmetic conv_f16_kernel.h documents: every operand is hi + lo fp16, each product is ah*bh + ah*bl + al*bh, weights are pre-scaled
// by 2^8 at pack time and the epilogue multiplies by 2^-8.
//   * a workgroup (4 waves) owns a brick of 128 output voxels of ONE sample (4 x 8 x 4, or 8 x 8 x 2 where W < 3: the bottom levels
//     of a 96 x 96 x 16 volume are 12 x 12 x 2) x NT 32-cout tiles (NT = 1, 2, 4).  Wave w owns cout tile w % NT and the M tiles
//     (32 voxels each) of M group w / NT, so the four waves always cover 4 (M tile, cout tile) pairs each NT wide;
//   * the halo patch ((TD+2)(TH+2)(TW+2) voxels <= 400) of one 16-channel K chunk is staged in LDS once as fp16 hi | lo planes, 80 bytes
//     per voxel; the prologue act(x*nscale + nshift) and the split run while staging; a patch voxel outside the volume is written as
//     ZERO (not act(shift)), so the padding contributes exactly 0, and it is never read from memory;
//   * all 27 taps of the chunk are consumed from LDS (one ds_read_b128 per plane and M tile), the weights stream from L2 in
//     MFMA-fragment order through a 3-step register ring;
//   * the patch is double buffered: the next chunk's loads are issued before the chunk's MFMAs, converted and stored after them; one
//     barrier per chunk.
// Accumulation order is fixed (chunk, tap, product term) and a brick never spans two samples: the result is bitwise repeatable and does
// not depend on the sample's position in the batch.  No atomics.
// Layers whose channel count is not a multiple of 16 (the stem: 1 or 2 channels) and CSD_PREC_F32 (the exact yardstick: one fp32 fmaf
// chain per output in tap-major, channel-minor order) run on a direct kernel, one thread per (voxel, cout).
#include <hip/hip_fp16.h>

#include <string.h>

#include <algorithm>

#include "common.h"

namespace csd {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float v4f_t __attribute__((ext_vector_type(4)));

#define C3_THREADS 256
#define C3_TAPS 27
#define C3_KC 16                  // channels per K chunk = one MFMA K step per tap
#define C3_PSB 80                 // bytes per staged voxel: [hi 16 ch][lo 16 ch][16 pad]
#define C3_LO 32                  // byte offset of the lo plane
#define C3_NPIX 128               // output voxels per brick
#define C3_MAXPATCH 400           // (8+2)(8+2)(2+2); 6*10*6 = 360 for the 4 x 8 x 4 brick
#define C3_NSLOT ((C3_MAXPATCH * 4 + C3_THREADS - 1) / C3_THREADS)     // staging slots (4 channels of one voxel) per thread
#define C3_WSCALE 256.0f
#define C3_STEP_BYTES 2048        // one (chunk, tap) of one cout tile: [hi | lo][64 lanes][8 halves]
#define C3_BR 3                   // weight ring depth (divides 27: the ring index stays a compile-time constant)

struct Conv3dArgs {
  const float* x0;
  const float* x1;
  const void* wpack;
  const float* bias;
  const float* nscale;
  const float* nshift;
  const float* temb;
  const float* res;
  float* out;
  int temb_stride, act;
  float out_scale;
  int B, D, H, W, C0, C1, Cout;
  int TD, TH, TW, nbd, nbh, nbw;
  int nck, ntiles, n_groups;
};

__device__ __forceinline__ float act3(float v, int act) {
  switch (act) {
    case CSD_ACT_SWISH: return v * __frcp_rn(1.0f + __expf(-v));
    case CSD_ACT_RELU: return v > 0.f ? v : 0.f;
    case CSD_ACT_LRELU: return v > 0.f ? v : 0.2f * v;
    case CSD_ACT_ELU: return v > 0.f ? v : expm1f(v);
    default: return v;
  }
}

// the direct kernel (CSD_PREC_F32, the yardstick): the same activations with expf and a true division instead of the fast intrinsics
__device__ __forceinline__ float act3_exact(float v, int act) {
  if (act == CSD_ACT_SWISH) return v / (1.0f + expf(-v));
  return act3(v, act);
}

__device__ __forceinline__ float4 ld4(const float* p) {
  const v4f_t v = *(const __attribute__((address_space(1))) v4f_t*)(p);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ half8 ld_h8(const char* p) { return *(const __attribute__((address_space(1))) half8*)(p); }

// ---- weight packs ----------------------------------------------------------------------------------------------------------------
// MFMA: [cout tile][chunk][tap][hi | lo][lane][8 halves]; lane l feeds cout (l & 31) of the tile with channels 8*(l >> 5) + j of the chunk
// flip_t: w is the FORWARD layer's weight [Cin][Cout][27] and the pack is that of its data gradient's convolution, w[ci][co][26 - tap]:
// what packing weight.flip(2, 3, 4).transpose(0, 1) gives, without the copy
__device__ __forceinline__ size_t c3_widx(int co, int ci, int tap, int Cin, int Cout, int flip_t) {
  return flip_t ? ((size_t)ci * Cout + co) * C3_TAPS + (C3_TAPS - 1 - tap) : ((size_t)co * Cin + ci) * C3_TAPS + tap;
}
__global__ void conv3d_pack_mfma_kernel(const float* __restrict__ w, _Float16* __restrict__ wp, int Cin, int Cout, int nck, size_t total,
                                        int flip_t) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i & 7);
    const int lane = (int)((i >> 3) & 63);
    size_t r = i >> 9;
    const int tap = (int)(r % C3_TAPS); r /= C3_TAPS;
    const int ck = (int)(r % nck);
    const int tile = (int)(r / nck);
    const int co = tile * 32 + (lane & 31);
    const int ci = ck * C3_KC + 8 * (lane >> 5) + j;
    const float v = co < Cout ? w[c3_widx(co, ci, tap, Cin, Cout, flip_t)] * C3_WSCALE : 0.f;
    const _Float16 hi = (_Float16)v;
    const size_t step = ((size_t)tile * nck + ck) * C3_TAPS + tap;
    _Float16* dst = wp + step * (C3_STEP_BYTES / 2) + lane * 8 + j;
    dst[0] = hi;
    dst[512] = (_Float16)(v - (float)hi);
  }
}

// direct kernel: [tap][Cin][Cout] (threads of a wave read consecutive couts)
__global__ void conv3d_pack_direct_kernel(const float* __restrict__ w, float* __restrict__ wt, int Cin, int Cout, size_t total, int flip_t) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cout);
    size_t r = i / Cout;
    const int ci = (int)(r % Cin);
    const int tap = (int)(r / Cin);
    wt[i] = w[c3_widx(co, ci, tap, Cin, Cout, flip_t)];
  }
}

// ---- direct convolution: one thread per (voxel, cout), fp32 fmaf chain ---------------------------------------------------------------
__global__ __launch_bounds__(C3_THREADS) void conv3d_direct_kernel(const Conv3dArgs k) {
  const size_t vox = (size_t)k.D * k.H * k.W;
  const size_t total = (size_t)k.B * vox * k.Cout;
  const size_t idx = (size_t)blockIdx.x * C3_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int co = (int)(idx % k.Cout);
  const size_t v = idx / k.Cout;
  const int b = (int)(v / vox);
  const int vi = (int)(v - (size_t)b * vox);
  const int x = vi % k.W;
  const int h = (vi / k.W) % k.H;
  const int d = vi / (k.W * k.H);
  const int Cin = k.C0 + k.C1;
  const float* wt = static_cast<const float*>(k.wpack);
  const bool has_norm = k.nscale != nullptr;
  const float* sc = has_norm ? k.nscale + (size_t)b * Cin : nullptr;
  const float* sh = has_norm ? k.nshift + (size_t)b * Cin : nullptr;
  float acc = 0.f;
  for (int tap = 0; tap < C3_TAPS; ++tap) {
    const int dd = d + tap / 9 - 1, hh = h + (tap / 3) % 3 - 1, ww = x + tap % 3 - 1;
    if (dd < 0 || dd >= k.D || hh < 0 || hh >= k.H || ww < 0 || ww >= k.W) continue;      // zero padding AFTER the prologue
    const size_t sp = (size_t)b * vox + ((size_t)dd * k.H + hh) * k.W + ww;
    const float* wp = wt + (size_t)tap * Cin * k.Cout + co;
    const float* p0 = k.x0 + sp * k.C0;
    for (int ci = 0; ci < k.C0; ++ci) {
      float xv = p0[ci];
      if (has_norm) xv = act3_exact(xv * sc[ci] + sh[ci], k.act);
      acc = fmaf(xv, wp[(size_t)ci * k.Cout], acc);
    }
    if (k.C1 > 0) {
      const float* p1 = k.x1 + sp * k.C1;
      for (int ci = 0; ci < k.C1; ++ci) {
        float xv = p1[ci];
        if (has_norm) xv = act3_exact(xv * sc[k.C0 + ci] + sh[k.C0 + ci], k.act);
        acc = fmaf(xv, wp[(size_t)(k.C0 + ci) * k.Cout], acc);
      }
    }
  }
  float add = k.res ? k.res[idx] : 0.f;
  if (k.temb) add += k.temb[(size_t)b * k.temb_stride + co];
  k.out[idx] = ((acc + (k.bias ? k.bias[co] : 0.f)) + add) * k.out_scale;
}

// ---- input boundary + stem of the planned network (unet3d.h): x [B, Cx, D, H, W] and y [B, Cy, D, H, W] (NCDHW, y optional) -> the first
// 3x3x3 convolution's output [B, D, H, W, Cout].  The network input v = y + y_sigma * y_noise (y only, when y_noise is given), then 2v - 1
// unless `centered`, is formed per tap in registers (2v is exact, so the value equals the one a separate pass would store); the
// convolution restates conv3d_direct_kernel's chain: taps outer, channels inner, x channels before y channels, one fp32 fmaf chain, a tap
// outside the volume is skipped.  Weights in the direct layout [tap][Cin][Cout].
__global__ __launch_bounds__(C3_THREADS) void conv3d_stem_kernel(const float* __restrict__ xs, const float* __restrict__ ys,
                                                                 const float* __restrict__ yn, float ysig, const float* __restrict__ wt,
                                                                 const float* __restrict__ bias, float* __restrict__ out, int B, int Cx,
                                                                 int Cy, int Cout, int D, int H, int W, int centered) {
  const size_t vox = (size_t)D * H * W;
  const size_t total = (size_t)B * vox * Cout;
  const size_t idx = (size_t)blockIdx.x * C3_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int co = (int)(idx % Cout);
  const size_t v = idx / Cout;
  const int b = (int)(v / vox);
  const int vi = (int)(v - (size_t)b * vox);
  const int x = vi % W;
  const int h = (vi / W) % H;
  const int d = vi / (W * H);
  const int Cin = Cx + Cy;
  float acc = 0.f;
  for (int tap = 0; tap < C3_TAPS; ++tap) {
    const int dd = d + tap / 9 - 1, hh = h + (tap / 3) % 3 - 1, ww = x + tap % 3 - 1;
    if (dd < 0 || dd >= D || hh < 0 || hh >= H || ww < 0 || ww >= W) continue;
    const size_t sp = ((size_t)dd * H + hh) * W + ww;
    const float* wp = wt + (size_t)tap * Cin * Cout + co;
    for (int ci = 0; ci < Cx; ++ci) {
      float xv = xs[((size_t)b * Cx + ci) * vox + sp];
      if (!centered) xv = 2.f * xv - 1.f;
      acc = fmaf(xv, wp[(size_t)ci * Cout], acc);
    }
    for (int ci = 0; ci < Cy; ++ci) {
      const size_t j = ((size_t)b * Cy + ci) * vox + sp;
      float yv = ys[j];
      if (yn) yv = yv + yn[j] * ysig;
      if (!centered) yv = 2.f * yv - 1.f;
      acc = fmaf(yv, wp[(size_t)(Cx + ci) * Cout], acc);
    }
  }
  out[idx] = ((acc + (bias ? bias[co] : 0.f)) + 0.f) * 1.0f;      // (the direct kernel's epilogue without residual / temb, out_scale 1)
}

// ---- implicit GEMM on the fp16 matrix cores, split operands -----------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(C3_THREADS, 2) void conv3d_mfma_kernel(const Conv3dArgs k) {
  constexpr int MT = NT;               // M tiles per wave
  extern __shared__ __attribute__((aligned(16))) char smem3[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kg = lane >> 5;            // which 8 of the 16 K values this lane feeds
  const int wn = wave % NT;            // cout tile of this wave inside the group
  const int mg = wave / NT;            // M group

  int w = blockIdx.x;
  const int ng = w % k.n_groups; w /= k.n_groups;
  const int bw = w % k.nbw; w /= k.nbw;
  const int bh = w % k.nbh; w /= k.nbh;
  const int bd = w % k.nbd;
  const int b = w / k.nbd;
  const int d0 = bd * k.TD, h0 = bh * k.TH, w0 = bw * k.TW;
  const int PH = k.TH + 2, PW = k.TW + 2;
  const int npatch = (k.TD + 2) * PH * PW;
  const int patch_bytes = npatch * C3_PSB;
  char* const buf0 = smem3;
  char* const buf1 = smem3 + patch_bytes;
  int* const otab = reinterpret_cast<int*>(smem3 + 2 * patch_bytes);   // [128] output voxel index inside the sample, or -1
  int* const stab = otab + C3_NPIX;                                      // [npatch] source voxel index inside the sample, or -1

  if (tid < C3_NPIX) {
    const int tw = tid % k.TW;
    const int r = tid / k.TW;
    const int th = r % k.TH, td = r / k.TH;
    const int d = d0 + td, h = h0 + th, x = w0 + tw;
    otab[tid] = (d < k.D && h < k.H && x < k.W) ? (d * k.H + h) * k.W + x : -1;
  }
  for (int p = tid; p < npatch; p += C3_THREADS) {
    const int pw = p % PW;
    const int r = p / PW;
    const int ph = r % PH, pd = r / PH;
    const int d = d0 - 1 + pd, h = h0 - 1 + ph, x = w0 - 1 + pw;
    stab[p] = (d >= 0 && d < k.D && h >= 0 && h < k.H && x >= 0 && x < k.W) ? (d * k.H + h) * k.W + x : -1;
  }
  __syncthreads();

  // LDS byte offset of tap (0,0,0) of this lane's voxel in each of its M tiles (+ its K half)
  int base[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = (mg * MT + i) * 32 + (lane & 31);
    const int tw = m % k.TW;
    const int r = m / k.TW;
    const int th = r % k.TH, td = r / k.TH;
    base[i] = ((td * PH + th) * PW + tw) * C3_PSB + kg * 16;
  }
  const int sH = PW * C3_PSB, sD = PH * PW * C3_PSB;

  // ---- staging: slot e = j * 256 + tid is channels 4*(e & 3) .. +3 of patch voxel e >> 2; e & 3 == tid & 3 for every j ----
  const size_t vox = (size_t)k.D * k.H * k.W;
  const int Cin = k.C0 + k.C1;
  const int total4 = npatch * 4;
  const int sub = tid & 3;
  const bool has_norm = k.nscale != nullptr;
  float4 sv[C3_NSLOT], st_sc, st_sh;
  int sp[C3_NSLOT];
  auto stage_load = [&](int ck) {
    const int cb = ck * C3_KC;
    const float* src;
    int Cs, coff;
    if (cb < k.C0) { src = k.x0; Cs = k.C0; coff = cb; }
    else { src = k.x1; Cs = k.C1; coff = cb - k.C0; }
    src += (size_t)b * vox * Cs + coff + sub * 4;
    if (has_norm) {
      st_sc = ld4(k.nscale + (size_t)b * Cin + cb + sub * 4);
      st_sh = ld4(k.nshift + (size_t)b * Cin + cb + sub * 4);
    }
#pragma unroll
    for (int j = 0; j < C3_NSLOT; ++j) {
      const int e = j * C3_THREADS + tid;
      sp[j] = e < total4 ? stab[e >> 2] : -1;
      sv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (sp[j] >= 0) sv[j] = ld4(src + (size_t)sp[j] * Cs);
    }
  };
  auto stage_store = [&](char* buf) {
#pragma unroll
    for (int j = 0; j < C3_NSLOT; ++j) {
      const int e = j * C3_THREADS + tid;
      if (e >= total4) continue;
      float4 v = sv[j];
      if (has_norm && sp[j] >= 0) {          // a voxel outside the volume stays 0: the padding is applied after the prologue
        v.x = act3(v.x * st_sc.x + st_sh.x, k.act);
        v.y = act3(v.y * st_sc.y + st_sh.y, k.act);
        v.z = act3(v.z * st_sc.z + st_sh.z, k.act);
        v.w = act3(v.w * st_sc.w + st_sh.w, k.act);
      }
      char* dst = buf + (e >> 2) * C3_PSB + sub * 8;
      half4 hi, lo;
      hi[0] = (_Float16)v.x; hi[1] = (_Float16)v.y; hi[2] = (_Float16)v.z; hi[3] = (_Float16)v.w;
      lo[0] = (_Float16)(v.x - (float)hi[0]); lo[1] = (_Float16)(v.y - (float)hi[1]);
      lo[2] = (_Float16)(v.z - (float)hi[2]); lo[3] = (_Float16)(v.w - (float)hi[3]);
      *reinterpret_cast<half4*>(dst) = hi;
      *reinterpret_cast<half4*>(dst + C3_LO) = lo;
    }
  };

  floatx16 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // weight stream of this wave's cout tile (a wave beyond the last tile recomputes the last one and stores nothing)
  const int wtile = min(ng * NT + wn, k.ntiles - 1);
  const char* wstep = static_cast<const char*>(k.wpack) + (size_t)wtile * k.nck * C3_TAPS * C3_STEP_BYTES + lane * 16;
  half8 breg[C3_BR][2];
#pragma unroll
  for (int q = 0; q < C3_BR - 1; ++q)
#pragma unroll
    for (int p = 0; p < 2; ++p) breg[q][p] = ld_h8(wstep + (size_t)q * C3_STEP_BYTES + p * 1024);
  wstep += (size_t)(C3_BR - 2) * C3_STEP_BYTES;       // the newest prefetched step

  stage_load(0);
  stage_store(buf0);
  __syncthreads();

  for (int ck = 0; ck < k.nck; ++ck) {
    const char* buf = (ck & 1) ? buf1 : buf0;
    char* nbuf = (ck & 1) ? buf0 : buf1;
    const bool more = ck + 1 < k.nck;
    if (more) stage_load(ck + 1);
    half8 areg[2][2];
    auto load_frag = [&](int q) {        // q = tap * MT + i, compile-time after unrolling
      const int tap = q / MT, i = q % MT;
      const char* p = buf + base[i] + (tap / 9) * sD + ((tap / 3) % 3) * sH + (tap % 3) * C3_PSB;
      areg[q & 1][0] = *reinterpret_cast<const half8*>(p);
      areg[q & 1][1] = *reinterpret_cast<const half8*>(p + C3_LO);
    };
    load_frag(0);
#pragma unroll
    for (int tap = 0; tap < C3_TAPS; ++tap) {
      const int bc = tap % C3_BR, bn = (tap + C3_BR - 1) % C3_BR;
      wstep += C3_STEP_BYTES;           // (the last two steps of the last chunk read the slack behind the stream)
#pragma unroll
      for (int p = 0; p < 2; ++p) breg[bn][p] = ld_h8(wstep + p * 1024);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int q = tap * MT + i;
        if (q + 1 < C3_TAPS * MT) load_frag(q + 1);
        const half8 ah = areg[q & 1][0], al = areg[q & 1][1];
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, breg[bc][0], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, breg[bc][1], acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, breg[bc][0], acc[i], 0, 0, 0);
      }
    }
    if (more) stage_store(nbuf);
    __syncthreads();
  }

  // ---- epilogue: ((acc * 2^-8 + bias) + res + temb) * out_scale.  Buffer descriptors based at the sample: a lane whose voxel or cout does
  // not exist uses an out-of-range offset (the load returns 0, the store is dropped) ----
  const int col = (ng * NT + wn) * 32 + (lane & 31);
  const bool cv = col < k.Cout;
  const int colc = cv ? col : 0;
  const float bv = k.bias ? k.bias[colc] : 0.f;
  const float tv = k.temb ? k.temb[(size_t)b * k.temb_stride + colc] : 0.f;
  constexpr unsigned OOB = 0x80000000u;
  constexpr int RSRC_FLAGS = 0x00020000;
  const bool has_res = k.res != nullptr;
  const __amdgpu_buffer_rsrc_t out_r = __builtin_amdgcn_make_buffer_rsrc(k.out + (size_t)b * vox * k.Cout, 0, OOB, RSRC_FLAGS);
  const __amdgpu_buffer_rsrc_t res_r = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(has_res ? k.res + (size_t)b * vox * k.Cout : k.out), 0, OOB, RSRC_FLAGS);
  const float wunscale = 1.0f / C3_WSCALE;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    unsigned off[16];
    float addv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = otab[(mg * MT + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg];
      off[r] = (cv && o >= 0) ? (unsigned)(o * k.Cout + col) * 4u : OOB;
      addv[r] = 0.f;
    }
    if (has_res) {
#pragma unroll
      for (int r = 0; r < 16; ++r) addv[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(res_r, off[r], 0, 0));
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float val = ((acc[i][r] * wunscale + bv) + (addv[r] + tv)) * k.out_scale;
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), out_r, off[r], 0, 0);
    }
  }
}

template <int NT>
int conv3d_mfma_launch(const Conv3dArgs& a, int nblocks, size_t lds, hipStream_t s) {
  CSD_SET_MAX_LDS_ONCE(conv3d_mfma_kernel<NT>);
  hipLaunchKernelGGL(conv3d_mfma_kernel<NT>, dim3(nblocks), dim3(C3_THREADS), lds, s, a);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

size_t mfma_pack_bytes(int Cin, int Cout) {
  const size_t nck = (size_t)cdiv(Cin, C3_KC), ntiles = (size_t)cdiv(Cout, 32);
  return (ntiles * nck * C3_TAPS + C3_BR) * C3_STEP_BYTES;        // + slack for the ring's reads past the last step
}

// ---- small operators -------------------------------------------------------------------------------------------------------------------
__global__ void avgpool3d_2_kernel(const float* __restrict__ in, float* __restrict__ out, int D, int H, int W, int C, size_t total) {
  const int OD = D >> 1, OH = H >> 1, OW = W >> 1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t r = i / C;
    const int ox = (int)(r % OW); r /= OW;
    const int oy = (int)(r % OH); r /= OH;
    const int oz = (int)(r % OD);
    const size_t b = r / OD;
    const float* p = in + (((b * D + 2 * oz) * H + 2 * oy) * W + 2 * ox) * C + c;
    const size_t sW = C, sH = (size_t)W * C, sD = (size_t)H * W * C;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) s += p[(t >> 2) * sD + ((t >> 1) & 1) * sH + (t & 1) * sW];
    out[i] = s * 0.125f;
  }
}

__global__ void nearest_up2_3d_kernel(const float* __restrict__ in, float* __restrict__ out, int D, int H, int W, int C, size_t total) {
  const int OD = D * 2, OH = H * 2, OW = W * 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t r = i / C;
    const int ox = (int)(r % OW); r /= OW;
    const int oy = (int)(r % OH); r /= OH;
    const int oz = (int)(r % OD);
    const size_t b = r / OD;
    out[i] = in[(((b * D + (oz >> 1)) * H + (oy >> 1)) * W + (ox >> 1)) * C + c];
  }
}

}  // namespace

// ---- the pieces of csd_conv3d_block for a caller that keeps packed weights (the planned 3-D network, unet3d.h) ------------------------
bool conv3d_is_direct(int precision, int C0) { return precision == CSD_PREC_F32 || C0 % 16 != 0; }

size_t conv3d_wpack_size(int Cin, int Cout, bool direct) {
  return direct ? (size_t)C3_TAPS * Cin * Cout * sizeof(float) : mfma_pack_bytes(Cin, Cout);
}

int conv3d_pack_launch(const float* weight, void* wpack, int Cin, int Cout, bool direct, hipStream_t s, bool flip_t) {
  if (direct) {
    const size_t nw = (size_t)C3_TAPS * Cin * Cout;
    hipLaunchKernelGGL(conv3d_pack_direct_kernel, dim3((unsigned)std::min<size_t>(cdiv64(nw, 256), 4096)), dim3(256), 0, s, weight,
                       static_cast<float*>(wpack), Cin, Cout, nw, flip_t ? 1 : 0);
    CSD_LAUNCH_CHECK();
    return CSD_OK;
  }
  const int nck = Cin / C3_KC, ntiles = cdiv(Cout, 32);
  const size_t nh = (size_t)ntiles * nck * C3_TAPS * 512;
  hipLaunchKernelGGL(conv3d_pack_mfma_kernel, dim3((unsigned)std::min<size_t>(cdiv64(nh, 256), 4096)), dim3(256), 0, s, weight,
                     static_cast<_Float16*>(wpack), Cin, Cout, nck, nh, flip_t ? 1 : 0);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

int conv3d_launch(const Conv3dCall& c, hipStream_t s) {
  const int Cin = c.C0 + c.C1;
  const size_t vox = (size_t)c.D * c.H * c.W;
  Conv3dArgs a;
  memset(&a, 0, sizeof(a));
  a.x0 = c.x0; a.x1 = c.x1; a.wpack = c.wpack; a.bias = c.bias; a.nscale = c.nscale; a.nshift = c.nshift; a.temb = c.temb; a.res = c.res;
  a.out = c.out;
  a.temb_stride = c.temb_stride; a.act = c.act; a.out_scale = c.out_scale;
  a.B = c.B; a.D = c.D; a.H = c.H; a.W = c.W; a.C0 = c.C0; a.C1 = c.C1; a.Cout = c.Cout;

  if (conv3d_is_direct(c.precision, c.C0)) {      // exact yardstick; thin layers (the stem)
    const size_t total = (size_t)c.B * vox * c.Cout;
    const size_t nb = cdiv64(total, C3_THREADS);
    CSD_REQUIRE(nb < ((size_t)1 << 31), "conv3d_block: %zu outputs exceed the direct kernel's grid", total);
    hipLaunchKernelGGL(conv3d_direct_kernel, dim3((unsigned)nb), dim3(C3_THREADS), 0, s, a);
    CSD_LAUNCH_CHECK();
    return CSD_OK;
  }

  a.nck = Cin / C3_KC;
  a.ntiles = cdiv(c.Cout, 32);
  const int NT = a.ntiles >= 3 ? 4 : a.ntiles;
  a.n_groups = cdiv(a.ntiles, NT);
  if (c.W >= 3) { a.TD = 4; a.TH = 8; a.TW = 4; }
  else { a.TD = 8; a.TH = 8; a.TW = 2; }
  a.nbd = cdiv(c.D, a.TD); a.nbh = cdiv(c.H, a.TH); a.nbw = cdiv(c.W, a.TW);
  const size_t nblocks = (size_t)c.B * a.nbd * a.nbh * a.nbw * a.n_groups;
  CSD_REQUIRE(nblocks < ((size_t)1 << 31), "conv3d_block: %zu workgroups exceed the grid", nblocks);
  const int npatch = (a.TD + 2) * (a.TH + 2) * (a.TW + 2);
  const size_t lds = (size_t)2 * npatch * C3_PSB + (size_t)(C3_NPIX + npatch) * sizeof(int);
  switch (NT) {
    case 1: return conv3d_mfma_launch<1>(a, (int)nblocks, lds, s);
    case 2: return conv3d_mfma_launch<2>(a, (int)nblocks, lds, s);
    default: return conv3d_mfma_launch<4>(a, (int)nblocks, lds, s);
  }
}

int conv3d_stem_launch(const float* x, const float* y, const float* y_noise, float y_sigma, const void* wpack, const float* bias, float* out,
                       int B, int Cx, int Cy, int Cout, int D, int H, int W, int centered, hipStream_t s) {
  const size_t total = (size_t)B * D * H * W * Cout;
  const size_t nb = cdiv64(total, C3_THREADS);
  CSD_REQUIRE(nb >= 1 && nb < ((size_t)1 << 31), "conv3d_stem: %zu outputs exceed the kernel's grid", total);
  hipLaunchKernelGGL(conv3d_stem_kernel, dim3((unsigned)nb), dim3(C3_THREADS), 0, s, x, y, y_noise, y_sigma, static_cast<const float*>(wpack),
                     bias, out, B, Cx, Cy, Cout, D, H, W, centered);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

}  // namespace csd

using namespace csd;

extern "C" size_t csd_conv3d_block_scratch_bytes(int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0) return 0;
  return scratch_aligned_bytes(std::max(mfma_pack_bytes(Cin, Cout), (size_t)C3_TAPS * Cin * Cout * sizeof(float)), kScratchPrefetchSlack);
}

extern "C" int csd_conv3d_block(const float* x0, const float* x1, const float* weight, const float* bias, const float* nscale,
                                const float* nshift, int act, const float* temb, int temb_stride, const float* res, float out_scale,
                                float* y, int B, int C0, int C1, int Cout, int D, int H, int W, int precision, void* scratch,
                                void* stream) {
  CSD_REQUIRE(x0 && weight && y && scratch, "conv3d_block: null argument");
  CSD_REQUIRE(precision == CSD_PREC_F16X3 || precision == CSD_PREC_F32,
              "conv3d_block: precision must be fp16x3 (CSD_PREC_F16X3) or fp32 (CSD_PREC_F32); fp16 and fp16f8 are not provided in 3-D");
  CSD_REQUIRE(B >= 1 && D >= 1 && H >= 1 && W >= 1 && C0 >= 1 && C1 >= 0 && Cout >= 1, "conv3d_block: bad shape B=%d %dx%dx%d C=%d+%d->%d",
              B, D, H, W, C0, C1, Cout);
  CSD_REQUIRE((x1 != nullptr) == (C1 > 0), "conv3d_block: x1 and C1 = %d do not agree", C1);
  CSD_REQUIRE(C1 == 0 || (C0 % 16 == 0 && C1 % 16 == 0), "conv3d_block: a two-source (virtual concat) layer needs C0 and C1 multiples of 16 (got %d + %d)",
              C0, C1);
  CSD_REQUIRE((nscale != nullptr) == (nshift != nullptr), "conv3d_block: nscale and nshift come together");
  CSD_REQUIRE(act >= CSD_ACT_NONE && act <= CSD_ACT_ELU, "conv3d_block: unknown activation id %d", act);
  CSD_REQUIRE(temb == nullptr || temb_stride >= Cout, "conv3d_block: temb_stride %d < Cout %d", temb_stride, Cout);
  const int Cin = C0 + C1;
  const size_t vox = (size_t)D * H * W;
  CSD_REQUIRE(vox * (size_t)std::max(Cin, Cout) * sizeof(float) < ((size_t)1 << 31) && vox < ((size_t)1 << 28),
              "conv3d_block: one sample (%dx%dx%d voxels, %d channels) exceeds the kernel's 2 GiB per-sample addressing", D, H, W, std::max(Cin, Cout));
  hipStream_t s = (hipStream_t)stream;
  void* wpack = scratch_aligned<void>(scratch);
  Conv3dCall c;
  c.x0 = x0; c.x1 = x1; c.wpack = wpack; c.bias = bias; c.nscale = nscale; c.nshift = nshift; c.temb = temb; c.res = res; c.out = y;
  c.temb_stride = temb_stride; c.act = act; c.out_scale = out_scale;
  c.B = B; c.C0 = C0; c.C1 = C1; c.Cout = Cout; c.D = D; c.H = H; c.W = W; c.precision = precision;
  const int rc = conv3d_pack_launch(weight, wpack, Cin, Cout, conv3d_is_direct(precision, C0), s);
  if (rc) return rc;
  return conv3d_launch(c, s);
}

extern "C" int csd_avgpool3d_2_ndhwc(const float* x, float* out, int B, int D, int H, int W, int C, void* stream) {
  CSD_REQUIRE(D >= 2 && H >= 2 && W >= 2 && D % 2 == 0 && H % 2 == 0 && W % 2 == 0, "avgpool3d_2: extents %dx%dx%d must be even", D, H, W);
  CSD_REQUIRE(x && out && B >= 1 && C >= 1, "avgpool3d_2: bad arguments");
  const size_t total = (size_t)B * (D / 2) * (H / 2) * (W / 2) * C;
  hipLaunchKernelGGL(avgpool3d_2_kernel, dim3((unsigned)std::min<size_t>(cdiv64(total, 256), 16384)), dim3(256), 0, (hipStream_t)stream, x, out,
                     D, H, W, C, total);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

extern "C" int csd_nearest_up2_3d_ndhwc(const float* x, float* out, int B, int D, int H, int W, int C, void* stream) {
  CSD_REQUIRE(x && out && B >= 1 && D >= 1 && H >= 1 && W >= 1 && C >= 1, "nearest_up2_3d: bad arguments");
  const size_t total = (size_t)B * D * 2 * H * 2 * W * 2 * C;
  hipLaunchKernelGGL(nearest_up2_3d_kernel, dim3((unsigned)std::min<size_t>(cdiv64(total, 256), 16384)), dim3(256), 0, (hipStream_t)stream, x,
                     out, D, H, W, C, total);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

// GroupNorm statistics only: nscale / nshift [B, C0 + C1] = rstd*gamma and beta - mean*rstd*gamma of x = x0 (| x1) on [B, S, C]
extern "C" size_t csd_groupnorm_scale_shift_scratch_bytes(int B, int C, int S, int groups) {
  GNPlan g;
  if (B < 1 || S < 1 || gn_plan(&g, B, S, C, 0, groups)) return 0;
  return scratch_aligned_bytes(gn_partial_bytes(g));
}

extern "C" int csd_groupnorm_scale_shift(const float* x0, const float* x1, const float* gamma, const float* beta, float* nscale,
                                         float* nshift, int B, int C0, int C1, int S, int groups, float eps, void* scratch, void* stream) {
  CSD_REQUIRE(x0 && gamma && beta && nscale && nshift && scratch && B >= 1 && S >= 1, "groupnorm_scale_shift: bad arguments");
  CSD_REQUIRE((x1 != nullptr) == (C1 > 0), "groupnorm_scale_shift: x1 and C1 = %d do not agree", C1);
  GNPlan g;
  int rc = gn_plan(&g, B, S, C0, C1, groups);
  if (rc) return rc;
  double* partial = scratch_aligned<double>(scratch);
  if ((rc = gn_stats_launch(g, x0, x1, partial, (hipStream_t)stream))) return rc;
  return gn_finalize_launch(g, partial, gamma, beta, eps, nscale, nshift, (hipStream_t)stream);
}
