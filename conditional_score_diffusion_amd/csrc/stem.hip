// stem.hip - the DDPM-family network's first layer as ONE launch (gfx950): cat(x, y [+ sigma * z]), the 2v - 1 data centering, the
// NCHW -> NHWC layout change and the 3 x 3 convolution of the <= 8 assembled channels to nf channels, with the next GroupNorm's tile
// partials in the epilogue (models/ddpm.py:163-168 + :283 + the conv3x3 of :95; sampling/conditional.py:104-110).
//
// Replaces assemble_input_kernel (83 us at 160^2, B = 64) + the generic fp16 conv on a 16-channel padded copy (310 us): the layer is
// bound by its 629 MB of output, so the whole input side (6 of 8 channels real, 0.1 GB) is done inside the tile that needs it.
//
// Persistent: four 4-wave workgroups per CU, each walking 16 x 8 pixel tiles of its XCD's contiguous share (one 32-pixel M tile per wave:
// <= 128 VGPRs).  The packed weights of ALL cout groups (2^8-scaled hi + lo A/B fragments, 30 KB for 96 couts) and the bias stay in LDS for
// the workgroup's run.  Per tile the 18 x 10 patch is read from the NCHW sources (coalesced along W, straight-line loads), assembled, split
// into fp16 hi + lo ONCE per patch pixel and kept as two 16-byte planes in LDS; K = tap * 8 + channel (72, padded to 80 = 5 MFMA K steps;
// the padding tap reads a zero pixel).  Products: hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 (NS = 2: the fp16x3 / fp16f8 modes - the
// raw inputs are not GroupNorm-ed, so the e4m3 correction form does not apply) or hi*hi only (NS = 1: the plain fp16 mode); the pixels are
// the M operand, so every output store covers whole 128-byte lines.  The loop's only wait on global memory (the next tile's patch, requested
// before the K loop) sits after the K loop: gfx9's in-order vmcnt makes a load wait also a wait for every older store.
//
// stem_wide_kernel (below) is the same layer for 9 .. 32 assembled channels, padded to Cpad = 16 or 32: K = tap * Cpad + channel, one or
// two MFMA K steps per tap.
//
// SQ (a compile-time variant of both kernels; csd_unet_config.x_squeeze, the 2x super-resolution networks): x is the HIGH-resolution
// image [B, Cx / 4, 2S, 2S] and channel 4 ci + 2 dy + dx of patch pixel (gy, gx) is its pixel (2 gy + dy, 2 gx + dx) - pure addressing,
// the dx pair read as one aligned 8-byte load (a wave still covers whole lines of the image rows it touches).  Out-of-image patch
// pixels stay masked zeros.  The SQ = false instantiations are the code they were.
//
// YS (a compile-time variant of stem_kernel; csd_unet_config.y_scale = K, the direct Kx super-resolution networks): y and its noise are
// LOW-resolution [B, Cy <= 4, S / K, S / K] (and Cx <= 4) and a y channel of patch pixel (gy, gx) is the bilinear upsample there (common.h: bilin_up_tap,
// bilin_perturb, bilin_combine - the functions of the assemble pass and of csd_bilinear_up, so the value does not depend on the route).
// The four taps per channel are REQUESTED in load_pixel like every other source value and combined in write_patch; a sample's
// low-resolution planes are a few KB and stay in L2.  No full-resolution copy of y exists.  The perturbation of a sampling step,
// y + sigma z at LOW resolution, is one small launch in front (bilinear_perturb_launch into the plan's scratch plane): holding the noise
// taps as well does not fit the 128 registers of this kernel's occupancy, so YS exists with YN = false only.  x comes from ONE uniform
// base + a 32-bit offset per channel (as SQ reads y).  The YS = false instantiations are the code they were.
#include <hip/hip_runtime.h>

#include "common.h"
#include "conv_ff.h"

namespace csd {

struct StemArgs {
  const float *x, *y, *yn;
  float ysig;
  const _Float16* w;
  const float* bias;
  float* out;
  double* stats;
  int B, S, Cx, Cy, Cout, tiles_x, tpi, n_groups, nblocks, centered;
  int ys = 0;   // YS: csd_unet_config.y_scale
  int abl;      // tuning aid (tune build, CSD_STEM_ABL): 1 no output stores, 2 no statistics, 4 no source loads, 8 no MFMAs
};

#define ST_PW 18
#define ST_PH 10
#define ST_TH 8                 // tile height (width 16)
#define ST_NPIX (ST_PW * ST_PH)
#define ST_ZERO ST_NPIX            // index of the all-zero pixel (the padding tap)
#define ST_PLANE 184               // pixels per LDS plane
#define ST_KSTEPS 5

template <int NT, int NS, bool YN, bool SQ, bool YS>
__global__ __launch_bounds__(256, 4) void stem_kernel(const StemArgs k) {
  static_assert(!(YS && (YN || SQ)), "stem_kernel: YS excludes YN (the perturbation is a launch in front) and SQ");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  half8* const phi = reinterpret_cast<half8*>(smem);
  half8* const plo = phi + ST_PLANE;
  float* const red = reinterpret_cast<float*>(smem + 2 * ST_PLANE * 16);      // [4 waves][NT * 32 couts][2]
  half8* const wl = reinterpret_cast<half8*>(smem + 2 * ST_PLANE * 16 + 4 * NT * 32 * 2 * 4);      // all cout groups' weight fragments
  float* const bl = reinterpret_cast<float*>(wl + k.n_groups * ST_KSTEPS * NT * NS * 64);           // bias [Cout]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kh = lane >> 5, p32 = lane & 31;
  const int S = k.S, Cx = k.Cx, Cy = k.Cy, Cout = k.Cout, n_groups = k.n_groups;
  const size_t HW = (size_t)S * S;
#ifdef CSD_TUNE
#define ST_ABL(bit) (k.abl & (bit))
#else
#define ST_ABL(bit) false
#endif

  // ---- persistent tile loop: workgroup p of gridDim.x (four per CU) runs the tiles j, j + P/8, ... of its XCD's contiguous share of the
  // launch (block p lands on XCD p % 8: neighbouring tiles of the same samples share their halo rows in one L2) ----
  const int xcd = blockIdx.x & 7, wj = blockIdx.x >> 3, wstride = gridDim.x >> 3;
  const int xq = k.nblocks >> 3, xr = k.nblocks & 7;
  const int x_start = xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq, x_len = xq + (xcd < xr ? 1 : 0);
  if (wj >= x_len) return;

  // the packed weights stay in LDS for the workgroup's whole run (30 KB at 96 couts: re-reading them from L2 per tile and wave was
  // 1.5 GB per launch, more than twice the layer's output)
  {
    const int n16 = n_groups * ST_KSTEPS * NT * NS * 64;
    wg_copy_to_lds<256, 8>(reinterpret_cast<char*>(wl), reinterpret_cast<const char*>(k.w), n16 * 16, tid);
  }

  // the assembled values of a patch pixel (thread t < 184 owns patch pixel t of every tile).  Straight-line on purpose: every load is
  // unconditional (absent channels and out-of-image pixels read a valid dummy address and are replaced by a select) - with branches
  // around the loads hipcc put an s_waitcnt vmcnt(0) behind each of them, which on gfx9's in-order counter also waits for the previous
  // tile's 48 output stores (measured: 116 of the kernel's 250 us)
  const int py = tid / ST_PW, px = tid - (tid / ST_PW) * ST_PW;
  const float* cp[8];
  const float* cn[8];
  size_t cs[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool isx = c < Cx, isy = !isx && c < Cx + Cy;
    // (YS: the y channels are not read at S x S - a dummy load here, their taps below)
    cp[c] = isx ? k.x + (size_t)c * HW : ((isy && !YS) ? k.y + (size_t)(c - Cx) * HW : k.x);
    cn[c] = (YN && isy && !YS) ? k.yn + (size_t)(c - Cx) * HW : k.x;
    cs[c] = isx ? (size_t)Cx * HW : ((isy && !YS) ? (size_t)Cy * HW : 0);
  }
  const int ylo = YS ? S / k.ys : 0;      // YS: side of the low-resolution planes
  // SQ (Cx == 4: one image channel): x channels 2 dy, 2 dy + 1 are one float2 of image row 2 gy + dy; channels 4 .. 7 are y or absent
  const float2* const xp0 = reinterpret_cast<const float2*>(k.x);
  // load_pixel only REQUESTS the values (raw registers); finish_pixel - called where the wait belongs - assembles them
  struct Raw { float x[8], n[8]; float2 p[2]; float t[4][4], wx, wy; int w; bool inimg; };      // (p: SQ only; t, wx, wy: YS only; w: LATE only)
  // sample b and image position (gy, gx) of this thread's patch pixel in tile w (LATE: write_patch finds the tile of its raw values)
  auto patch_origin = [&](int w, int& b, int& gy, int& gx) __attribute__((always_inline)) {
    b = w / k.tpi;
    const int tin = w - b * k.tpi;
    const int ty0 = (tin / k.tiles_x) * ST_TH, tx0 = (tin - (tin / k.tiles_x) * k.tiles_x) * 16;
    gy = ty0 + py - 1; gx = tx0 + px - 1;
  };
  // YS: the four taps of y channel j < Cy <= 4 (absent channels and out-of-image pixels read element 0 and are never used).  NT = 2:
  // requested with the rest of the patch, before the K loop.  NT = 3 (LATE): the 16 tap registers do not fit beside three accumulator
  // tiles (64 bytes of scratch per lane when held across the K loop), so they are requested in write_patch, behind the K loop, where the
  // youngest older stores are a whole K loop old - one exposed L2 round trip per tile, shared with three other workgroups of the CU.
  constexpr bool LATE = YS && NT == 3;
  auto load_taps = [&](int gy, int gx, int b, Raw& r) __attribute__((always_inline)) {
    const BilinTap ty = bilin_up_tap(r.inimg ? gy : 0, k.ys, ylo), tx = bilin_up_tap(r.inimg ? gx : 0, k.ys, ylo);
    r.wx = tx.w1; r.wy = ty.w1;
    const unsigned o4[4] = {(unsigned)(ty.i0 * ylo + tx.i0), (unsigned)(ty.i0 * ylo + tx.i1), (unsigned)(ty.i1 * ylo + tx.i0),
                            (unsigned)(ty.i1 * ylo + tx.i1)};
    const unsigned lo2 = (unsigned)(ylo * ylo);
    const float* const yb = k.y + (size_t)b * Cy * lo2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned cb = j < Cy ? (unsigned)j * lo2 : 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) r.t[j][q] = yb[cb + o4[q]];
    }
  };
  auto load_pixel = [&](int w, Raw& r) __attribute__((always_inline)) {
    // (the arithmetic of patch_origin, spelled out as it always was: routing this through the lambda changed the register allocation of
    // the existing instantiations - one spilled VGPR in stem_kernel<3, 1, false, false>)
    const int b = w / k.tpi, tin = w - b * k.tpi;
    const int ty0 = (tin / k.tiles_x) * ST_TH, tx0 = (tin - (tin / k.tiles_x) * k.tiles_x) * 16;
    const int gy = ty0 + py - 1, gx = tx0 + px - 1;
    if (LATE) r.w = w;      // (uniform: a scalar register; write_patch requests the taps of the SAME tile from it)
    r.inimg = !ST_ABL(4) && tid < ST_NPIX && (unsigned)gy < (unsigned)S && (unsigned)gx < (unsigned)S;      // (zero padding applies to the
    const unsigned pix = r.inimg ? (unsigned)(gy * S + gx) : 0u;                                              // ASSEMBLED tensor: 0, not -1)
    // (uniform 64-bit base + 32-bit lane offset: the saddr form of global_load - one address register for all the loads)
    if (SQ) {
      const unsigned pix2 = r.inimg ? (unsigned)(2 * gy * S + gx) : 0u;      // float2 index of image pixel (2 gy, 2 gx): (4 gy S + 2 gx) / 2
      r.p[0] = (xp0 + (size_t)b * (2 * HW))[pix2];
      r.p[1] = (xp0 + (size_t)b * (2 * HW))[pix2 + (unsigned)S];      // (image row 2 gy + 1: 2S floats on)
      // (y from ONE uniform base + a 32-bit offset per channel: the eight 64-bit channel pointers of the plain variant would not fit
      // the scalar registers beside the image pointers)
      const float* const yb = (Cy ? k.y : k.x) + (size_t)b * Cy * HW;
#pragma unroll
      for (int c = 4; c < 8; ++c) r.x[c] = yb[pix + (c - 4 < Cy ? (unsigned)(c - 4) * (unsigned)HW : 0u)];
      if (YN) {
        const float* const nb = k.yn + (size_t)b * Cy * HW;
#pragma unroll
        for (int c = 4; c < 8; ++c) r.n[c] = nb[pix + (c - 4 < Cy ? (unsigned)(c - 4) * (unsigned)HW : 0u)];
      }
    } else if (YS) {
      const float* const xb = k.x + (size_t)b * Cx * HW;
#pragma unroll
      for (int c = 0; c < 4; ++c) r.x[c] = xb[pix + (c < Cx ? (unsigned)c * (unsigned)HW : 0u)];      // (YS: Cx <= 4)
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) r.x[c] = (cp[c] + (size_t)b * cs[c])[pix];
    }
    if (YN && !SQ && !YS) {
#pragma unroll
      for (int c = 0; c < 8; ++c) r.n[c] = (cn[c] + (size_t)b * cs[c])[pix];
    }
    if (YS && !LATE) load_taps(gy, gx, b, r);
  };
  auto write_patch = [&](Raw& r) __attribute__((always_inline)) {      // assemble, split once: plane hi [pixel][8 ch], plane lo [pixel][8 ch]
    if (LATE) {      // (the taps of the tile load_pixel filled r for)
      int b, gy, gx;
      patch_origin(r.w, b, gy, gx);
      load_taps(gy, gx, b, r);
    }
    if (tid < ST_PLANE) {
      half8 h, l;
      float yv[4];
      if (YS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) yv[j] = bilin_combine(r.t[j][0], r.t[j][1], r.t[j][2], r.t[j][3], r.wx, r.wy);
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float t = (SQ && c < 4) ? ((c & 1) ? r.p[c >> 1].y : r.p[c >> 1].x) : ((YS && c >= 4) ? 0.f : r.x[c]);
        if (YS) {
#pragma unroll
          for (int j = 0; j < 4; ++j) t = (c == Cx + j) ? yv[j] : t;
        }
        if (YN && !YS && !(SQ && c < 4)) t = (c >= Cx && c < Cx + Cy) ? t + r.n[c] * k.ysig : t;
        t = k.centered ? t : 2.f * t - 1.f;
        const float v = (r.inimg && c < Cx + Cy) ? t : 0.f;
        h[c] = (_Float16)v;
        l[c] = (_Float16)(v - (float)h[c]);
      }
      phi[tid] = h;
      if (NS == 2) plo[tid] = l;
    }
  };
  Raw vn;
  load_pixel(x_start + wj, vn);
  for (int i = tid; i < Cout; i += 256) bl[i] = k.bias[i];
  write_patch(vn);
  const int pix0 = (wave * 2 + (p32 >> 4)) * ST_PW + (p32 & 15);
  const float wunscale = 1.0f / C16_WSCALE;
  ff_barrier();

  // Per tile: request the NEXT tile's patch -> K loop -> barrier -> convert + write the next patch -> output stores -> statistics.
  // gfx9 counts loads and stores on ONE in-order counter, so a wait for a load also waits for every store issued before it: the only
  // vmcnt wait of the loop (the patch conversion) sits where the youngest older stores are a whole K loop old, and nothing else in the
  // loop reads global memory (bias and weights live in LDS).  ff_barrier: LDS hand-over without a release fence (__syncthreads() drains
  // vmcnt(0) - the tile's output stores - at every barrier).
  for (int local = wj; local < x_len; local += wstride) {
    const int tile = x_start + local;
    const int b = tile / k.tpi, tin = tile - b * k.tpi;
    const int ty0 = (tin / k.tiles_x) * ST_TH, tx0 = (tin - (tin / k.tiles_x) * k.tiles_x) * 16;
    const bool more = local + wstride < x_len;
    if (more) load_pixel(tile + wstride, vn);

    for (int ng = 0; ng < n_groups; ++ng) {
      // ---- K loop: 5 steps of 16 = 2 taps x 8 channels; lanes of K half kh read tap 2s + kh ----
      floatx16 acc[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
      const half8* const wq = wl + (size_t)ng * ST_KSTEPS * NT * NS * 64 + lane;
#pragma unroll
      for (int s = 0; s < ST_KSTEPS; ++s) {
        constexpr int kNoTap = -1;
        const int t0 = 2 * s, t1 = 2 * s + 1;
        const int off0 = (t0 / 3) * ST_PW + t0 % 3;
        const int off1 = t1 < 9 ? (t1 / 3) * ST_PW + t1 % 3 : kNoTap;
        const int idx = kh ? (off1 == kNoTap ? ST_ZERO : pix0 + off1) : pix0 + off0;
        const half8 bh = phi[idx];
        half8 bl16;
        if (NS == 2) bl16 = plo[idx];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          if (ST_ABL(8)) continue;
          const half8 wh = wq[((s * NT + nt) * NS) * 64];
          if (NS == 2) {      // small products first
            const half8 wlo = wq[((s * NT + nt) * NS + NS - 1) * 64];
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, wlo, acc[nt], 0, 0, 0);
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl16, wh, acc[nt], 0, 0, 0);
          }
          acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, wh, acc[nt], 0, 0, 0);
        }
      }
      if (ng == n_groups - 1) {
        ff_barrier();                    // every wave has read this tile's patch (and the previous partials in red)
        if (more) write_patch(vn);
      } else {
        ff_barrier();                    // (several cout groups: the previous group's partials in red have been read)
      }

      // ---- epilogue: un-scale, bias, NHWC stores.  The pixels are the MFMA's M operand, so a lane holds ONE cout (ng * 32 NT + nt * 32 +
      //      lane % 32) of 16 pixels (register r = pixel 8 (r / 4) + 4 kh + r % 4 of the wave's 32): every store instruction writes two
      //      whole 128-byte lines (tools/probes/store_probe.hip: 5.4 TB/s against 3.3 TB/s for 16-byte pieces of four different instructions) ----
      const int c_lane = ng * NT * 32 + p32;
      float* const obase = k.out + (((size_t)b * S + ty0 + wave * 2) * S + tx0) * Cout + ng * NT * 32;      // uniform
      const unsigned lane_off = (unsigned)(4 * kh * Cout + p32);                                            // + one lane offset: saddr stores
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float bv = bl[c_lane + nt * 32];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float* const ub = obase + ((size_t)(r >> 3) * S + 8 * ((r >> 2) & 1) + (r & 3)) * Cout + nt * 32;
          acc[nt][r] = acc[nt][r] * wunscale + bv;
          if (!ST_ABL(1)) ub[lane_off] = acc[nt][r];
        }
      }

      // ---- GroupNorm partials of the written tile: (sum, sum of squares) per cout over its 128 pixels: in-lane over the 16 registers,
      //      one exchange between the K halves, the four waves through LDS ----
      if (k.stats && !ST_ABL(2)) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          float vs = 0.f, vq = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            vs += acc[nt][r];
            vq = fmaf(acc[nt][r], acc[nt][r], vq);
          }
          vs += __shfl_xor(vs, 32);
          vq += __shfl_xor(vq, 32);
          if (kh == 0) {
            red[(wave * NT * 32 + nt * 32 + p32) * 2 + 0] = vs;
            red[(wave * NT * 32 + nt * 32 + p32) * 2 + 1] = vq;
          }
        }
      }
      ff_barrier();                      // the partials and the next patch are in LDS
      if (k.stats && !ST_ABL(2) && tid < NT * 32) {
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
          s += (double)red[(wv * NT * 32 + tid) * 2 + 0];
          q += (double)red[(wv * NT * 32 + tid) * 2 + 1];
        }
        double* dst = k.stats + ((size_t)tile * Cout + ng * NT * 32 + tid) * 2;
        dst[0] = s;
        dst[1] = q;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The wide first layer: 9 .. 32 assembled channels (the 16 + 16 slab networks, the 12 Haar bands, 9 + 3), padded with exact zeros to
// CP = 16 * KS channels.  Same tile (16 x 8 pixels, one 32-pixel M tile per wave), same products, same epilogue and statistics as
// stem_kernel; what differs is where the operands live:
//   * K = tap * CP + channel: K step s = tap * KS + ks holds channels 16 ks .. 16 ks + 15 of one tap, lanes of K half kh the upper / lower 8.
//     All 9 KS steps are full - there is no padding tap.
//   * the weight fragments of ALL cout groups no longer fit LDS (9 taps x 2 K steps x 4 cout tiles x 2 planes = 144 KB at nf 128), so a
//     workgroup serves ONE cout group (blockIdx.y; 32 NT couts: <= 108 KB for NT = 3, CP = 32, two planes) for all its tiles: the fragments
//     are copied to LDS once per workgroup, the patch is assembled once per (tile, cout group).  The input side is re-read per cout group
//     (1 .. 4 groups), which is small beside the layer's output (nf * 4 bytes per pixel against <= 32 * 4).
//   * the patch is kept as CP / 8 chunk planes [chunk][pixel] of 8 halves: consecutive pixels are consecutive 16-byte slots for the
//     A-operand reads and for the writes.
// The tile walk is a plain grid-stride loop; a tile's patch is assembled by all 256 threads (item = (chunk, patch pixel), coalesced
// along W), out-of-image pixels and the padding channels are written as exact zeros (masked, never clamped: no load is issued for them).
// S % 16 == 0, so every tile is whole.
template <int NT, int NS, int KS, bool YN, bool SQ>
__global__ __launch_bounds__(256, 2) void stem_wide_kernel(const StemArgs k) {
  constexpr int CH = 2 * KS;                        // 8-channel chunks of a pixel
  constexpr int NSTEP = 9 * KS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  half8* const phi = reinterpret_cast<half8*>(smem);                     // [CH][ST_PLANE]
  half8* const plo = phi + CH * ST_PLANE;                                // (NS == 2)
  float* const red = reinterpret_cast<float*>(smem + NS * CH * ST_PLANE * 16);      // [4 waves][NT * 32 couts][2]
  float* const bl = red + 4 * NT * 32 * 2;                                // bias of this cout group [NT * 32]
  half8* const wl = reinterpret_cast<half8*>(bl + NT * 32);              // this cout group's weight fragments

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kh = lane >> 5, p32 = lane & 31;
  const int S = k.S, Cx = k.Cx, Cy = k.Cy, Cout = k.Cout;
  const int ng = blockIdx.y;
  const size_t HW = (size_t)S * S;

  wg_copy_to_lds<256, 8>(reinterpret_cast<char*>(wl), reinterpret_cast<const char*>(k.w) + (size_t)ng * NSTEP * NT * NS * 1024,
                         NSTEP * NT * NS * 1024, tid);
  if (tid < NT * 32) bl[tid] = k.bias[ng * NT * 32 + tid];

  const int pix0 = (wave * 2 + (p32 >> 4)) * ST_PW + (p32 & 15);
  const float wunscale = 1.0f / C16_WSCALE;
  const half8* const wq = wl + lane;

  for (int tile = blockIdx.x; tile < k.nblocks; tile += gridDim.x) {
    const int b = tile / k.tpi, tin = tile - b * k.tpi;
    const int ty0 = (tin / k.tiles_x) * ST_TH, tx0 = (tin - (tin / k.tiles_x) * k.tiles_x) * 16;

    // ---- assemble the 18 x 10 patch: cat(x, y [+ sigma z]), 2v - 1, fp16 hi | lo split, zeros outside the image and beyond Cx + Cy ----
    for (int it = tid; it < CH * ST_NPIX; it += 256) {
      const int q = it / ST_NPIX, pp = it - q * ST_NPIX;
      const int py = pp / ST_PW, px = pp - py * ST_PW;
      const int gy = ty0 + py - 1, gx = tx0 + px - 1;
      const bool inimg = (unsigned)gy < (unsigned)S && (unsigned)gx < (unsigned)S;
      const size_t pix = inimg ? (size_t)gy * S + gx : 0;
      half8 h, l;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = q * 8 + e;
        float v = 0.f;
        if (SQ && inimg && c < Cx) {      // (Cx % 4 == 0: channel c and its dx partner c ^ 1 are both x; one 8-byte load serves the pair)
          const float2 v2 = *reinterpret_cast<const float2*>(k.x + (size_t)b * Cx * HW + sq_image_off(c & ~1, (int)pix, gy, S, (int)HW));
          v = (e & 1) ? v2.y : v2.x;
          v = k.centered ? v : 2.f * v - 1.f;
        } else if (inimg && c < Cx) {
          v = k.x[((size_t)b * Cx + c) * HW + pix];
          v = k.centered ? v : 2.f * v - 1.f;
        } else if (inimg && c < Cx + Cy) {
          const size_t j = ((size_t)b * Cy + (c - Cx)) * HW + pix;
          v = k.y[j];
          if (YN) v = v + k.yn[j] * k.ysig;
          v = k.centered ? v : 2.f * v - 1.f;
        }
        h[e] = (_Float16)v;
        l[e] = (_Float16)(v - (float)h[e]);
      }
      phi[q * ST_PLANE + pp] = h;
      if (NS == 2) plo[q * ST_PLANE + pp] = l;
    }
    ff_barrier();                        // the patch (first tile: and the weights, the bias) is in LDS; the previous tile's partials are read

    // ---- K loop: 9 taps x KS steps of 16 channels ----
    floatx16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
      const int tap = s / KS, ks = s - tap * KS;
      const int idx = (ks * 2 + kh) * ST_PLANE + pix0 + (tap / 3) * ST_PW + tap % 3;
      const half8 bh = phi[idx];
      half8 bl16;
      if (NS == 2) bl16 = plo[idx];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const half8 wh = wq[((s * NT + nt) * NS) * 64];
        if (NS == 2) {      // small products first
          const half8 wlo = wq[((s * NT + nt) * NS + 1) * 64];
          acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, wlo, acc[nt], 0, 0, 0);
          acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl16, wh, acc[nt], 0, 0, 0);
        }
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, wh, acc[nt], 0, 0, 0);
      }
    }

    // ---- epilogue: un-scale, bias, NHWC stores (stem_kernel's: a lane holds ONE cout of 16 pixels, whole 128-byte lines per store) ----
    float* const obase = k.out + (((size_t)b * S + ty0 + wave * 2) * S + tx0) * Cout + ng * NT * 32;      // uniform
    const unsigned lane_off = (unsigned)(4 * kh * Cout + p32);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const float bv = bl[nt * 32 + p32];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* const ub = obase + ((size_t)(r >> 3) * S + 8 * ((r >> 2) & 1) + (r & 3)) * Cout + nt * 32;
        acc[nt][r] = acc[nt][r] * wunscale + bv;
        ub[lane_off] = acc[nt][r];
      }
    }

    // ---- GroupNorm partials of the written tile, as stem_kernel leaves them: (sum, sum of squares) per (tile, cout) ----
    if (k.stats) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        float vs = 0.f, vq = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          vs += acc[nt][r];
          vq = fmaf(acc[nt][r], acc[nt][r], vq);
        }
        vs += __shfl_xor(vs, 32);
        vq += __shfl_xor(vq, 32);
        if (kh == 0) {
          red[(wave * NT * 32 + nt * 32 + p32) * 2 + 0] = vs;
          red[(wave * NT * 32 + nt * 32 + p32) * 2 + 1] = vq;
        }
      }
    }
    ff_barrier();                        // the partials are in LDS; every wave has read this tile's patch
    if (k.stats && tid < NT * 32) {
      double s = 0.0, q = 0.0;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) {
        s += (double)red[(wv * NT * 32 + tid) * 2 + 0];
        q += (double)red[(wv * NT * 32 + tid) * 2 + 1];
      }
      double* dst = k.stats + ((size_t)tile * Cout + ng * NT * 32 + tid) * 2;
      dst[0] = s;
      dst[1] = q;
    }
  }
}

// ---------------------------------------------------------------------------------------------
static inline int stem_nt(int cout) { return cout % 96 == 0 ? 3 : 2; }

// padded channel count of the assembled input inside the kernels: 8 (stem_kernel) up to 8 real channels, the next multiple of 16 above
static inline int stem_cpad(int cin) { return cin <= 8 ? 8 : wide_cpad(cin); }
static inline size_t stem_wide_lds(int cpad, int nt, int planes) {
  return (size_t)planes * (cpad / 8) * ST_PLANE * 16 + 4 * (size_t)nt * 32 * 2 * 4 + (size_t)nt * 32 * 4 + (size_t)9 * (cpad / 16) * nt * planes * 1024;
}

bool stem_supported(int Cx, int Cy, int Cout, int S, int ns) {
  if (CSD_TUNE_ENV("CSD_NO_STEM")) return false;
  if (!(ns >= 1 && ns <= 3 && Cx > 0 && Cy >= 0 && S % 16 == 0 && S >= 16 && (Cout % 96 == 0 || Cout % 64 == 0))) return false;
  if (Cx + Cy <= 8) return true;
  return Cx + Cy <= 32 && stem_wide_lds(stem_cpad(Cx + Cy), stem_nt(Cout), ns >= 2 ? 2 : 1) <= 160 * 1024;
}

// what a network's plan runs as the fused layer: every shape stem_kernel covers, and stem_wide_kernel where it measured faster than the
// assemble pass + generic convolution: at 16 padded channels.  At 32 its one-cout-group weight fragments (72 - 108 KB)
// leave one workgroup per CU and it measured slower, so the plan keeps the fallback there; csd_input_conv still reaches the kernel
bool stem_planned(int Cx, int Cy, int Cout, int S, int ns) {
  return stem_supported(Cx, Cy, Cout, S, ns) && stem_cpad(Cx + Cy) <= 16;
}

size_t stem_packed_bytes(int Cin, int Cout, int ns) {
  const int nt = stem_nt(Cout), planes = ns >= 2 ? 2 : 1;
  const int ksteps = Cin <= 8 ? ST_KSTEPS : 9 * (stem_cpad(Cin) / 16);
  return (size_t)(Cout / (32 * nt)) * ksteps * nt * planes * 1024;
}

// weights in A-fragment order: [cout group][K step][cout tile][plane][lane = (k half << 5) | cout row][8 halves]; k = tap * 8 + channel,
// scaled by 2^8 (exact) so the lo plane stays out of the fp16 subnormals
__global__ void stem_pack_kernel(const float* __restrict__ w, _Float16* __restrict__ wpack, int Cin, int Cout, int planes, int nt,
                                 size_t n_halves) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_halves) return;
  const int e = (int)(idx & 7);
  const int ln = (int)((idx >> 3) & 63);
  size_t rest = idx >> 9;
  const int pl = (int)(rest % planes); rest /= planes;
  const int t = (int)(rest % nt); rest /= nt;
  const int s = (int)(rest % ST_KSTEPS);
  const int ng = (int)(rest / ST_KSTEPS);
  const int tap = 2 * s + (ln >> 5);
  const int cout = (ng * nt + t) * 32 + (ln & 31);
  float v = 0.f;
  if (tap < 9 && e < Cin && cout < Cout) v = w[((size_t)cout * Cin + e) * 9 + tap] * C16_WSCALE;
  const _Float16 hi = (_Float16)v;
  wpack[idx] = pl == 0 ? hi : (_Float16)(v - (float)hi);
}

// the wide layer's: [cout group][K step = tap * KS + ks][cout tile][plane][lane = (k half << 5) | cout row][8 halves], channel
// 16 ks + 8 (k half) + e; channels >= Cin (the padding) are exact zeros
__global__ void stem_wide_pack_kernel(const float* __restrict__ w, _Float16* __restrict__ wpack, int Cin, int Cout, int planes, int nt,
                                      int ks_per_tap, size_t n_halves) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_halves) return;
  const int e = (int)(idx & 7);
  const int ln = (int)((idx >> 3) & 63);
  size_t rest = idx >> 9;
  const int pl = (int)(rest % planes); rest /= planes;
  const int t = (int)(rest % nt); rest /= nt;
  const int s = (int)(rest % (9 * ks_per_tap));
  const int ng = (int)(rest / (9 * ks_per_tap));
  const int tap = s / ks_per_tap, ks = s - tap * ks_per_tap;
  const int cin = ks * 16 + (ln >> 5) * 8 + e;
  const int cout = (ng * nt + t) * 32 + (ln & 31);
  float v = 0.f;
  if (cin < Cin && cout < Cout) v = w[((size_t)cout * Cin + cin) * 9 + tap] * C16_WSCALE;
  const _Float16 hi = (_Float16)v;
  wpack[idx] = pl == 0 ? hi : (_Float16)(v - (float)hi);
}

int stem_pack_weight(const float* w, int Cin, int Cout, int ns, void* wpack, hipStream_t s) {
  const size_t n = stem_packed_bytes(Cin, Cout, ns) / 2;
  if (Cin > 8) {
    hipLaunchKernelGGL(stem_wide_pack_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, w, (_Float16*)wpack, Cin, Cout,
                       ns >= 2 ? 2 : 1, stem_nt(Cout), stem_cpad(Cin) / 16, n);
    CSD_LAUNCH_CHECK();
    return CSD_OK;
  }
  hipLaunchKernelGGL(stem_pack_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, w, (_Float16*)wpack, Cin, Cout,
                     ns >= 2 ? 2 : 1, stem_nt(Cout), n);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

int stem_tiles_per_image(int S) { return (S / 16) * (S / ST_TH); }

int stem_launch(const float* x, const float* y, const float* y_noise, float y_sigma, const void* wpack, const float* bias, float* out,
                double* stats, int B, int Cx, int Cy, int Cout, int S, int centered, int ns, hipStream_t s, int x_squeeze, int y_scale,
                float* y_tmp) {
  CSD_REQUIRE(stem_supported(Cx, Cy, Cout, S, ns), "stem: unsupported shape (%d+%d -> %d channels, %dx%d)", Cx, Cy, Cout, S, S);
  CSD_REQUIRE(!y_scale || (y_scale >= 2 && !x_squeeze && Cx <= 4 && Cy >= 1 && Cy <= 4 && S % y_scale == 0 && y),
              "stem: y_scale = %d needs up to 4 x and 1 .. 4 y channels (got %d + %d), no x_squeeze and image_size %% y_scale == 0",
              y_scale, Cx, Cy);
  CSD_REQUIRE(!x_squeeze || (Cx % 4 == 0 && (Cx + Cy > 8 || Cx == 4) && (reinterpret_cast<uintptr_t>(x) & 7) == 0),
              "stem: x_squeeze needs x_channels %% 4 == 0 (x_channels = 4 up to 8 assembled channels; got %d) and an 8-byte aligned x", Cx);
  const bool sq = x_squeeze != 0;
  StemArgs k;
  k.x = x; k.y = y; k.yn = y_noise; k.ysig = y_sigma;
  k.w = reinterpret_cast<const _Float16*>(wpack); k.bias = bias; k.out = out; k.stats = stats;
  k.ys = y_scale;
  if (y_scale && y_noise) {      // perturb at low resolution, then the kernel upsamples (no YN variant of YS: see the header)
    CSD_REQUIRE(y_tmp, "stem: y_scale with y_noise needs the scratch plane");
    const int lo = S / y_scale;
    const int rcp = bilinear_perturb_launch(y, y_noise, y_sigma, y_tmp, (size_t)B * Cy * lo * lo, s);
    if (rcp) return rcp;
    k.y = y_tmp; k.yn = nullptr;
  }
  k.B = B; k.S = S; k.Cx = Cx; k.Cy = y ? Cy : 0; k.Cout = Cout;
  k.tiles_x = S / 16; k.tpi = stem_tiles_per_image(S);
  const int nt = stem_nt(Cout);
  k.n_groups = Cout / (32 * nt);
  k.nblocks = B * k.tpi;               // tiles (every workgroup runs all cout groups of its tiles)
  k.centered = centered;
  k.abl = CSD_TUNE_ENV("CSD_STEM_ABL") ? atoi(CSD_TUNE_ENV("CSD_STEM_ABL")) : 0;
  const int planes = ns >= 2 ? 2 : 1;
  if (k.Cx + k.Cy > 8 || Cx + Cy > 8) {      // the wide layer: one cout group per workgroup row, a grid-stride walk over the tiles
    const int cpad = stem_cpad(Cx + Cy);      // (the weights were packed for Cx + Cy channels, with or without y)
    const size_t lds = stem_wide_lds(cpad, nt, planes);
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 2) per_cu = 2;               // (__launch_bounds__(256, 2))
    if (per_cu < 1) per_cu = 1;
    const int want = std::max(1, device_cu_count8() * per_cu / k.n_groups);
    const dim3 grid((unsigned)std::min(k.nblocks, want), (unsigned)k.n_groups);
    const bool ynw = y_noise != nullptr && k.Cy > 0;
    auto gow = [&](auto kern) -> int {
      CSD_SET_MAX_LDS_ONCE(kern);
      hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, k);
      return CSD_OK;
    };
    int rcw;
#define CSD_STEM_WIDE(NT_, NS_, KS_)                                                                                        \
  (sq ? (ynw ? gow(stem_wide_kernel<NT_, NS_, KS_, true, true>) : gow(stem_wide_kernel<NT_, NS_, KS_, false, true>))       \
      : (ynw ? gow(stem_wide_kernel<NT_, NS_, KS_, true, false>) : gow(stem_wide_kernel<NT_, NS_, KS_, false, false>)))
    if (cpad == 16) rcw = nt == 3 ? (planes == 2 ? CSD_STEM_WIDE(3, 2, 1) : CSD_STEM_WIDE(3, 1, 1)) : (planes == 2 ? CSD_STEM_WIDE(2, 2, 1) : CSD_STEM_WIDE(2, 1, 1));
    else rcw = nt == 3 ? (planes == 2 ? CSD_STEM_WIDE(3, 2, 2) : CSD_STEM_WIDE(3, 1, 2)) : (planes == 2 ? CSD_STEM_WIDE(2, 2, 2) : CSD_STEM_WIDE(2, 1, 2));
#undef CSD_STEM_WIDE
    if (rcw) return rcw;
    CSD_LAUNCH_CHECK();
    return CSD_OK;
  }
  const size_t lds = 2 * ST_PLANE * 16 + 4 * (size_t)nt * 32 * 2 * 4 + (size_t)k.n_groups * ST_KSTEPS * nt * planes * 1024 + (size_t)Cout * 4;
  CSD_REQUIRE(lds <= 160 * 1024, "stem: %d couts need %zu bytes of LDS", Cout, lds);
  const int n_cu = device_cu_count8();
  int per_cu = (int)((160 * 1024) / lds);      // persistent: as many workgroups per CU as LDS (and 128 VGPRs) allow, a multiple of the 8 XCDs
  if (per_cu > 4) per_cu = 4;
  if (per_cu < 1) per_cu = 1;
  const int want = n_cu * per_cu;
  const int grid = k.nblocks < want ? (k.nblocks + 7) / 8 * 8 : want;
  auto go = [&](auto kern) -> int {
    CSD_SET_MAX_LDS_ONCE(kern);           // (one flag array per kernel instantiation: the lambda's operator() is a template)
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, k);
    return CSD_OK;
  };
  int rc;
  const bool yn = y_noise != nullptr && k.Cy > 0 && !y_scale;
  // (SQ exists for the split-operand modes only: with one plane its y-noise variants do not fit 128 VGPRs without spilling, and the plan
  // of the plain fp16 mode keeps the assemble pass there - unet_layout.h)
  CSD_REQUIRE(!sq || planes == 2, "stem: x_squeeze on up to 8 channels is provided for the split-operand modes (fp16x3 / fp16f8) only");
  const bool ysv = y_scale != 0;
#define CSD_STEM_YN(NT_, NS_, SQ_) (yn ? go(stem_kernel<NT_, NS_, true, SQ_, false>) : go(stem_kernel<NT_, NS_, false, SQ_, false>))
  if (nt == 3 && planes == 2) rc = sq ? CSD_STEM_YN(3, 2, true) : (ysv ? go(stem_kernel<3, 2, false, false, true>) : CSD_STEM_YN(3, 2, false));
  else if (nt == 3) rc = ysv ? go(stem_kernel<3, 1, false, false, true>) : CSD_STEM_YN(3, 1, false);
  else if (planes == 2) rc = sq ? CSD_STEM_YN(2, 2, true) : (ysv ? go(stem_kernel<2, 2, false, false, true>) : CSD_STEM_YN(2, 2, false));
  else rc = ysv ? go(stem_kernel<2, 1, false, false, true>) : CSD_STEM_YN(2, 1, false);
#undef CSD_STEM_YN
  if (rc) return rc;
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

}  // namespace csd
