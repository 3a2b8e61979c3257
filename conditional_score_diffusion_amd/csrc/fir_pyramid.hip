// fir_pyramid.hip - the input pyramid of NCSN++ with progressive_input = 'residual' (models/ncsnpp.py:171-176, 300-307):
// layerspp.Downsample(with_conv=True) (layerspp.py:129-163) of the previous level's combined h (level 0: the network input),
// combined with the down block's output as (pyramid + h) / sqrt(2) (skip_rescale) or pyramid + h.
//
//   fir = True:  Conv2d_0 = conv_downsample_2d (up_or_down_sampling.py:144-178): upfirdn2d with the normalised 4-tap FIR, pads (2, 2)
//                (output side S + 1; upfirdn2d correlates with the FLIPPED kernel), then a VALID stride-2 3x3 conv, then the bias.
//   fir = False: Conv_0 on F.pad(x, (0, 1, 0, 1)), stride 2.
//
// Both are ONE 6x6 stride-2 convolution with pad 2 on the source:
//   out[b, i, j, o] = bias[o] + sum_{c, u, v} G[o, c, u, v] * x[b, 2i + u - 2, 2j + v - 2, c]
//   G[u][v] = sum_{a, b} W[a][b] * k2[a + 3 - u][b + 3 - v],   k2 = outer(k, k) / (sum k)^2
// (fir = False is the tap vector (0, 1, 0, 0): G[u][v] = W[u - 2][v - 2], only u, v in 2..4 are non-zero and the kernels skip the rest).
// G is folded once per weight in fp64 (fir_pyr_fold); the forward reads the fp32 source directly - no FIR intermediate in memory - and
// adds the bias, the residual h and the skip scale in its epilogue.  The arithmetic is fp32 FMA in every precision mode: the operand
// is the raw residual stream (kernel table).  Fixed summation orders throughout: a call is bitwise repeatable.
//
// Backward: the data gradient is the transposed 6x6 stride-2 convolution (per source pixel at most 3 x 3 dy taps), the weight gradient
// is dG (fixed-order partials per batch slice) folded back through the same FIR: dW[a][b] = sum_{u,v} dG[u][v] k2[a + 3 - u][b + 3 - v].
#include "common.h"

namespace csd {

static constexpr int PYR_T = 4;                  // output tile side of one workgroup
static constexpr int PYR_R = 2 * PYR_T + 4;      // source rows / columns a tile reads (12)
static constexpr int PYR_CK = 16;                // source channels staged per LDS burst

struct PyrTaps { float t[4]; };

__device__ __forceinline__ double pyr_k2(const PyrTaps& k, int a, int b, double inv_s2) {
  return (double)k.t[a] * (double)k.t[b] * inv_s2;
}

// G in the forward layout gf[c][u][v][o] and (optional) the data-gradient layout gt[u][v][o][c]
__global__ void fir_pyr_fold_kernel(const float* __restrict__ w, int Cin, int Cout, PyrTaps k, double inv_s2, float* __restrict__ gf,
                                    float* __restrict__ gt) {
  const int64_t n = (int64_t)Cout * Cin * 36;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int uv = (int)(e % 36);
    const int64_t oc = e / 36;
    const int c = (int)(oc % Cin), o = (int)(oc / Cin);
    const int u = uv / 6, v = uv % 6;
    const float* wp = w + ((int64_t)o * Cin + c) * 9;
    double acc = 0.0;
    for (int a = 0; a < 3; ++a) {
      const int ta = a + 3 - u;
      if (ta < 0 || ta > 3) continue;
      for (int b = 0; b < 3; ++b) {
        const int tb = b + 3 - v;
        if (tb < 0 || tb > 3) continue;
        acc += (double)wp[a * 3 + b] * pyr_k2(k, ta, tb, inv_s2);
      }
    }
    const float g = (float)acc;
    if (gf) gf[((int64_t)c * 36 + uv) * Cout + o] = g;
    if (gt) gt[((int64_t)uv * Cout + o) * Cin + c] = g;
  }
}

// forward: one wave per (64 output channels, 4x4 output pixels, sample); the 12 x 12 source window of PYR_CK channels is staged in LDS
template <int ULO, int UHI>
__global__ __launch_bounds__(64) void fir_pyr_conv_kernel(const float* __restrict__ x, int64_t sb, int sp, int64_t sc, int H, int Cin,
                                                          const float* __restrict__ g, const float* __restrict__ bias,
                                                          const float* __restrict__ res, float* __restrict__ out, int Cout, int Ho,
                                                          int tiles_x, float scale) {
  __shared__ __align__(16) float xs[PYR_CK * PYR_R * PYR_R];
  const int lane = threadIdx.x;
  const int o = blockIdx.x * 64 + lane;
  const bool live = o < Cout;
  const int oc = live ? o : Cout - 1;
  const int ty = blockIdx.y / tiles_x, tx = blockIdx.y - (blockIdx.y / tiles_x) * tiles_x;
  const int b = blockIdx.z;
  const int i0 = ty * PYR_T, j0 = tx * PYR_T;
  const int Y0 = 2 * i0 - 2, X0 = 2 * j0 - 2;
  const float* xb = x + (int64_t)b * sb;
  float acc[PYR_T][PYR_T];
#pragma unroll
  for (int i = 0; i < PYR_T; ++i)
#pragma unroll
    for (int j = 0; j < PYR_T; ++j) acc[i][j] = 0.f;
  for (int c0 = 0; c0 < Cin; c0 += PYR_CK) {
    const int ck = min(PYR_CK, Cin - c0);
    __syncthreads();
    for (int e = lane; e < ck * PYR_R * PYR_R; e += 64) {
      const int c = e % ck, p = e / ck;
      const int r = p / PYR_R, q = p - (p / PYR_R) * PYR_R;
      const int Y = Y0 + r, X = X0 + q;
      float v = 0.f;
      if (Y >= 0 && Y < H && X >= 0 && X < H) v = xb[(int64_t)(Y * H + X) * sp + (int64_t)(c0 + c) * sc];
      xs[(c * PYR_R + r) * PYR_R + q] = v;
    }
    __syncthreads();
    for (int c = 0; c < ck; ++c) {
      const float* gc = g + (int64_t)(c0 + c) * 36 * Cout + oc;
#pragma unroll
      for (int u = ULO; u <= UHI; ++u) {
        float wv[6];
#pragma unroll
        for (int v = ULO; v <= UHI; ++v) wv[v] = gc[(u * 6 + v) * Cout];
#pragma unroll
        for (int i = 0; i < PYR_T; ++i) {
          const float4* row = reinterpret_cast<const float4*>(xs + (c * PYR_R + 2 * i + u) * PYR_R);
          float xr[PYR_R];
#pragma unroll
          for (int q4 = 0; q4 < PYR_R / 4; ++q4) {
            const float4 t = row[q4];
            xr[4 * q4] = t.x; xr[4 * q4 + 1] = t.y; xr[4 * q4 + 2] = t.z; xr[4 * q4 + 3] = t.w;
          }
#pragma unroll
          for (int v = ULO; v <= UHI; ++v)
#pragma unroll
            for (int j = 0; j < PYR_T; ++j) acc[i][j] = fmaf(wv[v], xr[2 * j + v], acc[i][j]);
        }
      }
    }
  }
  if (!live) return;
  const float bo = bias ? bias[o] : 0.f;
#pragma unroll
  for (int i = 0; i < PYR_T; ++i)
#pragma unroll
    for (int j = 0; j < PYR_T; ++j) {
      const int oi = i0 + i, oj = j0 + j;
      if (oi >= Ho || oj >= Ho) continue;
      const int64_t idx = (((int64_t)b * Ho + oi) * Ho + oj) * Cout + o;
      float r = acc[i][j] + bo;
      if (res) r += res[idx];
      out[idx] = r * scale;
    }
}

// data gradient: dx[b, Y, X, c] = scale * sum_{i, j, o} G[o, c, Y + 2 - 2i, X + 2 - 2j] dy[b, i, j, o]  for c < nc.  By phase
// (Y = 2p + ry, u = ry + 2m) this is dx[2p + ry, 2q + rx] = sum_{m, n, o} G[o, c, ry + 2m, rx + 2n] dy[p + 1 - m, q + 1 - n, o]: one wave
// per (64 source channels, 4x4 dy positions = 8x8 dx pixels, sample); the 6x6 dy window of PYR_CK output channels is staged in LDS and
// every weight load (coalesced over c, layout gt[u][v][o][c]) feeds 16 FMAs.  dx element (b, Y, X, c) at b * db + (Y * H + X) * dp + c * dc
template <int ULO, int UHI>
__global__ __launch_bounds__(64) void fir_pyr_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ gt, float* __restrict__ dx,
                                                           int64_t db, int dp, int64_t dc, int H, int Cin, int nc, int Cout, int Ho, int tiles_x,
                                                           float scale) {
  __shared__ __align__(16) float ds[PYR_CK * 6 * 8];
  const int lane = threadIdx.x;
  const int c = blockIdx.x * 64 + lane;
  const bool live = c < nc;
  const int cc = live ? c : nc - 1;
  const int ty = blockIdx.y / tiles_x, tx = blockIdx.y - (blockIdx.y / tiles_x) * tiles_x;
  const int b = blockIdx.z;
  const int p0 = ty * PYR_T, q0 = tx * PYR_T;
  float acc[2][2][PYR_T][PYR_T];
#pragma unroll
  for (int ry = 0; ry < 2; ++ry)
#pragma unroll
    for (int rx = 0; rx < 2; ++rx)
#pragma unroll
      for (int i = 0; i < PYR_T; ++i)
#pragma unroll
        for (int j = 0; j < PYR_T; ++j) acc[ry][rx][i][j] = 0.f;
  for (int o0 = 0; o0 < Cout; o0 += PYR_CK) {
    const int ok = min(PYR_CK, Cout - o0);
    __syncthreads();
    for (int e = lane; e < ok * 36; e += 64) {
      const int o = e % ok, pix = e / ok;
      const int r = pix / 6, q = pix - (pix / 6) * 6;
      const int P = p0 - 1 + r, Q = q0 - 1 + q;
      float v = 0.f;
      if (P >= 0 && P < Ho && Q >= 0 && Q < Ho) v = dy[(((int64_t)b * Ho + P) * Ho + Q) * Cout + o0 + o];
      ds[(o * 6 + r) * 8 + q] = v;
    }
    __syncthreads();
    for (int o = 0; o < ok; ++o) {
      float d[6][6];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const float4* row = reinterpret_cast<const float4*>(ds + (o * 6 + r) * 8);
        const float4 a = row[0], t = row[1];
        d[r][0] = a.x; d[r][1] = a.y; d[r][2] = a.z; d[r][3] = a.w; d[r][4] = t.x; d[r][5] = t.y;
      }
      const float* gp = gt + (int64_t)(o0 + o) * Cin + cc;
#pragma unroll
      for (int u = ULO; u <= UHI; ++u)
#pragma unroll
        for (int v = ULO; v <= UHI; ++v) {
          const float w = gp[(int64_t)(u * 6 + v) * Cout * Cin];
#pragma unroll
          for (int i = 0; i < PYR_T; ++i)
#pragma unroll
            for (int j = 0; j < PYR_T; ++j)
              acc[u & 1][v & 1][i][j] = fmaf(w, d[i + 2 - (u >> 1)][j + 2 - (v >> 1)], acc[u & 1][v & 1][i][j]);
        }
    }
  }
  if (!live) return;
#pragma unroll
  for (int ry = 0; ry < 2; ++ry)
#pragma unroll
    for (int rx = 0; rx < 2; ++rx)
#pragma unroll
      for (int i = 0; i < PYR_T; ++i)
#pragma unroll
        for (int j = 0; j < PYR_T; ++j) {
          const int Y = 2 * (p0 + i) + ry, X = 2 * (q0 + j) + rx;
          if (Y >= H || X >= H) continue;
          dx[(int64_t)b * db + (int64_t)(Y * H + X) * dp + (int64_t)c * dc] = acc[ry][rx][i][j] * scale;
        }
}

// weight gradient, stage 1: part[sl][c][u][v][o] = sum over the samples of slice sl and every output pixel of dy[b, i, j, o] x[b, 2i+u-2, 2j+v-2, c]
template <int ULO, int UHI>
__global__ void fir_pyr_wgrad_kernel(const float* __restrict__ x, int64_t sb, int sp, int64_t sc, int H, int Cin, const float* __restrict__ dy,
                                     int Cout, int Ho, int B, int nsl, float* __restrict__ part) {
  const int64_t n = (int64_t)nsl * Cin * Cout;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int o = (int)(e % Cout);
    const int c = (int)((e / Cout) % Cin);
    const int sl = (int)(e / ((int64_t)Cout * Cin));
    const int b0 = (int)((int64_t)sl * B / nsl), b1 = (int)((int64_t)(sl + 1) * B / nsl);
    float acc[6][6];
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int v = 0; v < 6; ++v) acc[u][v] = 0.f;
    for (int b = b0; b < b1; ++b) {
      const float* xb = x + (int64_t)b * sb + (int64_t)c * sc;
      for (int i = 0; i < Ho; ++i)
        for (int j = 0; j < Ho; ++j) {
          const float d = dy[(((int64_t)b * Ho + i) * Ho + j) * Cout + o];
#pragma unroll
          for (int u = ULO; u <= UHI; ++u) {
            const int Y = 2 * i + u - 2;
            if (Y < 0 || Y >= H) continue;
#pragma unroll
            for (int v = ULO; v <= UHI; ++v) {
              const int X = 2 * j + v - 2;
              if (X < 0 || X >= H) continue;
              acc[u][v] = fmaf(d, xb[(int64_t)(Y * H + X) * sp], acc[u][v]);
            }
          }
        }
    }
    float* pp = part + ((int64_t)sl * Cin + c) * 36 * Cout + o;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int v = 0; v < 6; ++v) pp[(int64_t)(u * 6 + v) * Cout] = acc[u][v];
  }
}

// weight gradient, stage 2: dW[o, c, a, b] (=|+=) sum_{u, v} (sum_sl part) * k2[a + 3 - u][b + 3 - v]  (fixed order, fp64)
__global__ void fir_pyr_unfold_kernel(const float* __restrict__ part, int nsl, int Cin, int Cout, PyrTaps k, double inv_s2,
                                      float* __restrict__ dw, int beta) {
  const int64_t n = (int64_t)Cout * Cin * 9;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int ab = (int)(e % 9);
    const int64_t oc = e / 9;
    const int c = (int)(oc % Cin), o = (int)(oc / Cin);
    const int a = ab / 3, bb = ab % 3;
    double acc = 0.0;
    for (int u = 0; u < 6; ++u) {
      const int ta = a + 3 - u;
      if (ta < 0 || ta > 3) continue;
      for (int v = 0; v < 6; ++v) {
        const int tb = bb + 3 - v;
        if (tb < 0 || tb > 3) continue;
        const double kk = pyr_k2(k, ta, tb, inv_s2);
        if (kk == 0.0) continue;
        double s = 0.0;
        for (int sl = 0; sl < nsl; ++sl) s += (double)part[(((int64_t)sl * Cin + c) * 36 + u * 6 + v) * Cout + o];
        acc += s * kk;
      }
    }
    const float v = (float)acc;                  // beta = 1: dw += the rounded value (one fp32 addition)
    dw[e] = beta ? dw[e] + v : v;
  }
}

static PyrTaps pyr_taps(const float* taps4, double* inv_s2) {
  PyrTaps k;
  if (taps4) {
    for (int i = 0; i < 4; ++i) k.t[i] = taps4[i];
  } else {                                       // fir = False: F.pad(0, 1, 0, 1) + stride-2 conv
    k.t[0] = 0.f; k.t[1] = 1.f; k.t[2] = 0.f; k.t[3] = 0.f;
  }
  const double s = (double)k.t[0] + k.t[1] + k.t[2] + k.t[3];
  *inv_s2 = 1.0 / (s * s);
  return k;
}

static inline unsigned pyr_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 8192); }

int fir_pyr_fold_launch(const float* w, int Cin, int Cout, const float* taps4, float* gf, float* gt, hipStream_t s) {
  double inv_s2;
  const PyrTaps k = pyr_taps(taps4, &inv_s2);
  CSD_REQUIRE(std::isfinite(inv_s2), "fir_pyr: the FIR taps sum to zero");
  hipLaunchKernelGGL(fir_pyr_fold_kernel, dim3(pyr_grid((int64_t)Cout * Cin * 36)), dim3(256), 0, s, w, Cin, Cout, k, inv_s2, gf, gt);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

int fir_pyr_conv_launch(const float* x, int64_t sb, int sp, int64_t sc, int B, int H, int Cin, const float* gf, const float* bias,
                        const float* res, float* out, int Cout, bool fir, float scale, hipStream_t s) {
  CSD_REQUIRE(B >= 1 && H >= 2 && H % 2 == 0 && Cin >= 1 && Cout >= 1, "fir_pyr: bad shape B=%d H=%d Cin=%d Cout=%d", B, H, Cin, Cout);
  CSD_REQUIRE(B <= 65535, "fir_pyr: batch %d above the grid limit", B);
  const int Ho = H / 2, tiles = cdiv(Ho, PYR_T);
  const dim3 grid(cdiv(Cout, 64), tiles * tiles, B);
  if (fir)
    hipLaunchKernelGGL((fir_pyr_conv_kernel<0, 5>), grid, dim3(64), 0, s, x, sb, sp, sc, H, Cin, gf, bias, res, out, Cout, Ho, tiles, scale);
  else
    hipLaunchKernelGGL((fir_pyr_conv_kernel<2, 4>), grid, dim3(64), 0, s, x, sb, sp, sc, H, Cin, gf, bias, res, out, Cout, Ho, tiles, scale);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

int fir_pyr_dgrad_launch(const float* dy, const float* gt, float* dx, int64_t db, int dp, int64_t dc, int B, int H, int Cin, int nc, int Cout,
                         bool fir, float scale, hipStream_t s) {
  CSD_REQUIRE(nc >= 1 && nc <= Cin && H >= 2 && H % 2 == 0 && B >= 1 && B <= 65535, "fir_pyr dgrad: bad shape B=%d H=%d nc=%d", B, H, nc);
  const int Ho = H / 2, tiles = cdiv(Ho, PYR_T);
  const dim3 grid(cdiv(nc, 64), tiles * tiles, B);
  if (fir)
    hipLaunchKernelGGL((fir_pyr_dgrad_kernel<0, 5>), grid, dim3(64), 0, s, dy, gt, dx, db, dp, dc, H, Cin, nc, Cout, Ho, tiles, scale);
  else
    hipLaunchKernelGGL((fir_pyr_dgrad_kernel<2, 4>), grid, dim3(64), 0, s, dy, gt, dx, db, dp, dc, H, Cin, nc, Cout, Ho, tiles, scale);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

// batch slices of the weight gradient's first stage: enough (slice, c, o) threads to fill the device, at most B
int fir_pyr_wgrad_slices(int B, int Cin, int Cout) {
  const int64_t per = (int64_t)Cin * Cout;
  return (int)std::max<int64_t>(1, std::min<int64_t>(B, (262144 + per - 1) / per));
}
size_t fir_pyr_wgrad_scratch_floats(int B, int Cin, int Cout) { return (size_t)fir_pyr_wgrad_slices(B, Cin, Cout) * 36 * Cin * Cout; }

int fir_pyr_wgrad_launch(const float* x, int64_t sb, int sp, int64_t sc, int B, int H, int Cin, const float* dy, int Cout, const float* taps4,
                         bool fir, float* dw, float* scratch, hipStream_t s, int beta) {
  const int nsl = fir_pyr_wgrad_slices(B, Cin, Cout);
  const int64_t n = (int64_t)nsl * Cin * Cout;
  if (fir)
    hipLaunchKernelGGL((fir_pyr_wgrad_kernel<0, 5>), dim3(pyr_grid(n)), dim3(256), 0, s, x, sb, sp, sc, H, Cin, dy, Cout, H / 2, B, nsl, scratch);
  else
    hipLaunchKernelGGL((fir_pyr_wgrad_kernel<2, 4>), dim3(pyr_grid(n)), dim3(256), 0, s, x, sb, sp, sc, H, Cin, dy, Cout, H / 2, B, nsl, scratch);
  CSD_LAUNCH_CHECK();
  double inv_s2;
  const PyrTaps k = pyr_taps(fir ? taps4 : nullptr, &inv_s2);
  hipLaunchKernelGGL(fir_pyr_unfold_kernel, dim3(pyr_grid((int64_t)Cout * Cin * 9)), dim3(256), 0, s, scratch, nsl, Cin, Cout, k, inv_s2, dw, beta);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

}  // namespace csd

using namespace csd;

extern "C" size_t csd_fir_pyr_conv_scratch_bytes(int Cin, int Cout) {
  if (Cin < 1 || Cout < 1) return 0;
  return (size_t)36 * Cin * Cout * sizeof(float) + 256;
}

extern "C" int csd_fir_pyr_conv(const float* x, const float* w, const float* bias, const float* res, float* out, int B, int Cin, int Cout,
                                int H, int x_pixel_stride, const float* fir_kernel, float out_scale, void* scratch, void* stream) {
  CSD_REQUIRE(x && w && out && scratch, "fir_pyr_conv: null argument");
  CSD_REQUIRE(x_pixel_stride >= Cin, "fir_pyr_conv: pixel stride %d below Cin %d", x_pixel_stride, Cin);
  if (fir_kernel) {
    for (int i = 0; i < 4; ++i) CSD_REQUIRE(std::isfinite(fir_kernel[i]), "fir_pyr_conv: non-finite FIR tap");
  }
  const hipStream_t s = (hipStream_t)stream;
  float* gf = static_cast<float*>(scratch);
  int rc = fir_pyr_fold_launch(w, Cin, Cout, fir_kernel, gf, nullptr, s);
  if (rc) return rc;
  return fir_pyr_conv_launch(x, (int64_t)H * H * x_pixel_stride, x_pixel_stride, 1, B, H, Cin, gf, bias, res, out, Cout, fir_kernel != nullptr,
                             out_scale, s);
}
