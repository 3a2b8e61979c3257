// sampler.hip - the predictor / corrector "noise-add" steps of the reverse-SDE sampler and the
// on-device noise source.  HBM-bound elementwise work on the 3-channel state (NCHW fp32).
//
//   langevin   (sampling/correctors.py:58-78, 88-108; VE => alpha = 1):
//       score = net/std; gbar = mean_b ||score_b||_2 ; nbar = mean_b ||z_b||_2
//       step = (snr*nbar/gbar)^2 * 2 ; x_mean = x + step*score ; x = x_mean + sqrt(2*step)*z
//     The batch means couple the samples: a first kernel writes per-(sample,chunk)
//     fp64 partial sums, the update kernel folds them (deterministic order) in its prologue.
//   reverse diffusion (sampling/predictors.py:84-89,97-102 with sde_lib.py:135-140,410-418):
//       x_mean = x + G^2*score ; x = x_mean + G*z
//   reverse diffusion with a forward drift / as the probability flow (the same lines with sde_lib.py:65-102,186-195,49-63):
//       f = sqrt(alpha_i)*x - x (VP) | (phi*x)*dt (sub-VP) | 0 (VE) ; rev_f = f - G^2*score*kappa ; x_mean = x - rev_f ;
//       x = x_mean + G_noise*z, kappa = 1/2 and G_noise = 0 for the probability flow
// fp contraction is disabled so that mul/add round exactly like the reference's separate torch ops.
#include <algorithm>

#include "common.h"

#pragma clang fp contract(off)

namespace csd {

#define SQ_THREADS 256

int sumsq_nchunk(int64_t per) {
  int64_t n = per / (SQ_THREADS * 4 * 8);   // >= 8 float4 per thread
  if (n < 1) n = 1;
  if (n > 64) n = 64;
  return (int)n;
}

// partial[(b*nchunk + chunk)*2 + {0,1}] = sum a^2 , sum b^2 over the chunk (fp64)
__global__ __launch_bounds__(SQ_THREADS) void sumsq_rows_kernel(const float* __restrict__ a, int64_t a_stride,
                                                                const float* __restrict__ bb,
                                                                double* __restrict__ partial, int64_t per,
                                                                int nchunk) {
  __shared__ double red[2][SQ_THREADS / 64];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int64_t len = (per + nchunk - 1) / nchunk;
  const int64_t i0 = chunk * len, i1 = min(per, i0 + len);
  const float* pa = a + (size_t)b * a_stride;
  const float* pb = bb + (size_t)b * per;
  double sa = 0, sb = 0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += SQ_THREADS) {
    const float va = pa[i], vb = pb[i];
    sa += (double)va * va;
    sb += (double)vb * vb;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sa += __shfl_xor(sa, off);
    sb += __shfl_xor(sb, off);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = sa;
    red[1][threadIdx.x >> 6] = sb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ta = 0, tb = 0;
    for (int w = 0; w < SQ_THREADS / 64; ++w) { ta += red[0][w]; tb += red[1][w]; }
    partial[((size_t)b * nchunk + chunk) * 2 + 0] = ta;
    partial[((size_t)b * nchunk + chunk) * 2 + 1] = tb;
  }
}

// The loop of the five update kernels on the network's (row-strided) output: element i of sample b reads net[b*net_stride + i - b*per]
// (a paired network emits [score_x | score_y] per sample, so net_stride >= per) and divides by std; rule(x_i, score, z_i) yields
// (x_mean_i, the new x_i).  Each kernel writes its rule inline, in the reference's order of operations (fp contraction is off).
template <class Rule>
__device__ __forceinline__ void strided_update(float* __restrict__ x, float* __restrict__ x_mean, const float* __restrict__ net,
                                               int64_t net_stride, const float* __restrict__ z, float std, int64_t per, size_t total,
                                               Rule rule) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / (size_t)per;
    const float score = net[b * net_stride + (i - b * per)] / std;
    const float2 u = rule(x[i], score, z[i]);
    x_mean[i] = u.x;
    x[i] = u.y;
  }
}

__global__ __launch_bounds__(256) void langevin_update_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                              const float* __restrict__ net,
                                                              int64_t net_stride, const float* __restrict__ z,
                                                              const double* __restrict__ partial, int nchunk,
                                                              float std, float snr, float alpha, int B, int64_t per,
                                                              size_t total, int* __restrict__ nonfinite) {
  __shared__ float s_step;
  if (threadIdx.x < 64) {
    // fold partials: lanes stride over samples; each lane folds its samples' chunks in order
    double g = 0, n = 0;
    for (int b = threadIdx.x; b < B; b += 64) {
      double sa = 0, sb = 0;
      for (int c = 0; c < nchunk; ++c) {
        sa += partial[((size_t)b * nchunk + c) * 2 + 0];
        sb += partial[((size_t)b * nchunk + c) * 2 + 1];
      }
      g += sqrt(sa) / (double)std;   // ||net_b/std|| = ||net_b||/std
      n += sqrt(sb);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      g += __shfl_xor(g, off);
      n += __shfl_xor(n, off);
    }
    if (threadIdx.x == 0) {
      const float gbar = (float)(g / B), nbar = (float)(n / B);
      const float r = snr * nbar / gbar;
      s_step = r * r * 2.f * alpha;  // (snr*nbar/gbar)**2 * 2 * alpha; alpha = 1 for the VE SDEs, sde.alphas[timestep] for VP / subVP
      // the finiteness contract of the fused loop: the norms see every element of the score and of the noise, so a NaN / Inf
      // anywhere (an fp16-operand mode past its range) shows here at no cost; csd_pc_sample reports the flag at its final sync
      if (blockIdx.x == 0 && nonfinite && !(fabsf(s_step) <= 3.0e38f)) *nonfinite = 1;
    }
  }
  __syncthreads();
  const float step = s_step;
  const float nz = sqrtf(step * 2.f);
  strided_update(x, x_mean, net, net_stride, z, std, per, total, [=](float xi, float score, float zi) {
    const float xm = xi + step * score;
    return make_float2(xm, xm + nz * zi);
  });
}

// global-norm exactness mode: sums[0] = sum_b ||net_b||/std, sums[1] = sum_b ||z_b|| over THIS rank's samples,
// fp32 like the reference's torch.norm(...).mean() operands; the caller all-reduces the two floats over the ranks
__global__ __launch_bounds__(64) void norm_sums_kernel(const double* __restrict__ partial, int nchunk, float std, int B,
                                                       float* __restrict__ sums) {
  double g = 0, n = 0;
  for (int b = threadIdx.x; b < B; b += 64) {
    double sa = 0, sb = 0;
    for (int c = 0; c < nchunk; ++c) {
      sa += partial[((size_t)b * nchunk + c) * 2 + 0];
      sb += partial[((size_t)b * nchunk + c) * 2 + 1];
    }
    g += sqrt(sa) / (double)std;
    n += sqrt(sb);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    g += __shfl_xor(g, off);
    n += __shfl_xor(n, off);
  }
  if (threadIdx.x == 0) { sums[0] = (float)g; sums[1] = (float)n; }
}

// the Langevin update with the step size of the GLOBAL batch: gbar = sums[0] / Bg, nbar = sums[1] / Bg
__global__ __launch_bounds__(256) void langevin_update_global_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                                     const float* __restrict__ net, int64_t net_stride,
                                                                     const float* __restrict__ z,
                                                                     const float* __restrict__ sums, int Bg, float std,
                                                                     float snr, float alpha, int64_t per, size_t total,
                                                                     int* __restrict__ nonfinite) {
  const float gbar = sums[0] / (float)Bg, nbar = sums[1] / (float)Bg;
  const float r = snr * nbar / gbar;
  const float step = r * r * 2.f * alpha;
  if (blockIdx.x == 0 && threadIdx.x == 0 && nonfinite && !(fabsf(step) <= 3.0e38f)) *nonfinite = 1;
  const float nz = sqrtf(step * 2.f);
  strided_update(x, x_mean, net, net_stride, z, std, per, total, [=](float xi, float score, float zi) {
    const float xm = xi + step * score;
    return make_float2(xm, xm + nz * zi);
  });
}

__global__ __launch_bounds__(256) void reverse_diffusion_update_kernel(float* __restrict__ x,
                                                                       float* __restrict__ x_mean,
                                                                       const float* __restrict__ net,
                                                                       int64_t net_stride,
                                                                       const float* __restrict__ z, float std,
                                                                       float G, int64_t per, size_t total) {
  const float G2 = G * G;
  strided_update(x, x_mean, net, net_stride, z, std, per, total, [=](float xi, float score, float zi) {
    const float rev_f = 0.f - G2 * score;   // f = 0 for VE
    const float xm = xi - rev_f;
    return make_float2(xm, xm + G * zi);
  });
}

// the reverse-diffusion update of an SDE with a linear forward drift, and of the probability flow of any SDE, in the reference's order
// of operations: f = (a*x)*b, minus x when sub_x (VP discretize: a = sqrt(alpha_i), b = 1; Euler default of sub-VP: a = phi(t),
// b = dt, sub_x = 0; drift == 0: f = 0, the VE SDEs); rev_f = f - G^2*score*kappa; x_mean = x - rev_f; x = x_mean + g_noise*z
__global__ __launch_bounds__(256) void reverse_diffusion_drift_update_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                                             const float* __restrict__ net, int64_t net_stride,
                                                                             const float* __restrict__ z, float std, float G,
                                                                             float a, float b, int drift, int sub_x, float kappa,
                                                                             float g_noise, int64_t per, size_t total) {
  const float G2 = G * G;
  strided_update(x, x_mean, net, net_stride, z, std, per, total, [=](float xi, float score, float zi) {
    float f = 0.f;
    if (drift) {
      f = (a * xi) * b;
      if (sub_x) f = f - xi;
    }
    const float rev_f = f - (G2 * score) * kappa;
    const float xm = xi - rev_f;
    return make_float2(xm, xm + g_noise * zi);
  });
}

// x_mean = p*x + (a/std)*net, x = x_mean + c*z on the network's (row-strided) output: the affine update rules inside the fused loop
__global__ __launch_bounds__(256) void affine_net_update_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                                const float* __restrict__ net, int64_t net_stride,
                                                                const float* __restrict__ z, float std, float p, float a, float c,
                                                                int64_t per, size_t total) {
  strided_update(x, x_mean, net, net_stride, z, std, per, total, [=](float xi, float score, float zi) {
    const float xm = p * xi + a * score;
    return make_float2(xm, xm + c * zi);
  });
}

// out[b] = ||a_b||_2 (fp64 sum of squares, one workgroup per sample): the per-sample norms of the Langevin step size
// (sampling/correctors.py:102-103) for callers that combine them across ranks before the update
__global__ __launch_bounds__(256) void row_norms_kernel(const float* __restrict__ a, float* __restrict__ out, int64_t per) {
  __shared__ double red[4];
  const float* p = a + (size_t)blockIdx.x * per;
  double s = 0;
  for (int64_t i = threadIdx.x; i < per; i += 256) { const float v = p[i]; s += (double)v * v; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (float)sqrt(red[0] + red[1] + red[2] + red[3]);
}

// general one-step update shared by the Euler-Maruyama / ancestral-sampling predictors and the annealed
// Langevin corrector (sampling/predictors.py:52-76,105-179, correctors.py:111-142 of the reference): with
// per-call scalars p, a, c     x_mean = p*x + a*score,   x = x_mean + c*z
__global__ __launch_bounds__(256) void affine_noise_update_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                                  const float* __restrict__ score,
                                                                  const float* __restrict__ z, float p, float a,
                                                                  float c, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const float xm = p * x[i] + a * score[i];
    x_mean[i] = xm;
    x[i] = xm + c * z[i];
  }
}

// ---- Philox4x32-10 + Box-Muller: philox_normal4 (common.h) ----------------------------------------
__global__ void randn_kernel(float* __restrict__ out, size_t n, uint64_t seed, uint64_t stream_id) {
  const size_t n4 = (n + 3) / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    float v[4];
    philox_normal4(i, seed, stream_id, v);
    const size_t base = i * 4;
    if (base + 3 < n) {
      *reinterpret_cast<float4*>(out + base) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int j = 0; j < 4 && base + j < n; ++j) out[base + j] = v[j];
    }
  }
}

// the 4-wide accessors of the two blend kernels: a group of 4 consecutive floats as one float4 (full), or its first cnt elements
__device__ __forceinline__ void load4(const float* p, bool full, int cnt, float v[4]) {
  if (full) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
    for (int j = 0; j < cnt; ++j) v[j] = p[j];
  }
}

__device__ __forceinline__ void store4(float* p, bool full, int cnt, const float v[4]) {
  if (full) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int j = 0; j < cnt; ++j) p[j] = v[j];
  }
}

// inpainting: re-impose the known pixels after an update (sampling/unconditional.py:268-271), in the reference's order of operations:
//   masked_mean = m*data ; masked = masked_mean + std*z ; x = x*(1 - mask) + masked*mask ; x_mean = x*(1 - mask) + masked_mean*mask
// (x_mean from the NEW x).  m, std: per-call scalars (all samples share one time).  z: the tape, or - z == nullptr and draw - the
// normals of (seed, stream_id) made in registers with randn_kernel's mapping (one thread = one Philox counter = 4 consecutive
// elements), which saves the write and the read of a noise buffer; neither: masked = masked_mean (std == 0, the initial state).
// vec: every pointer is 16-byte aligned - full groups move as float4, the last partial group and unaligned tensors element-wise.
__global__ __launch_bounds__(256) void inpaint_blend_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                            const float* __restrict__ data, const float* __restrict__ mask,
                                                            const float* __restrict__ z, float m, float std, size_t n, uint64_t seed,
                                                            uint64_t stream_id, int draw, int vec) {
  const size_t n4 = (n + 3) / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t base = i * 4;
    const bool full = vec && base + 3 < n;
    const int cnt = base + 3 < n ? 4 : (int)(n - base);
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f}, mk[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f};
    load4(x + base, full, cnt, xv);
    load4(data + base, full, cnt, dv);
    load4(mask + base, full, cnt, mk);
    if (z) load4(z + base, full, cnt, zv);
    if (!z && draw) philox_normal4(i, seed, stream_id, zv);
    float xn[4], xm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float masked_mean = m * dv[j];
      const float masked = (z || draw) ? masked_mean + std * zv[j] : masked_mean;
      const float keep = 1.f - mk[j];
      xn[j] = xv[j] * keep + masked * mk[j];
      xm[j] = xn[j] * keep + masked_mean * mk[j];
    }
    store4(x + base, full, cnt, xn);
    if (x_mean) store4(x_mean + base, full, cnt, xm);
  }
}

// colorization: re-impose the gray channel after an update (controllable_generation.py:143-154 of the reference).  With
//   decouple(v)[j] = sum_i v[i]*M[i][j], couple = the same contraction with M^-1, and channel 0 of the decoupled space the gray one:
//   masked_mean = m*gray0 ; masked = masked_mean + z0*std ; x = couple(masked, decouple(x)[1], decouple(x)[2]) ;
//   x_mean = couple(masked_mean, decouple(x)[1], decouple(x)[2]) with the NEW x (a second decouple).
// init: the initial state (:180-182), x holding the prior: couple(decouple(gray)*mask + decouple(prior*(1 - mask))) - the prior loses
// its channel 0 in IMAGE space, so channel 0 of the sum is m*gray0 + decouple(0, prior1, prior2)[0].
// One thread owns 4 consecutive pixels of one sample in all three planes.  z: a tape tensor of the state's size whose channel-0 plane
// is read, or - z == nullptr and draw - the same elements of a full-size randn fill of (seed, stream_id): element e is lane e % 4 of
// counter e / 4, so a group whose first element is no multiple of 4 takes its lanes from two counters.  Every contraction is
// (v0*A0j + v1*A1j) + v2*A2j.  vec: every pointer is 16-byte aligned and hw % 4 == 0 - the planes move as float4, else element-wise.
struct ColorMatrix { float m[3][3], inv[3][3]; };

__device__ __forceinline__ void mat3_contract(const float (&a)[3][3], float v0, float v1, float v2, float out[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = (v0 * a[0][j] + v1 * a[1][j]) + v2 * a[2][j];
}

__global__ __launch_bounds__(256) void colorize_blend_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                             const float* __restrict__ gray0, const float* __restrict__ z, float m,
                                                             float std, size_t hw, size_t groups, size_t total, ColorMatrix cm,
                                                             uint64_t seed, uint64_t stream_id, int draw, int init, int vec) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / groups, p = (i - b * groups) * 4;
    const int cnt = p + 3 < hw ? 4 : (int)(hw - p);
    const bool full = vec && cnt == 4;
    const size_t e0 = b * 3 * hw + p;                // the group's first element in channel 0 of the state (and of a full-size draw)
    float c[3][4] = {}, g0[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k) load4(x + e0 + k * hw, full, cnt, c[k]);
    load4(gray0 + b * hw + p, full, cnt, g0);
    if (z) {
      load4(z + e0, full, cnt, zv);
    } else if (draw) {
      const int off = (int)(e0 & 3);
      float lo[4], hi[4] = {0.f, 0.f, 0.f, 0.f};
      philox_normal4(e0 >> 2, seed, stream_id, lo);
      if (off) philox_normal4((e0 >> 2) + 1, seed, stream_id, hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) zv[j] = off + j < 4 ? lo[(off + j) & 3] : hi[(off + j) & 3];
    }
    float xn[3][4], xm[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float d[3], o[3];
      const float masked_mean = m * g0[j];
      if (init) {
        mat3_contract(cm.m, c[0][j] * 0.f, c[1][j], c[2][j], d);
        d[0] = masked_mean + d[0];
      } else {
        mat3_contract(cm.m, c[0][j], c[1][j], c[2][j], d);
        d[0] = (z || draw) ? masked_mean + zv[j] * std : masked_mean;
      }
      mat3_contract(cm.inv, d[0], d[1], d[2], o);
      xn[0][j] = o[0]; xn[1][j] = o[1]; xn[2][j] = o[2];
      if (x_mean) {
        mat3_contract(cm.m, o[0], o[1], o[2], d);
        mat3_contract(cm.inv, masked_mean, d[1], d[2], o);
        xm[0][j] = o[0]; xm[1][j] = o[1]; xm[2][j] = o[2];
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      store4(x + e0 + k * hw, full, cnt, xn[k]);
      if (x_mean) store4(x_mean + e0 + k * hw, full, cnt, xm[k]);
    }
  }
}

// gray0 = decouple(gray)[:, 0]: [B, 3, hw] -> [B, 1, hw], once per sampler call
__global__ __launch_bounds__(256) void colorize_gray0_kernel(const float* __restrict__ gray, float* __restrict__ gray0, size_t hw,
                                                             size_t total, float m00, float m10, float m20) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / hw;
    const float* g = gray + b * 3 * hw + (i - b * hw);
    gray0[i] = (g[0] * m00 + g[hw] * m10) + g[2 * hw] * m20;
  }
}

__global__ void scale_rows_kernel(float* __restrict__ out, const float* __restrict__ in,
                                  const float* __restrict__ scale, int divide, size_t per, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const float sc = scale[i / per];
    out[i] = divide ? in[i] / sc : in[i] * sc;
  }
}

// the finiteness contract for loops without a Langevin corrector, and for the state the loop returns: one pass over x at the END
__global__ __launch_bounds__(256) void finite_check_kernel(const float* __restrict__ x, size_t total, int* __restrict__ nonfinite) {
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) bad |= !(fabsf(x[i]) <= 3.0e38f);
  if (bad) *nonfinite = 1;
}

static int ew_grid(size_t total) { return (int)std::min<size_t>(cdiv64(total, 256), 4096); }

// the launch of a grid-stride kernel over `work` items: 256 threads, at most 4096 workgroups
template <class Kernel, class... Args>
static int ew_launch(Kernel kernel, size_t work, hipStream_t s, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(ew_grid(work)), dim3(256), 0, s, args...);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

int finite_check_launch(const float* x, size_t total, int* nonfinite, hipStream_t s) {
  return ew_launch(finite_check_kernel, total, s, x, total, nonfinite);
}

int sumsq_rows_launch(const float* net, int64_t net_stride, const float* z, double* partial, int B, int64_t per,
                      int nchunk, hipStream_t s) {
  hipLaunchKernelGGL(sumsq_rows_kernel, dim3(nchunk, B), dim3(SQ_THREADS), 0, s, net, net_stride, z, partial, per,
                     nchunk);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

int langevin_update_launch(float* x, float* x_mean, const float* net, int64_t net_stride, const float* z,
                           const double* partial, int nchunk, float std, float snr, float alpha, int B, int64_t per,
                           hipStream_t s, int* nonfinite) {
  const size_t total = (size_t)B * per;
  return ew_launch(langevin_update_kernel, total, s, x, x_mean, net, net_stride, z, partial, nchunk, std, snr, alpha, B, per, total,
                   nonfinite);
}

int norm_sums_launch(const double* partial, int nchunk, float std, int B, float* sums, hipStream_t s) {
  hipLaunchKernelGGL(norm_sums_kernel, dim3(1), dim3(64), 0, s, partial, nchunk, std, B, sums);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

int langevin_update_global_launch(float* x, float* x_mean, const float* net, int64_t net_stride, const float* z,
                                  const float* sums, int Bg, float std, float snr, float alpha, int B, int64_t per,
                                  hipStream_t s, int* nonfinite) {
  const size_t total = (size_t)B * per;
  return ew_launch(langevin_update_global_kernel, total, s, x, x_mean, net, net_stride, z, sums, Bg, std, snr, alpha, per, total,
                   nonfinite);
}

int reverse_diffusion_update_launch(float* x, float* x_mean, const float* net, int64_t net_stride, const float* z,
                                    float std, float G, int B, int64_t per, hipStream_t s) {
  const size_t total = (size_t)B * per;
  return ew_launch(reverse_diffusion_update_kernel, total, s, x, x_mean, net, net_stride, z, std, G, per, total);
}

int reverse_diffusion_drift_update_launch(float* x, float* x_mean, const float* net, int64_t net_stride, const float* z, float std,
                                          float G, float a, float b, int drift, int sub_x, float kappa, float g_noise, int B,
                                          int64_t per, hipStream_t s) {
  const size_t total = (size_t)B * per;
  return ew_launch(reverse_diffusion_drift_update_kernel, total, s, x, x_mean, net, net_stride, z, std, G, a, b, drift, sub_x, kappa,
                   g_noise, per, total);
}

int affine_net_update_launch(float* x, float* x_mean, const float* net, int64_t net_stride, const float* z, float std, float p,
                             float a, float c, int B, int64_t per, hipStream_t s) {
  const size_t total = (size_t)B * per;
  return ew_launch(affine_net_update_kernel, total, s, x, x_mean, net, net_stride, z, std, p, a, c, per, total);
}

int affine_noise_update_launch(float* x, float* x_mean, const float* score, const float* z, float p, float a, float c,
                               size_t total, hipStream_t s) {
  return ew_launch(affine_noise_update_kernel, total, s, x, x_mean, score, z, p, a, c, total);
}

int randn_launch(float* out, int64_t n, uint64_t seed, uint64_t stream_id, hipStream_t s) {
  if (n <= 0) return CSD_OK;
  CSD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "randn: output must be 16-byte aligned");
  return ew_launch(randn_kernel, (size_t)(n + 3) / 4, s, out, (size_t)n, seed, stream_id);
}

int inpaint_blend_launch(float* x, float* x_mean, const float* data, const float* mask, const float* z, float m, float std, size_t n,
                         uint64_t seed, uint64_t stream_id, hipStream_t s) {
  if (n == 0) return CSD_OK;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_mean) | reinterpret_cast<uintptr_t>(data) |
                         reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(z);
  CSD_REQUIRE((bits & 3) == 0, "inpaint_blend: tensors must be 4-byte aligned");
  return ew_launch(inpaint_blend_kernel, (n + 3) / 4, s, x, x_mean, data, mask, z, m, std, n, seed, stream_id,
                   (z == nullptr && std != 0.f) ? 1 : 0, (bits & 15) == 0 ? 1 : 0);
}

// the host 3 x 3 matrix M (NULL: the reference's literals, controllable_generation.py:117-119) and its inverse (NULL: the float64
// inverse of M rounded once) -> ColorMatrix; refuses max |M M^T - I| > 1e-6 and an inverse with max |M inv - I| > 1e-6
static int color_matrix(const float* matrix, const float* inv_matrix, ColorMatrix* out, const char* who) {
  static const float ref[9] = {5.7735014e-01f, -8.1649649e-01f, 4.7008697e-08f, 5.7735026e-01f, 4.0824834e-01f, 7.0710671e-01f,
                               5.7735026e-01f, 4.0824822e-01f, -7.0710683e-01f};
  const float* m = matrix ? matrix : ref;
  double worst = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += (double)m[3 * a + k] * (double)m[3 * b + k];
      const double d = std::fabs(s - (a == b ? 1.0 : 0.0));
      if (!(d <= worst)) worst = d;                  // (a NaN entry lands here too)
    }
  CSD_REQUIRE(worst <= 1e-6, "%s: the colorization matrix is not orthogonal: max |M M^T - I| = %.3e (limit 1e-6)", who, worst);
  float inv[9];
  if (inv_matrix) {
    worst = 0.0;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += (double)m[3 * a + k] * (double)inv_matrix[3 * k + b];
        const double d = std::fabs(s - (a == b ? 1.0 : 0.0));
        if (!(d <= worst)) worst = d;
      }
    CSD_REQUIRE(worst <= 1e-6, "%s: inv_matrix is not the inverse of matrix: max |M inv - I| = %.3e (limit 1e-6)", who, worst);
    std::copy(inv_matrix, inv_matrix + 9, inv);
  } else {                                           // adjugate / determinant in double
    double a[3][3], det = 0.0;
    for (int k = 0; k < 9; ++k) a[k / 3][k % 3] = m[k];
    double co[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        co[r][c] = a[(r + 1) % 3][(c + 1) % 3] * a[(r + 2) % 3][(c + 2) % 3] - a[(r + 1) % 3][(c + 2) % 3] * a[(r + 2) % 3][(c + 1) % 3];
    for (int c = 0; c < 3; ++c) det += a[0][c] * co[0][c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) inv[3 * r + c] = (float)(co[c][r] / det);
  }
  for (int k = 0; k < 9; ++k) { out->m[k / 3][k % 3] = m[k]; out->inv[k / 3][k % 3] = inv[k]; }
  return CSD_OK;
}

int colorize_blend_launch(float* x, float* x_mean, const float* gray0, const float* z, float m, float std, int B, size_t hw, int init,
                          const float* matrix, const float* inv_matrix, uint64_t seed, uint64_t stream_id, hipStream_t s) {
  ColorMatrix cm;
  int rc = color_matrix(matrix, inv_matrix, &cm, "colorize_blend");
  if (rc) return rc;
  if (B <= 0 || hw == 0) return CSD_OK;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_mean) | reinterpret_cast<uintptr_t>(gray0) |
                         reinterpret_cast<uintptr_t>(z);
  CSD_REQUIRE((bits & 3) == 0, "colorize_blend: tensors must be 4-byte aligned");
  const size_t groups = (hw + 3) / 4, total = (size_t)B * groups;
  return ew_launch(colorize_blend_kernel, total, s, x, init ? nullptr : x_mean, gray0, init ? nullptr : z, m, std, hw, groups, total, cm,
                   seed, stream_id, (!init && z == nullptr && std != 0.f) ? 1 : 0, init ? 1 : 0,
                   ((bits & 15) == 0 && hw % 4 == 0) ? 1 : 0);
}

int colorize_gray0_launch(const float* gray, float* gray0, int B, size_t hw, const float* matrix, hipStream_t s) {
  ColorMatrix cm;
  int rc = color_matrix(matrix, nullptr, &cm, "colorize_gray0");
  if (rc) return rc;
  const size_t total = (size_t)B * hw;
  if (total == 0) return CSD_OK;
  return ew_launch(colorize_gray0_kernel, total, s, gray, gray0, hw, total, cm.m[0][0], cm.m[1][0], cm.m[2][0]);
}

int scale_rows_launch(float* out, const float* in, const float* scale, int divide, int B, int64_t per,
                      hipStream_t s) {
  const size_t total = (size_t)B * per;
  if (total == 0) return CSD_OK;
  return ew_launch(scale_rows_kernel, total, s, out, in, scale, divide, (size_t)per, total);
}

// use_path bridge (sde_lib.py:323-339): y_t = w0 * y0 + w1 * y_{t+tau} + std * z, in place on the state; prev == nullptr: w1 term absent
__global__ void bridge_update_kernel(const float* __restrict__ y0, float* __restrict__ state, const float* __restrict__ z, float w0,
                                     float w1, float sd, int has_prev, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float m = has_prev ? y0[i] * w0 + state[i] * w1 : y0[i] * w0;      // (the host path: axpby(axpby(y, y_prev, w0, w1), z, 1, std))
    state[i] = m * 1.0f + z[i] * sd;
  }
}

int bridge_update_launch(const float* y0, float* state, const float* z, float w0, float w1, float sd, int has_prev, size_t n,
                         hipStream_t s) {
  const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(bridge_update_kernel, dim3(grid), dim3(256), 0, s, y0, state, z, w0, w1, sd, has_prev, n);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

}  // namespace csd

using namespace csd;

extern "C" size_t csd_update_scratch_bytes(int B) { return (size_t)B * 64 * 2 * sizeof(double); }

extern "C" int csd_langevin_step(float* x, float* x_mean, const float* net, const float* z, float std, float snr, float alpha,
                                 int B, int64_t per_sample, void* scratch, void* stream) {
  CSD_REQUIRE(B > 0 && per_sample > 0 && scratch && alpha > 0.f, "langevin_step: bad arguments");
  const int nchunk = sumsq_nchunk(per_sample);
  int rc = sumsq_rows_launch(net, per_sample, z, (double*)scratch, B, per_sample, nchunk, (hipStream_t)stream);
  if (rc) return rc;
  return langevin_update_launch(x, x_mean, net, per_sample, z, (const double*)scratch, nchunk, std, snr, alpha, B, per_sample,
                                (hipStream_t)stream);
}

extern "C" int csd_reverse_diffusion_step(float* x, float* x_mean, const float* net, const float* z, float std,
                                          float G, int B, int64_t per_sample, void* stream) {
  CSD_REQUIRE(B > 0 && per_sample > 0, "reverse_diffusion_step: bad arguments");
  return reverse_diffusion_update_launch(x, x_mean, net, per_sample, z, std, G, B, per_sample, (hipStream_t)stream);
}

extern "C" int csd_reverse_diffusion_step_ex(float* x, float* x_mean, const float* net, const float* z, float std, float G,
                                             float drift_a, float drift_b, int drift_form, float kappa, float g_noise, int B,
                                             int64_t per_sample, void* stream) {
  CSD_REQUIRE(x && x_mean && net && z && B > 0 && per_sample > 0, "reverse_diffusion_step_ex: bad arguments");
  CSD_REQUIRE(drift_form >= 0 && drift_form <= 2, "reverse_diffusion_step_ex: drift_form is 0 (none), 1 ((a*x)*b) or 2 ((a*x)*b - x)");
  return reverse_diffusion_drift_update_launch(x, x_mean, net, per_sample, z, std, G, drift_a, drift_b, drift_form != 0,
                                               drift_form == 2, kappa, g_noise, B, per_sample, (hipStream_t)stream);
}

extern "C" int csd_row_norms(const float* a, float* out, int B, int64_t per_sample, void* stream) {
  CSD_REQUIRE(a && out && B > 0 && per_sample > 0, "row_norms: bad arguments");
  hipLaunchKernelGGL(row_norms_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, out, per_sample);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

extern "C" int csd_affine_noise_step(float* x, float* x_mean, const float* score, const float* z, float p, float a,
                                     float c, int64_t n, void* stream) {
  CSD_REQUIRE(x && x_mean && score && z && n > 0, "affine_noise_step: bad arguments");
  return affine_noise_update_launch(x, x_mean, score, z, p, a, c, (size_t)n, (hipStream_t)stream);
}

extern "C" int csd_randn(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream) {
  return randn_launch(out, n, seed, stream_id, (hipStream_t)stream);
}

extern "C" int csd_scale_rows(float* out, const float* in, const float* scale, int divide, int B,
                              int64_t per_sample, void* stream) {
  return scale_rows_launch(out, in, scale, divide, B, per_sample, (hipStream_t)stream);
}

extern "C" int csd_inpaint_blend(float* x, float* x_mean, const float* data, const float* mask, const float* z, float mean_scale,
                                 float std, int64_t n, uint64_t seed, uint64_t stream_id, void* stream) {
  CSD_REQUIRE(x && data && mask && n > 0, "inpaint_blend: bad arguments");
  return inpaint_blend_launch(x, x_mean, data, mask, z, mean_scale, std, (size_t)n, seed, stream_id, (hipStream_t)stream);
}

extern "C" int csd_colorize_blend(float* x, float* x_mean, const float* gray0, const float* z, float mean_scale, float std, int B,
                                  int64_t hw, int init, const float* matrix, const float* inv_matrix, uint64_t seed,
                                  uint64_t stream_id, void* stream) {
  CSD_REQUIRE(x && gray0 && B > 0 && hw > 0 && (init == 0 || init == 1), "colorize_blend: bad arguments");
  return colorize_blend_launch(x, x_mean, gray0, z, mean_scale, std, B, (size_t)hw, init, matrix, inv_matrix, seed, stream_id,
                               (hipStream_t)stream);
}

extern "C" int csd_colorize_gray0(const float* gray, float* gray0, int B, int64_t hw, const float* matrix, void* stream) {
  CSD_REQUIRE(gray && gray0 && B > 0 && hw > 0, "colorize_gray0: bad arguments");
  return colorize_gray0_launch(gray, gray0, B, (size_t)hw, matrix, (hipStream_t)stream);
}
