// ode_rk45.hip - the vector arithmetic of an embedded Runge-Kutta 5(4) step (Dormand-Prince) on a state that stays in device memory:
//
//   combine       out_i = y_i + h sum_{j<s} coef_j K_j,i         (a stage's argument, or the 5th-order update), optionally also
//                 x32_i = float(out_i) for i < nx                (the score network's fp32 input, in the same pass)
//   error sumsq   sum_i (h sum_{j<7} E_j K_j,i / (atol + rtol max(|y_i|, |ynew_i|)))^2
//   scaled sumsq  sum_i ((alpha u_i + beta w_i) / (atol + rtol |y_i|))^2           (the three norms of the initial-step selection)
//   drift         K_i = a_b y_i + c_b h_i                        (csd_pf_ode_rhs without the divergence sums: the ODE sampler)
//
// y, out, K are fp64; K holds 7 rows, k_stride doubles apart: row j at K + j * k_stride.  A negative stride walks the rows backwards,
// which is how the caller makes the last stage of an accepted step the first of the next (FSAL) without a copy.  The tableau rows
// arrive by value (kernel arguments), there is no device table.  Every pass is memory-bound (the combine reads up to 8 doubles and
// writes one per element, the error sum reads 9): 16-byte accesses, four elements per lane and step, a grid-stride loop over a grid
// of at most two workgroups per CU.  The sums are fixed-order: one fp64 partial per workgroup (lanes in a fixed tree), then one
// workgroup adds the partials in index order.  No atomics: the same bits on every run.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxParts = 512;            // ~2 workgroups per CU

// workgroups of a pass over n elements - the two rules of likelihood.hip's pf_parts on one row: enough for ~2 per CU, at most one
// per 1024 elements (one 16-byte step of every lane of the fp32 output)
int ode_parts(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 1023) / 1024, kMaxParts)); }

// the same rules per row of a [B, D] batch (likelihood.hip: pf_parts)
int drift_parts(int B, int64_t D) {
  const int64_t by_len = (D + 8191) / 8192;
  const int64_t by_grid = (512 + B - 1) / B;
  const int64_t cap = std::max<int64_t>(1, (D + 1023) / 1024);
  return (int)std::min<int64_t>(std::min<int64_t>(std::max(by_len, by_grid), cap), 256);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }

// fixed-order tree over the block: s[0] = sum of all lanes' values
__device__ void block_sum(double* s, double v) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (t < w) s[t] += s[t + w];
    __syncthreads();
  }
}

__device__ __forceinline__ double sq(double v) { return v * v; }

// sum_{j<s} coef_j K_j,i (j ascending)
__device__ __forceinline__ double stage_sum(const double* __restrict__ K, int64_t ks, int s, const csd_ode_coef& coef, int64_t i) {
  double acc = coef.c[0] * K[i];
#pragma unroll
  for (int j = 1; j < 7; ++j)
    if (j < s) acc += coef.c[j] * K[j * ks + i];
  return acc;
}

__device__ __forceinline__ void stage_sum4(const double* __restrict__ K, int64_t ks, int s, const csd_ode_coef& coef, int64_t i,
                                           double2& a01, double2& a23) {
  const double2 k01 = ld2(K + i), k23 = ld2(K + i + 2);
  a01.x = coef.c[0] * k01.x; a01.y = coef.c[0] * k01.y;
  a23.x = coef.c[0] * k23.x; a23.y = coef.c[0] * k23.y;
#pragma unroll
  for (int j = 1; j < 7; ++j)
    if (j < s) {
      const double* kr = K + j * ks + i;
      const double2 r01 = ld2(kr), r23 = ld2(kr + 2);
      const double cj = coef.c[j];
      a01.x += cj * r01.x; a01.y += cj * r01.y;
      a23.x += cj * r23.x; a23.y += cj * r23.y;
    }
}

// VEC: y, K, out, x32 16-byte aligned and k_stride even (every K row 16-byte aligned)
template <bool VEC>
__global__ void __launch_bounds__(kThreads) ode_combine_kernel(const double* __restrict__ y, const double* __restrict__ K, int64_t ks,
                                                               int s, csd_ode_coef coef, double h, double* __restrict__ out,
                                                               float* __restrict__ x32, int64_t nx, int64_t n) {
  const int64_t tid = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t nq = VEC ? n / 4 : 0;
  for (int64_t q = tid; q < nq; q += stride) {
    const int64_t i = 4 * q;
    double2 a01, a23;
    stage_sum4(K, ks, s, coef, i, a01, a23);
    const double2 y01 = ld2(y + i), y23 = ld2(y + i + 2);
    double2 o01, o23;
    o01.x = y01.x + h * a01.x; o01.y = y01.y + h * a01.y;
    o23.x = y23.x + h * a23.x; o23.y = y23.y + h * a23.y;
    *reinterpret_cast<double2*>(out + i) = o01;
    *reinterpret_cast<double2*>(out + i + 2) = o23;
    if (i + 4 <= nx) {
      *reinterpret_cast<float4*>(x32 + i) = make_float4((float)o01.x, (float)o01.y, (float)o23.x, (float)o23.y);
    } else if (i < nx) {                                    // (the quad that holds the end of the image rows)
      x32[i] = (float)o01.x;
      if (i + 1 < nx) x32[i + 1] = (float)o01.y;
      if (i + 2 < nx) x32[i + 2] = (float)o23.x;
    }
  }
  for (int64_t i = 4 * nq + tid; i < n; i += stride) {
    const double o = y[i] + h * stage_sum(K, ks, s, coef, i);
    out[i] = o;
    if (i < nx) x32[i] = (float)o;
  }
}

__device__ __forceinline__ double err_term(double e, double y, double yn, double atol, double rtol) {
  const double ay = fabs(y), an = fabs(yn);
  const double m = ay > an ? ay : an;                       // (a NaN in ynew stays a NaN)
  return sq(e / (atol + rtol * m));
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) ode_error_kernel(const double* __restrict__ y, const double* __restrict__ yn,
                                                             const double* __restrict__ K, int64_t ks, csd_ode_coef E, double h,
                                                             double atol, double rtol, int64_t n, double* __restrict__ part) {
  __shared__ double sm[kThreads];
  const int64_t tid = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t nq = VEC ? n / 4 : 0;
  double acc = 0.0;
  for (int64_t q = tid; q < nq; q += stride) {
    const int64_t i = 4 * q;
    double2 a01, a23;
    stage_sum4(K, ks, 7, E, i, a01, a23);
    const double2 y01 = ld2(y + i), y23 = ld2(y + i + 2), n01 = ld2(yn + i), n23 = ld2(yn + i + 2);
    acc += err_term(h * a01.x, y01.x, n01.x, atol, rtol);
    acc += err_term(h * a01.y, y01.y, n01.y, atol, rtol);
    acc += err_term(h * a23.x, y23.x, n23.x, atol, rtol);
    acc += err_term(h * a23.y, y23.y, n23.y, atol, rtol);
  }
  for (int64_t i = 4 * nq + tid; i < n; i += stride) acc += err_term(h * stage_sum(K, ks, 7, E, i), y[i], yn[i], atol, rtol);
  block_sum(sm, acc);
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

// w may be NULL (beta is then unused)
template <bool VEC>
__global__ void __launch_bounds__(kThreads) ode_scaled_kernel(const double* __restrict__ u, const double* __restrict__ w, double alpha,
                                                              double beta, const double* __restrict__ y, double atol, double rtol,
                                                              int64_t n, double* __restrict__ part) {
  __shared__ double sm[kThreads];
  const int64_t tid = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t nh = VEC ? n / 2 : 0;
  double acc = 0.0;
  for (int64_t q = tid; q < nh; q += stride) {
    const int64_t i = 2 * q;
    const double2 u2 = ld2(u + i), y2 = ld2(y + i);
    double vx = alpha * u2.x, vy = alpha * u2.y;
    if (w) {
      const double2 w2 = ld2(w + i);
      vx += beta * w2.x; vy += beta * w2.y;
    }
    acc += sq(vx / (atol + rtol * fabs(y2.x)));
    acc += sq(vy / (atol + rtol * fabs(y2.y)));
  }
  for (int64_t i = 2 * nh + tid; i < n; i += stride) {
    double v = alpha * u[i];
    if (w) v += beta * w[i];
    acc += sq(v / (atol + rtol * fabs(y[i])));
  }
  block_sum(sm, acc);
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

// one workgroup: the P <= kMaxParts partials in index order per lane, then the fixed tree
__global__ void __launch_bounds__(kThreads) ode_finalize_kernel(const double* __restrict__ part, int P, double* __restrict__ result) {
  __shared__ double sm[kThreads];
  double acc = 0.0;
  for (int p = threadIdx.x; p < P; p += kThreads) acc += part[p];
  block_sum(sm, acc);
  if (threadIdx.x == 0) result[0] = sm[0];
}

// grid (parts, B).  VEC: D, net_stride multiples of 4 and every pointer 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(kThreads) ode_drift_kernel(const double* __restrict__ y, const float* __restrict__ h, int64_t ns,
                                                             const double* __restrict__ a, const double* __restrict__ c,
                                                             double* __restrict__ out, int64_t D, int64_t chunk) {
  const int b = blockIdx.y, p = blockIdx.x;
  const int64_t lo = (int64_t)p * chunk, hi = lo + chunk < D ? lo + chunk : D;
  const double ab = a[b], cb = c[b];
  const double* yr = y + (size_t)b * D;
  double* orow = out + (size_t)b * D;
  const float* hr = h + (size_t)b * ns;
  if (VEC) {
    for (int64_t i = lo + 4 * threadIdx.x; i < hi; i += 4 * kThreads) {
      const float4 h4 = *reinterpret_cast<const float4*>(hr + i);
      const double2 x01 = ld2(yr + i), x23 = ld2(yr + i + 2);
      double2 d01, d23;
      d01.x = ab * x01.x + cb * (double)h4.x;
      d01.y = ab * x01.y + cb * (double)h4.y;
      d23.x = ab * x23.x + cb * (double)h4.z;
      d23.y = ab * x23.y + cb * (double)h4.w;
      *reinterpret_cast<double2*>(orow + i) = d01;
      *reinterpret_cast<double2*>(orow + i + 2) = d23;
    }
  } else {
    for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) orow[i] = ab * yr[i] + cb * (double)hr[i];
  }
}

bool overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + qn && b < a + pn;
}

int64_t iabs64(int64_t v) { return v < 0 ? -v : v; }

}  // namespace

extern "C" size_t csd_ode_scratch_bytes(int64_t n) {
  if (n < 1) return 0;
  return (size_t)ode_parts(n) * sizeof(double) + 256;
}

extern "C" int csd_ode_combine(const double* y, const double* K, int64_t k_stride, int s, csd_ode_coef coef, double h, double* out,
                               float* x32, int64_t nx, int64_t n, void* stream) {
  CSD_REQUIRE(y && K && out && n >= 1, "ode_combine: bad arguments");
  CSD_REQUIRE(s >= 1 && s <= 7, "ode_combine: s = %d stages, expected 1..7", s);
  CSD_REQUIRE(iabs64(k_stride) >= n, "ode_combine: |k_stride| %lld < n %lld", (long long)k_stride, (long long)n);
  CSD_REQUIRE(nx >= 0 && nx <= n && (nx == 0 || x32), "ode_combine: nx %lld outside [0, n = %lld] or x32 missing", (long long)nx,
              (long long)n);
  CSD_REQUIRE(aligned16(y) && aligned16(K) && aligned16(out) && aligned16(x32), "ode_combine: y, K, out and x32 must be 16-byte aligned");
  const size_t nb = (size_t)n * sizeof(double);
  CSD_REQUIRE(!overlap(out, nb, y, nb), "ode_combine: out aliases y");
  const double* k_lo = k_stride < 0 ? K + (s - 1) * k_stride : K;          // (the lowest of the s rows that are read)
  CSD_REQUIRE(!overlap(out, nb, k_lo, ((size_t)(s - 1) * iabs64(k_stride) + n) * sizeof(double)), "ode_combine: out aliases K");
  const int blocks = ode_parts(n);
  if (k_stride % 2 == 0)
    hipLaunchKernelGGL(ode_combine_kernel<true>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, y, K, k_stride, s, coef, h, out,
                       x32, nx, n);
  else
    hipLaunchKernelGGL(ode_combine_kernel<false>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, y, K, k_stride, s, coef, h, out,
                       x32, nx, n);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

extern "C" int csd_ode_error_sumsq(const double* y, const double* ynew, const double* K, int64_t k_stride, csd_ode_coef E, double h,
                                   double atol, double rtol, int64_t n, double* result, void* scratch, void* stream) {
  CSD_REQUIRE(y && ynew && K && result && scratch && n >= 1, "ode_error_sumsq: bad arguments");
  CSD_REQUIRE(iabs64(k_stride) >= n, "ode_error_sumsq: |k_stride| %lld < n %lld", (long long)k_stride, (long long)n);
  CSD_REQUIRE(aligned16(y) && aligned16(ynew) && aligned16(K) && aligned16(scratch),
              "ode_error_sumsq: y, ynew, K and scratch must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(scratch);
  const int P = ode_parts(n);
  if (k_stride % 2 == 0)
    hipLaunchKernelGGL(ode_error_kernel<true>, dim3(P), dim3(kThreads), 0, st, y, ynew, K, k_stride, E, h, atol, rtol, n, part);
  else
    hipLaunchKernelGGL(ode_error_kernel<false>, dim3(P), dim3(kThreads), 0, st, y, ynew, K, k_stride, E, h, atol, rtol, n, part);
  CSD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ode_finalize_kernel, dim3(1), dim3(kThreads), 0, st, part, P, result);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

extern "C" int csd_ode_scaled_sumsq(const double* u, const double* w, double alpha, double beta, const double* y, double atol,
                                    double rtol, int64_t n, double* result, void* scratch, void* stream) {
  CSD_REQUIRE(u && y && result && scratch && n >= 1, "ode_scaled_sumsq: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(scratch);
  const int P = ode_parts(n);
  if (aligned16(u) && aligned16(w) && aligned16(y))
    hipLaunchKernelGGL(ode_scaled_kernel<true>, dim3(P), dim3(kThreads), 0, st, u, w, alpha, beta, y, atol, rtol, n, part);
  else
    hipLaunchKernelGGL(ode_scaled_kernel<false>, dim3(P), dim3(kThreads), 0, st, u, w, alpha, beta, y, atol, rtol, n, part);
  CSD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ode_finalize_kernel, dim3(1), dim3(kThreads), 0, st, part, P, result);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

extern "C" int csd_ode_drift(const double* y, const float* h, int64_t net_stride, const double* a, const double* c, double* out, int B,
                             int64_t D, void* stream) {
  CSD_REQUIRE(y && h && a && c && out, "ode_drift: null argument");
  CSD_REQUIRE(B >= 1 && B <= 65535 && D >= 1 && net_stride >= D, "ode_drift: bad shape (B %d, D %lld, net_stride %lld)", B, (long long)D,
              (long long)net_stride);
  CSD_REQUIRE(out != y, "ode_drift: out aliases y");
  const int P = drift_parts(B, D);
  const int64_t chunk = ((D + P - 1) / P + 3) / 4 * 4;            // (a multiple of 4: the 16-byte steps of a part stay in the part)
  const int Pg = (int)((D + chunk - 1) / chunk);                   // (<= P: no empty part)
  const bool vec = D % 4 == 0 && net_stride % 4 == 0 && aligned16(y) && aligned16(h) && aligned16(out);
  if (vec)
    hipLaunchKernelGGL(ode_drift_kernel<true>, dim3(Pg, B), dim3(kThreads), 0, (hipStream_t)stream, y, h, net_stride, a, c, out, D, chunk);
  else
    hipLaunchKernelGGL(ode_drift_kernel<false>, dim3(Pg, B), dim3(kThreads), 0, (hipStream_t)stream, y, h, net_stride, a, c, out, D, chunk);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}
