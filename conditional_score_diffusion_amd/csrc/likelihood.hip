// likelihood.hip - the probability-flow ODE right-hand side of the likelihood (reference likelihood.py:53-103: get_likelihood_fn's
// ode_func with get_div_fn's Hutchinson-Skilling divergence), for a network already evaluated at the state:
//
//   drift_i = a_b x_i + c_b h_i                     f(x, t) = a_b x (every sde_lib drift is linear in x), score = s_b h,
//   dlogp_b = a_b sum eps_i^2 + c_b sum v_i eps_i   c_b = -g_b^2 s_b / 2, v = d (h . eps) / d x (csd_unet_backward_ex's d_x)
//
// One pass over the rows reads x (fp64), h, v, eps (fp32) with 16-byte loads, writes the drift (fp64) and a pair of fp64 partial sums
// per workgroup; a B-workgroup finalize adds the partials of a row in index order.  No atomics: the result is the same bits every run.
// The pass is memory-bound (28 bytes per element).
#include "common.h"

namespace {

constexpr int kThreads = 256;

// workgroups per row: enough for ~2 per CU over the whole batch, at most one per 1024 elements (one 16-byte step of every lane)
int pf_parts(int B, int64_t D) {
  const int64_t by_len = (D + 8191) / 8192;
  const int64_t by_grid = (512 + B - 1) / B;
  const int64_t cap = std::max<int64_t>(1, (D + 1023) / 1024);
  return (int)std::min<int64_t>(std::min<int64_t>(std::max(by_len, by_grid), cap), 256);
}

// fixed-order tree over the block: s[0] = sum of all lanes' values
__device__ void block_sum2(double* s0, double* s1, double v0, double v1) {
  const int t = threadIdx.x;
  s0[t] = v0; s1[t] = v1;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (t < w) { s0[t] += s0[t + w]; s1[t] += s1[t + w]; }
    __syncthreads();
  }
}

// grid (parts, B).  VEC: D, net_stride multiples of 4 (16-byte rows for the fp32 tensors, 32-byte for the fp64 ones)
template <bool VEC>
__global__ void __launch_bounds__(kThreads) pf_rhs_kernel(const double* __restrict__ y, const float* __restrict__ h,
                                                          const float* __restrict__ v, const float* __restrict__ eps, int64_t ns,
                                                          const double* __restrict__ a, const double* __restrict__ c,
                                                          double* __restrict__ out, double* __restrict__ part, int64_t D, int64_t chunk) {
  __shared__ double s0[kThreads], s1[kThreads];
  const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x;
  const int64_t lo = (int64_t)p * chunk, hi = lo + chunk < D ? lo + chunk : D;
  const double ab = a[b], cb = c[b];
  const double* yr = y + (size_t)b * D;
  double* orow = out + (size_t)b * D;
  const float* hr = h + (size_t)b * ns;
  const float* er = eps + (size_t)b * ns;
  const float* vr = v + (size_t)b * D;
  double see = 0.0, sve = 0.0;
  if (VEC) {
    for (int64_t i = lo + 4 * threadIdx.x; i < hi; i += 4 * kThreads) {
      const float4 h4 = *reinterpret_cast<const float4*>(hr + i);
      const float4 e4 = *reinterpret_cast<const float4*>(er + i);
      const float4 v4 = *reinterpret_cast<const float4*>(vr + i);
      const double2 x01 = *reinterpret_cast<const double2*>(yr + i);
      const double2 x23 = *reinterpret_cast<const double2*>(yr + i + 2);
      double2 d01, d23;
      d01.x = ab * x01.x + cb * (double)h4.x;
      d01.y = ab * x01.y + cb * (double)h4.y;
      d23.x = ab * x23.x + cb * (double)h4.z;
      d23.y = ab * x23.y + cb * (double)h4.w;
      *reinterpret_cast<double2*>(orow + i) = d01;
      *reinterpret_cast<double2*>(orow + i + 2) = d23;
      see += (double)e4.x * e4.x + (double)e4.y * e4.y + (double)e4.z * e4.z + (double)e4.w * e4.w;
      sve += (double)v4.x * e4.x + (double)v4.y * e4.y + (double)v4.z * e4.z + (double)v4.w * e4.w;
    }
  } else {
    for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
      const double e = er[i];
      orow[i] = ab * yr[i] + cb * (double)hr[i];
      see += e * e;
      sve += (double)vr[i] * e;
    }
  }
  block_sum2(s0, s1, see, sve);
  if (threadIdx.x == 0) {
    part[((size_t)b * P + p) * 2] = s0[0];
    part[((size_t)b * P + p) * 2 + 1] = s1[0];
  }
}

// one workgroup per row: the row's partials in index order
__global__ void pf_finalize_kernel(const double* __restrict__ part, int P, const double* __restrict__ a, const double* __restrict__ c,
                                   double* __restrict__ logp) {
  if (threadIdx.x != 0) return;
  const int b = blockIdx.x;
  double see = 0.0, sve = 0.0;
  for (int p = 0; p < P; ++p) {
    see += part[((size_t)b * P + p) * 2];
    sve += part[((size_t)b * P + p) * 2 + 1];
  }
  logp[b] = a[b] * see + c[b] * sve;
}

// x32 = float(y[0 : n]), labels32 = float(labels)
__global__ void pf_state_kernel(const double* __restrict__ y, float* __restrict__ x32, int64_t n, const double* __restrict__ labels,
                                float* __restrict__ labels32, int B) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = n / 4;
  for (int64_t i = tid; i < n4; i += stride) {
    const double2 a = reinterpret_cast<const double2*>(y)[2 * i];
    const double2 b = reinterpret_cast<const double2*>(y)[2 * i + 1];
    reinterpret_cast<float4*>(x32)[i] = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += stride) x32[i] = (float)y[i];
  if (labels)
    for (int64_t i = tid; i < B; i += stride) labels32[i] = (float)labels[i];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int csd_pf_ode_state(const double* y, const double* labels, float* x32, float* labels32, int B, int64_t D, void* stream) {
  CSD_REQUIRE(y && x32 && B >= 1 && D >= 1, "pf_ode_state: bad arguments");
  CSD_REQUIRE(!labels || labels32, "pf_ode_state: labels need labels32");
  CSD_REQUIRE(aligned16(y) && aligned16(x32), "pf_ode_state: y and x32 must be 16-byte aligned");
  const int64_t n = (int64_t)B * D;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n / 4 + kThreads - 1) / kThreads, 2048));
  hipLaunchKernelGGL(pf_state_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, y, x32, n, labels, labels32, B);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

extern "C" size_t csd_pf_ode_scratch_bytes(int B, int64_t D) {
  if (B < 1 || D < 1) return 0;
  return (size_t)B * pf_parts(B, D) * 2 * sizeof(double) + 256;
}

extern "C" int csd_pf_ode_rhs(const double* y, const float* h, const float* v, const float* eps, int64_t net_stride, const double* a,
                              const double* c, double* out, int B, int64_t D, void* scratch, void* stream) {
  CSD_REQUIRE(y && h && v && eps && a && c && out && scratch, "pf_ode_rhs: null argument");
  CSD_REQUIRE(B >= 1 && B <= 65535 && D >= 1 && net_stride >= D, "pf_ode_rhs: bad shape (B %d, D %lld, net_stride %lld)", B,
              (long long)D, (long long)net_stride);
  hipStream_t s = (hipStream_t)stream;
  const int P = pf_parts(B, D);
  const int64_t chunk = ((D + P - 1) / P + 3) / 4 * 4;            // (a multiple of 4: the 16-byte steps of a part stay in the part)
  const int Pg = (int)((D + chunk - 1) / chunk);                   // (<= P: no empty part)
  double* part = static_cast<double*>(scratch);
  const bool vec = D % 4 == 0 && net_stride % 4 == 0 && aligned16(y) && aligned16(h) && aligned16(v) && aligned16(eps) && aligned16(out);
  if (vec)
    hipLaunchKernelGGL(pf_rhs_kernel<true>, dim3(Pg, B), dim3(kThreads), 0, s, y, h, v, eps, net_stride, a, c, out, part, D, chunk);
  else
    hipLaunchKernelGGL(pf_rhs_kernel<false>, dim3(Pg, B), dim3(kThreads), 0, s, y, h, v, eps, net_stride, a, c, out, part, D, chunk);
  CSD_LAUNCH_CHECK();
  hipLaunchKernelGGL(pf_finalize_kernel, dim3(B), dim3(64), 0, s, part, Pg, a, c, out + (size_t)B * D);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}
