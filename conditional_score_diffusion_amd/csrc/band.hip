// Band split / merge (include/csd.h: csd_band_split, csd_band_merge): the 2x2-block, stride-2 orthogonal transform between an image
// [B, C, 2S, 2S] and its four band-major bands [B, 4C, S, S] - the Haar step of the multi-scale models
// (lightning_modules/HaarMultiScaleSdeGenerativeModel.py:15-39).  Memory-bound: every element is read once and written once.
//   merge: one thread owns a dx pair (V = 1) or four of them (V = 4) of ONE image row 2i + dy: it reads the four bands at (i, j ..
//          j + V), coalesced along j, and stores 2V contiguous floats of the image (8 or 2 x 16 bytes).  The two rows of a block are
//          two threads; the second finds the bands in the cache.
//   split: a band needs both rows, so one thread owns the two dx pairs of a 2x2 block (V = 1) or of four blocks (V = 4): 8- or
//          16-byte loads on the image, coalesced 4- or 16-byte stores on the bands.
// The 4 x 4 matrix travels by value as a kernel argument (no device table, no upload).  No LDS, no scratch; every output is the
// fma chain fmaf(m3, v3, fmaf(m2, v2, fmaf(m1, v1, m0 * v0))), so a call is bitwise repeatable and independent of V.
#include "common.h"

namespace csd {

struct BandMatrix { float m[4][4]; };      // m[k][2 dy + dx]

__device__ __forceinline__ float band_dot(float m0, float m1, float m2, float m3, float v0, float v1, float v2, float v3) {
  return fmaf(m3, v3, fmaf(m2, v2, fmaf(m1, v1, m0 * v0)));
}

// total = B * C * 2S * (S / V) threads' worth of work: (b, c, row = 2i + dy, jv)
template <int V>
__global__ __launch_bounds__(256) void band_merge_kernel(const float* __restrict__ lo, size_t lo_ld, const float* __restrict__ hi,
                                                         size_t hi_ld, float* __restrict__ x, size_t x_ld, int C, int S, BandMatrix M,
                                                         size_t total) {
  const int SV = S / V;
  const size_t hw = (size_t)S * S;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(t % SV) * V;
    size_t r = t / SV;
    const int row = (int)(r % (2 * S)); r /= 2 * S;
    const int c = (int)(r % C);
    const size_t b = r / C;
    const int dy = row & 1;
    const size_t p = (size_t)(row >> 1) * S + j;
    const float* l0 = lo + b * lo_ld + (size_t)c * hw + p;
    const float* h1 = hi + b * hi_ld + (size_t)c * hw + p;
    float* dst = x + b * x_ld + ((size_t)c * 2 * S + row) * 2 * S + 2 * j;
    const float e0 = M.m[0][2 * dy], e1 = M.m[1][2 * dy], e2 = M.m[2][2 * dy], e3 = M.m[3][2 * dy];
    const float o0 = M.m[0][2 * dy + 1], o1 = M.m[1][2 * dy + 1], o2 = M.m[2][2 * dy + 1], o3 = M.m[3][2 * dy + 1];
    if constexpr (V == 4) {
      const float4 b0 = *reinterpret_cast<const float4*>(l0);
      const float4 b1 = *reinterpret_cast<const float4*>(h1);
      const float4 b2 = *reinterpret_cast<const float4*>(h1 + (size_t)C * hw);
      const float4 b3 = *reinterpret_cast<const float4*>(h1 + (size_t)2 * C * hw);
      float4 u, w;
      u.x = band_dot(e0, e1, e2, e3, b0.x, b1.x, b2.x, b3.x); u.y = band_dot(o0, o1, o2, o3, b0.x, b1.x, b2.x, b3.x);
      u.z = band_dot(e0, e1, e2, e3, b0.y, b1.y, b2.y, b3.y); u.w = band_dot(o0, o1, o2, o3, b0.y, b1.y, b2.y, b3.y);
      w.x = band_dot(e0, e1, e2, e3, b0.z, b1.z, b2.z, b3.z); w.y = band_dot(o0, o1, o2, o3, b0.z, b1.z, b2.z, b3.z);
      w.z = band_dot(e0, e1, e2, e3, b0.w, b1.w, b2.w, b3.w); w.w = band_dot(o0, o1, o2, o3, b0.w, b1.w, b2.w, b3.w);
      reinterpret_cast<float4*>(dst)[0] = u;
      reinterpret_cast<float4*>(dst)[1] = w;
    } else {
      const float b0 = l0[0], b1 = h1[0], b2 = h1[(size_t)C * hw], b3 = h1[(size_t)2 * C * hw];
      *reinterpret_cast<float2*>(dst) = make_float2(band_dot(e0, e1, e2, e3, b0, b1, b2, b3), band_dot(o0, o1, o2, o3, b0, b1, b2, b3));
    }
  }
}

// total = B * C * S * (S / V): (b, c, i, jv)
template <int V>
__global__ __launch_bounds__(256) void band_split_kernel(const float* __restrict__ x, size_t x_ld, float* __restrict__ bands,
                                                         size_t bands_ld, int C, int S, BandMatrix M, size_t total) {
  const int SV = S / V;
  const size_t hw = (size_t)S * S;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(t % SV) * V;
    size_t r = t / SV;
    const int i = (int)(r % S); r /= S;
    const int c = (int)(r % C);
    const size_t b = r / C;
    const float* top = x + b * x_ld + ((size_t)c * 2 * S + 2 * i) * 2 * S + 2 * j;
    const float* bot = top + 2 * S;
    float* dst = bands + b * bands_ld + (size_t)c * hw + (size_t)i * S + j;
    float a[V][4];                                   // per block: a00, a01, a10, a11
    if constexpr (V == 4) {
      const float4 t0 = reinterpret_cast<const float4*>(top)[0], t1 = reinterpret_cast<const float4*>(top)[1];
      const float4 u0 = reinterpret_cast<const float4*>(bot)[0], u1 = reinterpret_cast<const float4*>(bot)[1];
      a[0][0] = t0.x; a[0][1] = t0.y; a[0][2] = u0.x; a[0][3] = u0.y;
      a[1][0] = t0.z; a[1][1] = t0.w; a[1][2] = u0.z; a[1][3] = u0.w;
      a[2][0] = t1.x; a[2][1] = t1.y; a[2][2] = u1.x; a[2][3] = u1.y;
      a[3][0] = t1.z; a[3][1] = t1.w; a[3][2] = u1.z; a[3][3] = u1.w;
    } else {
      const float2 t0 = *reinterpret_cast<const float2*>(top), u0 = *reinterpret_cast<const float2*>(bot);
      a[0][0] = t0.x; a[0][1] = t0.y; a[0][2] = u0.x; a[0][3] = u0.y;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float o[V];
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = band_dot(M.m[k][0], M.m[k][1], M.m[k][2], M.m[k][3], a[v][0], a[v][1], a[v][2], a[v][3]);
      float* d = dst + (size_t)k * C * hw;
      if constexpr (V == 4) *reinterpret_cast<float4*>(d) = make_float4(o[0], o[1], o[2], o[3]);
      else d[0] = o[0];
    }
  }
}

// the host matrix (NULL: orthonormal Haar) -> BandMatrix; refuses max |M M^T - I| > 1e-6
static int band_matrix(const float* matrix, BandMatrix* out, const char* who) {
  static const float haar[16] = {.5f, .5f, .5f, .5f, .5f, -.5f, .5f, -.5f, .5f, .5f, -.5f, -.5f, .5f, -.5f, -.5f, .5f};
  const float* m = matrix ? matrix : haar;
  double worst = 0.0;
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += (double)m[4 * a + k] * (double)m[4 * b + k];
      const double d = std::fabs(s - (a == b ? 1.0 : 0.0));
      if (!(d <= worst)) worst = d;                  // (a NaN entry lands here too)
    }
  CSD_REQUIRE(worst <= 1e-6, "%s: the band matrix is not orthogonal: max |M M^T - I| = %.3e (limit 1e-6)", who, worst);
  for (int k = 0; k < 16; ++k) out->m[k / 4][k % 4] = m[k];
  return CSD_OK;
}

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int band_extents(const char* who, int B, int C, int S, const float* img, int64_t img_ld, int64_t b0_ld, int nb0, int64_t b1_ld,
                        int nb1) {
  CSD_REQUIRE(B >= 1 && C >= 1 && S >= 1 && S <= 16384, "%s: bad extents B %d, C %d, S %d", who, B, C, S);
  const int64_t hw = (int64_t)S * S;
  CSD_REQUIRE(img_ld >= 4 * C * hw && b0_ld >= nb0 * C * hw && b1_ld >= nb1 * C * hw,
              "%s: a per-sample stride is smaller than the sample (C %d, S %d: image %lld, bands %lld / %lld floats)", who, C, S,
              (long long)img_ld, (long long)b0_ld, (long long)b1_ld);
  CSD_REQUIRE((reinterpret_cast<uintptr_t>(img) & 7) == 0 && img_ld % 2 == 0, "%s: the image needs 8-byte aligned samples (an even stride)", who);
  return CSD_OK;
}

int band_merge_launch(const float* lo, int64_t lo_ld, const float* hi, int64_t hi_ld, float* x, int64_t x_ld, int B, int C, int S,
                      const float* matrix, hipStream_t s) {
  CSD_REQUIRE(lo && hi && x, "band_merge: null tensor");
  int rc = band_extents("band_merge", B, C, S, x, x_ld, lo_ld, 1, hi_ld, 3);
  if (rc) return rc;
  BandMatrix M;
  if ((rc = band_matrix(matrix, &M, "band_merge"))) return rc;
  const bool v4 = S % 4 == 0 && al16(lo) && al16(hi) && al16(x) && lo_ld % 4 == 0 && hi_ld % 4 == 0 && x_ld % 4 == 0;
  const size_t total = (size_t)B * C * 2 * S * (S / (v4 ? 4 : 1));
  const dim3 grid((unsigned)std::min<size_t>(cdiv64(total, 256), 8192));
  if (v4) hipLaunchKernelGGL(band_merge_kernel<4>, grid, dim3(256), 0, s, lo, (size_t)lo_ld, hi, (size_t)hi_ld, x, (size_t)x_ld, C, S, M, total);
  else hipLaunchKernelGGL(band_merge_kernel<1>, grid, dim3(256), 0, s, lo, (size_t)lo_ld, hi, (size_t)hi_ld, x, (size_t)x_ld, C, S, M, total);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

int band_split_launch(const float* x, int64_t x_ld, float* bands, int64_t bands_ld, int B, int C, int S, const float* matrix,
                      hipStream_t s) {
  CSD_REQUIRE(x && bands, "band_split: null tensor");
  int rc = band_extents("band_split", B, C, S, x, x_ld, bands_ld, 4, bands_ld, 4);
  if (rc) return rc;
  BandMatrix M;
  if ((rc = band_matrix(matrix, &M, "band_split"))) return rc;
  const bool v4 = S % 4 == 0 && al16(x) && al16(bands) && x_ld % 4 == 0 && bands_ld % 4 == 0;
  const size_t total = (size_t)B * C * S * (S / (v4 ? 4 : 1));
  const dim3 grid((unsigned)std::min<size_t>(cdiv64(total, 256), 8192));
  if (v4) hipLaunchKernelGGL(band_split_kernel<4>, grid, dim3(256), 0, s, x, (size_t)x_ld, bands, (size_t)bands_ld, C, S, M, total);
  else hipLaunchKernelGGL(band_split_kernel<1>, grid, dim3(256), 0, s, x, (size_t)x_ld, bands, (size_t)bands_ld, C, S, M, total);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

}  // namespace csd

extern "C" int csd_band_split(const float* x, int64_t x_ld, float* bands, int64_t bands_ld, int B, int C, int S, const float* matrix,
                              void* stream) {
  return csd::band_split_launch(x, x_ld, bands, bands_ld, B, C, S, matrix, (hipStream_t)stream);
}

extern "C" int csd_band_merge(const float* lo, int64_t lo_ld, const float* hi, int64_t hi_ld, float* x, int64_t x_ld, int B, int C, int S,
                              const float* matrix, void* stream) {
  return csd::band_merge_launch(lo, lo_ld, hi, hi_ld, x, x_ld, B, C, S, matrix, (hipStream_t)stream);
}
