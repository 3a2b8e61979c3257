// dsm_loss.hip - the denoising score-matching objective of a training step as two passes around the network (losses.py:55-232 of the
// reference; include/csd.h: csd_dsm_perturb, csd_dsm_residual).
//
//   perturb    x_t[b, i] = fl(fl(m_b x[b, i]) + fl(std_b z))         three single roundings: bitwise the scale_rows + scale_rows + axpby
//                                                                   route of losses._perturb (m == NULL: m_b = 1, exact)
//   residual   r = fl(fl(a_b h) + fl(b_b z)) on every element of a segment of the network's flat per-sample output row,
//              d_out = fl(fl(fl(2 w_b) a_b) r)  (the gradient of the value below with respect to h),
//              loss_rows[b] = sum over segments and elements of w_b r^2 in fp64, *loss = sum_b loss_rows[b]
//
// z is a caller's tensor (the noise tape) or - z == NULL - element b * length + i of a csd_randn fill of (seed, stream_id), made in
// registers with philox_normal4: neither pass writes or reads a noise buffer then, and both see the same normals.
// Every reduction has a fixed shape: a thread adds its groups in ascending order, a wave folds by xor-shuffles, the four wave sums and
// then the CSD_DSM_PARTS partials of a (sample, segment) are added in index order.  No atomics: two runs agree bitwise, and a sample's
// values depend on its batch position only through its Philox element numbers.
#include <algorithm>

#include "common.h"

// every product and sum below rounds once.  Plain operators under this pragma, not the __f*_rn intrinsics: those are plain operators
// too, but written in a header in front of the pragma, so the compiler fuses them after inlining
#pragma clang fp contract(off)

namespace csd {

namespace {

constexpr int kDsmThreads = 256;

// the four values of a group that starts at flat element e0 of a (seed, stream_id) fill: lane e % 4 of counter e / 4, so a group whose
// first element is no multiple of 4 takes its lanes from two counters (as colorize_blend_kernel does)
__device__ __forceinline__ void philox_group4(size_t e0, uint64_t seed, uint64_t stream_id, float zv[4]) {
  const int off = (int)(e0 & 3);
  float lo[4], hi[4] = {0.f, 0.f, 0.f, 0.f};
  philox_normal4(e0 >> 2, seed, stream_id, lo);
  if (off) philox_normal4((e0 >> 2) + 1, seed, stream_id, hi);
#pragma unroll
  for (int j = 0; j < 4; ++j) zv[j] = off + j < 4 ? lo[(off + j) & 3] : hi[(off + j) & 3];
}

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

}  // namespace

// one thread = 4 consecutive elements of the flat [B, per] tensor = one Philox counter of the fill.  vec: every pointer is 16-byte
// aligned.  per % 4 != 0: a group may span two samples, each element then looks up its own sample.
__global__ __launch_bounds__(kDsmThreads) void dsm_perturb_kernel(float* __restrict__ xt, const float* __restrict__ x,
                                                                  const float* __restrict__ m, const float* __restrict__ sd,
                                                                  const float* __restrict__ z, size_t per, size_t n, uint64_t seed,
                                                                  uint64_t stream_id, int vec) {
  const size_t n4 = (n + 3) / 4;
  const bool one_row = (per & 3) == 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t base = i * 4;
    const int cnt = base + 3 < n ? 4 : (int)(n - base);
    const bool full = vec && cnt == 4;
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    load4(x + base, full, cnt, xv);
    if (z) load4(z + base, full, cnt, zv);
    else philox_normal4(i, seed, stream_id, zv);
    const size_t b0 = base / per;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t b = one_row ? b0 : (j < cnt ? (base + j) / per : b0);
      const float xm = m ? m[b] * xv[j] : xv[j];
      const float sz = sd[b] * zv[j];
      o[j] = xm + sz;
    }
    store4(xt + base, full, cnt, o);
  }
}

struct DsmSeg {
  long long off, len;                 // floats inside a row
  const float* a;
  const float* b;
  const float* w;
  const float* z;                     // [B, len] or null = the (seed, stream) fill
  unsigned long long stream;
  int vec_net, vec_z;                 // 16-byte accesses to net / d_out, to z
};
struct DsmArgs {
  DsmSeg seg[2];
  long long gap_off[3], gap_len[3];   // the row positions outside every segment (d_out = 0 there)
  int n_seg, n_gap;
};

// grid (CSD_DSM_PARTS, B): workgroup (p, b) owns the p-th run of 4-element groups of each segment of sample b, and the p-th share of the gaps
__global__ __launch_bounds__(kDsmThreads) void dsm_residual_kernel(const float* __restrict__ net, long long net_stride, DsmArgs args,
                                                                   float* __restrict__ d_out, double* __restrict__ partials,
                                                                   uint64_t seed) {
  __shared__ double red[kDsmThreads / 64];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t row = (size_t)b * (size_t)net_stride;
  for (int s = 0; s < args.n_seg; ++s) {
    const DsmSeg& sg = args.seg[s];
    const float av = sg.a[b], bv = sg.b[b], wv = sg.w[b];
    const float c2 = (2.f * wv) * av;
    const double wd = (double)wv;
    const long long groups = (sg.len + 3) / 4, chunk = (groups + CSD_DSM_PARTS - 1) / CSD_DSM_PARTS;
    const long long g0 = (long long)p * chunk, g1 = min(groups, g0 + chunk);
    const float* hrow = net + row + sg.off;
    float* drow = d_out ? d_out + row + sg.off : nullptr;
    const float* zrow = sg.z ? sg.z + (size_t)b * (size_t)sg.len : nullptr;
    double acc = 0.0;
    for (long long g = g0 + tid; g < g1; g += kDsmThreads) {
      const long long i0 = g * 4;
      const int cnt = i0 + 3 < sg.len ? 4 : (int)(sg.len - i0);
      float hv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4];
      load4(hrow + i0, sg.vec_net && cnt == 4, cnt, hv);
      if (zrow) load4(zrow + i0, sg.vec_z && cnt == 4, cnt, zv);
      else philox_group4((size_t)b * (size_t)sg.len + (size_t)i0, seed, sg.stream, zv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float ah = av * hv[j], bz = bv * zv[j];
        const float r = j < cnt ? ah + bz : 0.f;
        dv[j] = c2 * r;
        acc = __fma_rn(wd, (double)r * (double)r, acc);
      }
      if (drow) store4(drow + i0, sg.vec_net && cnt == 4, cnt, dv);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    __syncthreads();                  // (the previous segment's read of red[] is over)
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partials[((size_t)b * args.n_seg + s) * CSD_DSM_PARTS + p] = ((red[0] + red[1]) + red[2]) + red[3];
  }
  if (d_out) {
    for (int k = 0; k < args.n_gap; ++k) {
      float* drow = d_out + row + args.gap_off[k];
      for (long long i = (long long)p * kDsmThreads + tid; i < args.gap_len[k]; i += (long long)CSD_DSM_PARTS * kDsmThreads) drow[i] = 0.f;
    }
  }
}

// loss_rows[b] = the sample's partials added in index order; *loss = the rows added in index order (one workgroup)
__global__ __launch_bounds__(kDsmThreads) void dsm_finalize_kernel(const double* __restrict__ partials, int per_row,
                                                                   double* __restrict__ loss_rows, float* __restrict__ loss, int B) {
  for (int b = threadIdx.x; b < B; b += kDsmThreads) {
    const double* q = partials + (size_t)b * per_row;
    double s = 0.0;
    for (int k = 0; k < per_row; ++k) s += q[k];
    loss_rows[b] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int b = 0; b < B; ++b) t += loss_rows[b];
    *loss = (float)t;
  }
}

static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace csd

using namespace csd;

extern "C" int csd_dsm_perturb(float* xt, const float* x, const float* m, const float* sd, const float* z, int B, int64_t per_sample,
                               uint64_t seed, uint64_t stream_id, void* stream) {
  CSD_REQUIRE(B >= 1, "dsm_perturb: B = %d, need B >= 1", B);
  CSD_REQUIRE(per_sample >= 1, "dsm_perturb: per_sample = %lld, need per_sample >= 1", (long long)per_sample);
  CSD_REQUIRE(xt && x && sd, "dsm_perturb: null pointer (xt %p, x %p, std %p)", (void*)xt, (const void*)x, (const void*)sd);
  CSD_REQUIRE(!misaligned(xt, 4) && !misaligned(x, 4) && !misaligned(m, 4) && !misaligned(sd, 4) && !misaligned(z, 4),
              "dsm_perturb: misaligned pointer: every tensor must be 4-byte aligned");
  const size_t n = (size_t)B * (size_t)per_sample;
  const int vec = !misaligned(xt, 16) && !misaligned(x, 16) && !misaligned(z, 16);
  const size_t n4 = (n + 3) / 4;
  const int grid = (int)std::min<size_t>((n4 + kDsmThreads - 1) / kDsmThreads, 4096);
  hipLaunchKernelGGL(dsm_perturb_kernel, dim3(grid), dim3(kDsmThreads), 0, (hipStream_t)stream, xt, x, m, sd, z, (size_t)per_sample, n,
                     seed, stream_id, vec);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

extern "C" int csd_dsm_residual(const float* net, int64_t net_stride, const csd_dsm_segment* segments, int n_seg, float* d_out,
                                double* partials, double* loss_rows, float* loss, int B, uint64_t seed, void* stream) {
  CSD_REQUIRE(B >= 1, "dsm_residual: B = %d, need B >= 1", B);
  CSD_REQUIRE(B <= 65535, "dsm_residual: B = %d, at most 65535 samples per call", B);
  CSD_REQUIRE(n_seg >= 1 && n_seg <= 2, "dsm_residual: n_seg = %d, need 1 or 2 segments", n_seg);
  CSD_REQUIRE(net_stride >= 1, "dsm_residual: net_stride = %lld, need net_stride >= 1", (long long)net_stride);
  CSD_REQUIRE(net && segments && partials && loss_rows && loss,
              "dsm_residual: null pointer (net %p, segments %p, partials %p, loss_rows %p, loss %p)", (const void*)net,
              (const void*)segments, (void*)partials, (void*)loss_rows, (void*)loss);
  CSD_REQUIRE(!misaligned(net, 4) && !misaligned(d_out, 4) && !misaligned(loss, 4),
              "dsm_residual: misaligned pointer: net, d_out and loss must be 4-byte aligned");
  CSD_REQUIRE(!misaligned(partials, 8) && !misaligned(loss_rows, 8),
              "dsm_residual: misaligned pointer: partials and loss_rows must be 8-byte aligned");
  DsmArgs args = {};
  args.n_seg = n_seg;
  const bool vec_row = !misaligned(net, 16) && !misaligned(d_out, 16) && net_stride % 4 == 0;
  for (int s = 0; s < n_seg; ++s) {
    const csd_dsm_segment& g = segments[s];
    CSD_REQUIRE(g.offset >= 0 && g.length >= 1 && g.offset <= net_stride && g.length <= net_stride - g.offset,
                "dsm_residual: segment %d = [%lld, %lld + %lld) lies beyond net_stride = %lld", s, (long long)g.offset,
                (long long)g.offset, (long long)g.length, (long long)net_stride);
    CSD_REQUIRE(g.a && g.b && g.w, "dsm_residual: segment %d has a null coefficient pointer (a %p, b %p, w %p)", s, (const void*)g.a,
                (const void*)g.b, (const void*)g.w);
    CSD_REQUIRE(!misaligned(g.a, 4) && !misaligned(g.b, 4) && !misaligned(g.w, 4) && !misaligned(g.z, 4),
                "dsm_residual: segment %d has a misaligned pointer: a, b, w and z must be 4-byte aligned", s);
    DsmSeg& d = args.seg[s];
    d.off = g.offset; d.len = g.length; d.a = g.a; d.b = g.b; d.w = g.w; d.z = g.z; d.stream = g.stream_id;
    d.vec_net = vec_row && g.offset % 4 == 0;
    d.vec_z = g.z && !misaligned(g.z, 16) && g.length % 4 == 0;
  }
  int order[2] = {0, 1};
  if (n_seg == 2) {
    if (segments[1].offset < segments[0].offset) std::swap(order[0], order[1]);
    const csd_dsm_segment &lo = segments[order[0]], &hi = segments[order[1]];
    CSD_REQUIRE(lo.offset + lo.length <= hi.offset, "dsm_residual: overlapping segments [%lld, %lld) and [%lld, %lld)",
                (long long)lo.offset, (long long)(lo.offset + lo.length), (long long)hi.offset, (long long)(hi.offset + hi.length));
  }
  long long pos = 0;
  for (int k = 0; k <= n_seg; ++k) {
    const long long end = k < n_seg ? segments[order[k]].offset : net_stride;
    if (end > pos) {
      args.gap_off[args.n_gap] = pos;
      args.gap_len[args.n_gap++] = end - pos;
    }
    if (k < n_seg) pos = segments[order[k]].offset + segments[order[k]].length;
  }
  hipLaunchKernelGGL(dsm_residual_kernel, dim3(CSD_DSM_PARTS, B), dim3(kDsmThreads), 0, (hipStream_t)stream, net, (long long)net_stride,
                     args, d_out, partials, seed);
  CSD_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsm_finalize_kernel, dim3(1), dim3(kDsmThreads), 0, (hipStream_t)stream, partials, n_seg * CSD_DSM_PARTS, loss_rows,
                     loss, B);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}
