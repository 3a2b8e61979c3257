// common.h - shared declarations for libcsd_hip.so (gfx950 only; no CUDA/compat paths).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/csd.h"

// Tuning switches (kernel selection A/B, occupancy pads, ablations) exist in the TUNING build only (`make tune` ->
// libcsd_hip_tune.so, selected with CSD_LIB_PATH): in the product library CSD_TUNE_ENV is a null constant, the branches it guards
// are dead code and nothing in libcsd_hip.so depends on the process environment - except the three weight-gradient A/B switches
// that tests/test_gpu_training.py::test_weight_gradient_ab_schedules_agree exercises (backward.hip, wgrad_bf16.hip).
#ifdef CSD_TUNE
#define CSD_TUNE_ENV(name) getenv(name)
#else
#define CSD_TUNE_ENV(name) (static_cast<const char*>(nullptr))
#endif

namespace csd {

// thread-local last-error text behind csd_last_error()
void set_error(const char* fmt, ...);
const char* get_error();

#define CSD_CHECK_HIP(expr)                                                         \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      csd::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return CSD_ERR_HIP;                                                           \
    }                                                                               \
  } while (0)

#define CSD_REQUIRE(cond, ...)                 \
  do {                                         \
    if (!(cond)) {                             \
      csd::set_error(__VA_ARGS__);             \
      return CSD_ERR_INVALID;                  \
    }                                          \
  } while (0)

#define CSD_LAUNCH_CHECK()                                                          \
  do {                                                                              \
    hipError_t _e = hipGetLastError();                                              \
    if (_e != hipSuccess) {                                                         \
      csd::set_error("%s:%d: kernel launch -> %s", __FILE__, __LINE__, hipGetErrorString(_e)); \
      return CSD_ERR_HIP;                                                           \
    }                                                                               \
  } while (0)

// Per-device launch state (a process may drive several GPUs): the CU count of the current device, rounded down to a multiple of the 8
// XCDs, and a per-(kernel instantiation, device) flag for attributes that are per device (hipFuncAttributeMaxDynamicSharedMemorySize).
#define CSD_MAX_DEVICES 64
static inline int current_device_index() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= CSD_MAX_DEVICES) dev = 0;
  return dev;
}
static inline int device_cu_count8() {
  static int n_cu[CSD_MAX_DEVICES] = {0};
  const int dev = current_device_index();
  if (!n_cu[dev]) {
    hipDeviceProp_t prop;
    int n = 8;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount / 8 * 8;
    n_cu[dev] = n < 8 ? 8 : n;
  }
  return n_cu[dev];
}
// once per (call site = kernel instantiation, device): allow up to 160 KB of dynamic LDS
#define CSD_SET_MAX_LDS_ONCE(kern)                                                                                       \
  do {                                                                                                                   \
    static bool _set[CSD_MAX_DEVICES] = {false};                                                                         \
    const int _dev = csd::current_device_index();                                                                        \
    if (!_set[_dev]) {                                                                                                   \
      CSD_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
      _set[_dev] = true;                                                                                                 \
    }                                                                                                                    \
  } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

#ifdef __HIPCC__
// csd_unet_config.x_squeeze: element offset, inside one sample's x block, of squeezed channel c = 4 ci + 2 dy + dx at pixel (i, j) of the
// S x S map (hw = S * S, p = i * S + j): the image [ci][2i + dy][2j + dx] of 2S x 2S.  The dx pair of a channel pair is 8 contiguous bytes.
__device__ __forceinline__ unsigned sq_image_off(int c, int p, int i, int S, int hw) {
  return (unsigned)((c >> 2) * 4 * hw + 2 * (p + i * S) + ((c >> 1) & 1) * 2 * S + (c & 1));
}
// row p / S of pixel p of an S x S map from the correctly rounded rcp_s = 1.f / S: exact for S <= 1024 (p + 0.5 < 2^23 is exact, the
// product is off by less than S * 2^-23 <= 2^-13 while (p + 0.5) / S stays 1 / (2 S) >= 2^-11 away from an integer) - three
// instructions per store where an integer division is twenty (csd_unet_create holds x_squeeze to image_size <= 1024)
__device__ __forceinline__ int sq_row(int p, float rcp_s) { return (int)(((float)p + 0.5f) * rcp_s); }
// csd_unet_config.y_scale = K: the bilinear resampling of torch's F.interpolate(mode = 'bilinear', align_corners = False, no
// antialias) between a side-s map and its K times larger side-S map, S = K s.  Upwards the source coordinate of output index o is
// max((o + 0.5) / K - 0.5, 0) = max(2o + 1 - K, 0) / (2K): the tap i0 is the integer quotient and the weight of i1 = min(i0 + 1, s - 1) is
// the remainder over 2K - exact integers, no floor of a float.  Every kernel that resamples goes through these functions, and their
// arithmetic is spelled in single roundings (no contraction left to the compiler): a value does not depend on which kernel computed it.
struct BilinTap { int i0, i1; float w1; };
__device__ __forceinline__ BilinTap bilin_up_tap(int o, int K, int s) {
  const int num = 2 * o + 1 - K;
  BilinTap t;
  t.i0 = num > 0 ? num / (2 * K) : 0;
  t.w1 = num > 0 ? __fdiv_rn((float)(num - t.i0 * 2 * K), (float)(2 * K)) : 0.f;
  t.i1 = min(t.i0 + 1, s - 1);
  return t;
}
// the value of an output pixel from its four (possibly perturbed) taps a b / c d and the weights of the second column / row, combined
// as torch does: wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d)
__device__ __forceinline__ float bilin_combine(float a, float b, float c, float d, float wx1, float wy1) {
  const float wx0 = __fsub_rn(1.f, wx1), wy0 = __fsub_rn(1.f, wy1);
  const float top = __fmaf_rn(wx1, b, __fmul_rn(wx0, a)), bot = __fmaf_rn(wx1, d, __fmul_rn(wx0, c));
  return __fmaf_rn(wy1, bot, __fmul_rn(wy0, top));
}
// the perturbation of a tap, y + sig z at LOW resolution (then the upsample, as the reference does)
__device__ __forceinline__ float bilin_perturb(float v, float z, float sig) { return __fmaf_rn(z, sig, v); }
// output pixel (oy, ox) of the upsampled plane: the four taps of `plane` [s, s] (+ sig * the same taps of `noise` when noise != null)
__device__ __forceinline__ float bilin_up(const float* __restrict__ plane, const float* __restrict__ noise, float sig, int oy, int ox,
                                          int K, int s) {
  const BilinTap ty = bilin_up_tap(oy, K, s), tx = bilin_up_tap(ox, K, s);
  const int o00 = ty.i0 * s + tx.i0, o01 = ty.i0 * s + tx.i1, o10 = ty.i1 * s + tx.i0, o11 = ty.i1 * s + tx.i1;
  float a = plane[o00], b = plane[o01], c = plane[o10], d = plane[o11];
  if (noise) {
    a = bilin_perturb(a, noise[o00], sig); b = bilin_perturb(b, noise[o01], sig);
    c = bilin_perturb(c, noise[o10], sig); d = bilin_perturb(d, noise[o11], sig);
  }
  return bilin_combine(a, b, c, d, tx.w1, ty.w1);
}
// Downwards by an integer K the same formula lands on fixed taps: K even - the mean of the 2 x 2 block at rows / columns K i + K / 2 - 1,
// K i + K / 2 (both weights 1 / 2); K odd - the single pixel K i + (K - 1) / 2.  bilin_down_first = the first of those rows / columns.
__device__ __forceinline__ int bilin_down_first(int i, int K) { return K * i + ((K & 1) ? (K - 1) / 2 : K / 2 - 1); }
__device__ __forceinline__ float bilin_down(const float* __restrict__ plane, int i, int j, int K, int S) {
  const int r = bilin_down_first(i, K), c = bilin_down_first(j, K);
  const float* q = plane + (size_t)r * S + c;
  if (K & 1) return q[0];
  return __fmul_rn(0.25f, __fadd_rn(__fadd_rn(q[0], q[1]), __fadd_rn(q[S], q[S + 1])));
}
// its adjoint at full-resolution pixel (r, c): a quarter (K odd: all) of the gradient of the block's output pixel when (r, c) is one of
// its taps, else zero.  g [s, s].
__device__ __forceinline__ float bilin_down_adjoint(const float* __restrict__ g, int r, int c, int K, int s) {
  const int i = r / K, j = c / K, fr = bilin_down_first(i, K), fc = bilin_down_first(j, K);
  const bool hit = (K & 1) ? (r == fr && c == fc) : ((r == fr || r == fr + 1) && (c == fc || c == fc + 1));
  if (!hit) return 0.f;
  const float v = g[i * s + j];
  return (K & 1) ? v : __fmul_rn(0.25f, v);
}
// Workgroup copy global -> LDS of `bytes` (a multiple of 16): DEPTH 16-byte loads per thread IN FLIGHT before the first store.  The plain
// loop `for (i = tid * 16; i < bytes; i += THREADS * 16) lds[i] = src[i]` compiles to load / s_waitcnt vmcnt(0) / ds_write per
// iteration - one L2 round trip (~0.7 us) per 4 KiB of the workgroup: the 72 - 144 KiB weight copy of a pw16 workgroup was 12 - 25 us of
// every launch, and the whole ~20 us floor of its launches on the small maps (NOTEBOOK round 6).  Addresses are clamped, not branched
// around: a guarded load sits in its own basic block behind a wait.
template <int THREADS, int DEPTH = 8>
__device__ __forceinline__ void wg_copy_to_lds(char* __restrict__ dst, const char* __restrict__ src, int bytes, int tid) {
  typedef unsigned int u4_t __attribute__((ext_vector_type(4)));
  for (int i0 = tid * 16; i0 < bytes; i0 += THREADS * 16 * DEPTH) {
    u4_t v[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      const int i = i0 + u * THREADS * 16;
      v[u] = *reinterpret_cast<const u4_t*>(src + (i < bytes ? i : i0));
    }
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      const int i = i0 + u * THREADS * 16;
      if (i < bytes) *reinterpret_cast<u4_t*>(dst + i) = v[u];
    }
  }
}
// ---- Philox4x32-10 + Box-Muller ------------------------------------------------------------------
__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3,
                                             uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
  const uint32_t n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
  const uint32_t n3 = (uint32_t)p0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

// the four standard normals of Philox counter i: key = seed, (c2, c3) = stream_id; lane j is element 4*i + j of the stream
// (every kernel that draws takes its normals from here, so a draw does not depend on which kernel made it: contraction is off inside)
__device__ __forceinline__ void philox_normal4(size_t i, uint64_t seed, uint64_t stream_id, float v[4]) {
#pragma clang fp contract(off)
  uint32_t c0 = (uint32_t)i, c1 = (uint32_t)(i >> 32), c2 = (uint32_t)stream_id, c3 = (uint32_t)(stream_id >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  // uniforms in (0,1]: (u32 + 1) * 2^-32 computed via the top 24 bits to stay exact in fp32
  const float u0 = ((float)(c0 >> 8) + 1.0f) * (1.0f / 16777216.0f);
  const float u1 = ((float)(c1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(c2 >> 8) + 1.0f) * (1.0f / 16777216.0f);
  const float u3 = ((float)(c3 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
  float s0, cs0, s1, cs1;
  sincosf(6.283185307179586f * u1, &s0, &cs0);
  sincosf(6.283185307179586f * u3, &s1, &cs1);
  v[0] = r0 * cs0; v[1] = r0 * s0; v[2] = r1 * cs1; v[3] = r1 * s1;
}
#endif
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---------------------------------------------------------------------------------------
// Caller-owned scratch buffers are described ONCE, by a layout function that asks a ScratchCarver for the buffer's regions in order and
// returns them in a struct together with bytes().  On a null base the carver only measures: that call is the csd_*_scratch_bytes
// entry.  On the caller's pointer the same calls hand out the regions: that is the operator.  A region is added, resized or moved in
// its layout function and nowhere else.
// ---------------------------------------------------------------------------------------
constexpr size_t kScratchSlack = 1024;           // trailing bytes no region owns, part of the declared size of most operator buffers ...
constexpr size_t kScratchPrefetchSlack = 4096;   // ... and of the buffers that hold a packed convolution weight (csd_conv2d, the block convolutions)
constexpr size_t kScratchGranule = 64 * sizeof(float);      // take(): a region is whole 64-float granules, so every region stays 256-byte aligned
static inline size_t scratch_floats(size_t floats) { return align_up(floats * sizeof(float), kScratchGranule) / sizeof(float); }
struct ScratchCarver {
  char* base;
  size_t off = 0, high = 0, pad = 0;
  // align_base: the caller's pointer may have any alignment - the first region starts at the next 256-byte boundary, and bytes() counts
  // the 256 bytes that can cost
  explicit ScratchCarver(void* scratch, bool align_base = false) : base(static_cast<char*>(scratch)) {
    if (align_base) {
      base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~(uintptr_t)255);
      pad = 256;
    }
  }
  template <class T> T* take_exact(size_t count) {              // count elements, no rounding (partials and weights with sizes of their own)
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
  template <class T> T* take(size_t count) { return take_exact<T>(align_up(count * sizeof(T), kScratchGranule) / sizeof(T)); }
  // regions that share bytes (two operators, one buffer): take one set, rewind(mark) to where it began, take the other
  void rewind(size_t mark) { high = off > high ? off : high; off = mark; }
  size_t bytes(size_t slack = 0) const { return (off > high ? off : high) + pad + slack; }
};
// a buffer of ONE region behind an aligned base: its declared size, and the region
static inline size_t scratch_aligned_bytes(size_t region_bytes, size_t slack = 0) {
  ScratchCarver c(nullptr, true);
  c.take_exact<char>(region_bytes);
  return c.bytes(slack);
}
template <class T> static inline T* scratch_aligned(void* scratch) { return reinterpret_cast<T*>(ScratchCarver(scratch, true).base); }

// ---------------------------------------------------------------------------------------
// Convolution as implicit GEMM on the fp32 matrix cores (conv_f32.hip)
//   M = output pixels (B*OH*OW), N = Cout, K = taps*Cin.  Activations NHWC fp32.
// ---------------------------------------------------------------------------------------
struct ConvPlan {
  // problem
  int B, IH, IW, OH, OW;    // source / output spatial size (source = before optional x2 upsample)
  int C0, C1;               // channels of source 0 / source 1 (virtual concat), Cin = C0 + C1
  int Cout;                 // real output channels
  int taps;                 // 1 or 9
  int stride, pad, up;      // out(o) reads in((o*stride + r - pad) >> up)
  // tiling (filled by conv_plan_tiles)
  int KC;                   // channels per LDS chunk (8 or 16)
  int NT;                   // 32-wide cout tiles per workgroup (1..3)
  int MT;                   // fp16 kernel: 32-pixel M tiles per workgroup (2/4); fp32 kernel: unused
  int KCS;                  // fp16 kernel, fp16 source: 16-channel sub-chunks per K stage (1 = chunk-wise)
  int LC;                   // fp16 kernel, fp16 source: 1 = loader/consumer persistent schedule (conv_f16_lc.h)
  int TH, TW;               // output tile, TH*TW <= 128
  int PH, PW;               // staged source patch
  int tiles_x, tiles_y;     // tiles over (B*OH virtual rows, OW)
  int n_groups;             // Cout tiles / NT
  int CoutPad;              // n_groups*NT*32
  size_t lds_bytes;
  int qnt;                  // quad schedule (conv_f16_q.hip): 16-cout tiles per N half; 0 = by Cout (3: Cout % 96 == 0, else 4); 1: 32-cout groups
};

struct ConvArgs {
  const float* src0;
  const float* src1;
  const float* wpack;       // [CoutPad/32][Cin/KC][taps][KC/8][64][4]
  const float* bias;        // [CoutPad] or null
  const float* temb;        // [B][temb_stride] (already offset to this layer's columns) or null
  const float* res;         // NHWC residual [B,OH,OW,Cout] or null
  const float* nscale;      // [B][Cin] GroupNorm scale (rstd*gamma) or null
  const float* nshift;      // [B][Cin]
  float* out;
  int temb_stride;
  int out_stride;           // channels of the destination tensor (NHWC) - ignored for nchw
  int out_coff;             // channel offset inside the destination tensor
  int out_nchw;             // 1: write [B,Cout,OH,OW]
  int out_sq = 0;           // out_nchw and > 0: the first out_sq channels are stored as the 2x image of csd_unet_config.x_squeeze (sq_image_off)
  int act;                  // activation applied after the norm prologue
  float out_scale;          // multiplies the final value (1, or 1/sqrt(2) for skip_rescale)
  double* stats;            // fp16 3x3 kernel: per-tile GroupNorm partials [tile][Cout][2] (sum, sum of squares) or null
  long long* dbg;           // tuning builds only (CSD_C16_TIMING): per-workgroup phase timestamps, else null
};

int conv_plan_tiles(ConvPlan* p);                       // chooses KC/NT/tile, returns csd_status
size_t conv_packed_floats(const ConvPlan& p);           // floats of the packed weight (+ slack)
// pack one weight tensor: layout 0 = OIHW [Cout_src][Cin][kh][kw], 1 = NIN [Cin][Cout_src];
// cout_off places it inside a wider (concatenated) packed tensor.
int conv_pack_weight(const ConvPlan& p, const float* w, int layout, int cin_src, int cout_src, int cout_off,
                     float* wpack, hipStream_t s);
int conv_launch(const ConvPlan& p, const ConvArgs& a, hipStream_t s);

// fp16-MFMA variant (conv_f16.hip): ns = 2 -> split hi/lo operands, 3 MFMAs per product (F16X3);
// ns = 1 -> plain fp16 operands (F16).  Covers 3x3 stride-1 (optionally nearest-x2-fused) layers whose
// Cin is a multiple of 16; everything else stays on the fp32 kernel.
bool conv16_supported(const ConvPlan& p);
int conv16_kcs(int ns, int cin);
int conv16_plan_tiles(ConvPlan* p, int ns, int kcs = 1, bool lc = false);
size_t conv16_packed_bytes(const ConvPlan& p, int ns);
int conv16_pack_weight(const ConvPlan& p, int ns, const float* w, int layout, int cin_src, int cout_src,
                       int cout_off, void* wpack, hipStream_t s);
int conv16_launch(const ConvPlan& p, int ns, const ConvArgs& a, hipStream_t s, bool in16 = false);
// "quad" schedule (conv_f16_q.hip): fp16-source 3x3 stride-1 layers with Cout % 96 == 0, four balanced waves
bool conv16q_supported(const ConvPlan& p, int ns);
size_t conv16q_packed_bytes(const ConvPlan& p, int ns);
int conv16q_pack_weight(const ConvPlan& p, int ns, const float* w, int layout, int cin_src, int cout_src, int cout_off,
                        void* wpack, hipStream_t s);
int conv16q_plan_tiles(ConvPlan* p, int ns);
// phase-decomposed Upsample on the quad schedule (ConvPlan.up == 2; conv_f16_q.hip)
bool conv16q_up4_supported(const ConvPlan& p, int ns);
bool conv16q_up4_stats_ok(const ConvPlan& p);      // (after conv16q_plan_tiles) its epilogue statistics are a function of the sample alone
size_t conv16q_up4_packed_bytes(const ConvPlan& p, int ns);
int conv16q_pack_weight_up4(const ConvPlan& p, int ns, const float* w, void* wpack, hipStream_t s);
// raw: src0 is the fp32 NHWC source itself (ns = 2, a layer without a GroupNorm in front: the kernel's staging does the hi | lo split)
int conv16q_launch(const ConvPlan& p, int ns, const ConvArgs& a, hipStream_t s, bool raw = false);
// fused-prologue schedule (conv_ff.hip): 3x3 stride-1 layers on 16 x 16 tiles that lie inside one sample, fp32 NHWC sources
// (two-source virtual concat), GroupNorm affine + activation + fp16 split applied while staging (no gn_apply16 pass)
bool convff_supported(const ConvPlan& p, int ns);
size_t convff_packed_bytes(const ConvPlan& p, int ns);
int convff_pack_weight(const ConvPlan& p, int ns, const float* w, int layout, int cin_src, int cout_src, int cout_off,
                       void* wpack, hipStream_t s);
int convff_plan_tiles(ConvPlan* p, int ns);
// the layers conv_ff runs as the software-pipelined stream of conv_xk.hip (fp32-class operands, an even number >= 4 of 16-channel stages)
bool convff_pipelined(const ConvPlan& p, int ns);
int convff_launch(const ConvPlan& p, int ns, const ConvArgs& a, hipStream_t s);
// pointwise (1x1) layers on the fp16 MFMA path (conv_pw16.hip): fp32 NHWC in / out, optional GroupNorm affine on the
// input, bias + residual epilogue; no LDS staging of activations - a pure HBM stream
bool pw16_supported(const ConvPlan& p, int ns);
size_t pw16_packed_bytes(const ConvPlan& p, int ns);
int pw16_pack_weight(const ConvPlan& p, int ns, const float* w, int layout, int cin_src, int cout_src, int cout_off,
                     void* wpack, hipStream_t s);
int pw16_launch(const ConvPlan& p, int ns, const ConvArgs& a, hipStream_t s);
// tap-partial form of a 3x3 convolution with <= 6 output channels: one pointwise contraction to 9*cout partial channels + a 9-tap gather
bool pw16_taps_supported(int cin, int cout, int ns);
int pw16_taps_cout(int cout);
int pw16_pack_weight_taps(const ConvPlan& p, int ns, const float* w, int cout, void* wpack, hipStream_t s);
int tapsum_launch(const float* part, const float* bias, const float* res, float* out, int B, int H, int W, int cout, int nchw,
                  float out_scale, hipStream_t s, int out_sq = 0);
// stem.hip: cat(x, y [+ sigma z]) + 2v - 1 + NCHW -> NHWC + the first 3 x 3 conv (<= 8 -> Cout channels) + GroupNorm tile partials, one launch
// padded channel count of an assembled network input of MORE than 8 channels: the next multiple of 16, with exact zeros in the padding
// (the one rule behind Net::in_cpad, stem_wide_kernel's Cpad and csd_input_conv; up to 8 channels each keeps its own width)
static inline int wide_cpad(int cin) { return (cin + 15) / 16 * 16; }
bool stem_supported(int Cx, int Cy, int Cout, int S, int ns);      // the kernels cover the shape
bool stem_planned(int Cx, int Cy, int Cout, int S, int ns);        // ... and a network's plan uses them for it (where they measured faster)
size_t stem_packed_bytes(int Cin, int Cout, int ns);      // Cin = Cx + Cy: <= 8 stem_kernel's layout, 9 .. 32 stem_wide_kernel's
int stem_pack_weight(const float* w, int Cin, int Cout, int ns, void* wpack, hipStream_t s);
int stem_tiles_per_image(int S);
int stem_launch(const float* x, const float* y, const float* y_noise, float y_sigma, const void* wpack, const float* bias, float* out,
                double* stats, int B, int Cx, int Cy, int Cout, int S, int centered, int ns, hipStream_t s, int x_squeeze = 0,
                int y_scale = 0, float* y_tmp = nullptr);      // (y_tmp: y_scale with y_noise - [B, Cy, S / K, S / K] floats of scratch)
// out = y + sig * z in one rounding (bilin_perturb): the low-resolution perturbation in front of the y_scale first layer
int bilinear_perturb_launch(const float* y, const float* z, float sig, float* out, size_t n, hipStream_t st);
// y16 = fp16 split of act(x*scale + shift): hi plane (and lo plane when ns == 2), NHWC halves [B*HW][C0+C1]
// statistics + finalize + apply + split of a small map in one launch (norm.hip); gn_fused16_groups() == 0: use the three-launch form
int gn_fused16_groups(int HW, int C0, int C1, int G);
int gn_fused16_launch(const float* src0, const float* src1, int C0, int C1, const float* gamma, const float* beta, float eps,
                      void* hi, void* lo, int B, int HW, int G, int act, hipStream_t s, int f8, float* nscale = nullptr,
                      float* nshift = nullptr);      // hi == nullptr: statistics only (scale / shift out)
int gn_apply16_launch(const float* src0, const float* src1, int C0, int C1, const float* nscale, const float* nshift,
                      void* hi, void* lo, int B, int HW, int act, hipStream_t s, int f8 = 0);
static inline int precision_ns(int precision) {   // CSD_PREC_* -> number of fp16 planes (0: fp32 kernel)
  return (precision == CSD_PREC_F16X3 || precision == CSD_PREC_F16F8) ? 2 : (precision == CSD_PREC_F16 ? 1 : 0);
}

// ---------------------------------------------------------------------------------------
// GroupNorm statistics -> per-(b,c) scale/shift consumed by the conv staging prologue (norm.hip)
// ---------------------------------------------------------------------------------------
struct GNPlan {
  int B, HW, C0, C1, G, nchunk;
};
size_t gn_partial_bytes(const GNPlan& p);
int gn_plan(GNPlan* p, int B, int HW, int C0, int C1, int G);
// per_channel: partial = [B * nchunk][C][2] (sum, sum of squares) per channel - the layout of the conv epilogues' tile partials
int gn_stats_launch(const GNPlan& p, const float* src0, const float* src1, double* partial,
                    hipStream_t s, int per_channel = 0);
// rs / ms (optional): the plain statistics (rstd, -mean * rstd) per (sample, channel) as well
int gn_finalize_launch(const GNPlan& p, const double* partial, const float* gamma, const float* beta,
                       float eps, float* nscale, float* nshift, hipStream_t s, float* rs = nullptr, float* ms = nullptr);
// finalize from the per-tile partials the conv epilogues wrote (ConvArgs::stats): source s has Cs channels and
// tpi_s tiles per sample, laid out [B*tpi_s][Cs][2]; p1 may be null (single source)
int gn_finalize_tiles_launch(const double* p0, int tpi0, int C0, const double* p1, int tpi1, int C1, int B, int HW, int G,
                             const float* gamma, const float* beta, float eps, float* nscale, float* nshift,
                             hipStream_t s);
// stand-alone apply: y = act(x*scale + shift), NHWC
// mask != null: y = dropout(act(x*scale + shift)) with the mask csd_dropout would draw for (seed, stream_id), written to mask
// hi (/ lo) != null: the fp16 hi (| lo) planes of y too ([B*HW][C] halves each), as gn_apply16 would split y
int gn_apply_launch(const float* x, const float* nscale, const float* nshift, float* y, int B, int HW,
                    int C, int act, hipStream_t s, float* mask = nullptr, float p_drop = 0.f, uint64_t seed = 0, uint64_t stream_id = 0,
                    void* hi = nullptr, void* lo = nullptr);
// the final writers of the planned backward's parameter gradients take `beta`: 0 stores the gradient (the C ABI's form), 1 adds it to what
// the slot holds - the fp32 value the store would have written, rounded first, then ONE fp32 addition (csd_unet_backward_acc)
// two csd_sum_rows of one shape in one launch (backward.hip)
int sum_rows2(const float* x0, float* out0, const float* x1, float* out1, int R, int C, void* stream, int beta = 0);
int sum_rows_beta(const float* x, float* out, int R, int C, int beta, void* stream);
// csd_conv2d_wgrad_ex / one csd_bgemm (batch 1) with beta (backward.hip)
int conv2d_wgrad_beta(const float* x, const float* dy, float* dw, int B, int Cin, int Cout, int H, int W, int ksize, int stride,
                      int pad_mode, int up2, int layout, void* scratch, void* stream, int beta);
int bgemm_beta(const float* A, const float* Bm, float* Cm, int M, int N, int K, int64_t sam, int64_t sak, int64_t sbk, int64_t sbn,
               int64_t scm, int64_t scn, float alpha, int beta, void* stream);
// csd_groupnorm_act_nhwc with the training forward's dropout fused into the apply pass (train_nhwc.hip)
int groupnorm_act_dropout_nhwc(const float* x, const float* gamma, const float* beta, float* y, float* rs, float* ms, float* mask,
                               float p_drop, uint64_t seed, uint64_t stream_id, int B, int C, int HW, int groups, float eps, int act,
                               void* scratch, void* stream, void* planes = nullptr, int plane_count = 0);
// the operand planes conv2d_impl would split an NHWC source into (quad schedule): 0 = it would not (other kernel), else 1 or 2 planes of
// B*H*W*Cin halves each, hi first
int conv2d_operand_planes(int B, int Cin, int Cout, int H, int W, int ksize, int stride, int pad_mode, int up2, int precision);

// ---------------------------------------------------------------------------------------
// attention core on NHWC qkv (attention.hip): qkv [B, L, ld] with q at +0, k at +C, v at +2C
// ---------------------------------------------------------------------------------------
int attention_launch(const float* qkv, int ld, float* out, int B, int L, int C, hipStream_t s);
// the same core on the fp16 matrix cores: ns = 2 split operands (3 MFMAs per product, fp32-class), ns = 1 plain fp16
int attention16_launch(const float* qkv, int ld, float* out, int B, int L, int C, int ns, hipStream_t s);

// ---------------------------------------------------------------------------------------
// small kernels (elementwise.hip)
// ---------------------------------------------------------------------------------------
int timestep_embedding_launch(const float* t, float* out, int B, int dim, hipStream_t s);
// out[b][n] = g(sum_k f(in[b][k]) * W[n][k] + bias[n]);  f = act_in, g = act_out
int linear_launch(const float* in, const float* W, const float* bias, float* out, int B, int K, int N,
                  int act_in, hipStream_t s, int act_out = 0);
// NCHW x (+ y (+ sigma*noise)) -> NHWC [B,H,W,Cpad], v -> 2v-1 unless centered
int assemble_input_launch(const float* x, const float* y, const float* y_noise, float y_sigma,
                          float* out, int B, int Cx, int Cy, int HW, int Cpad, int centered,
                          hipStream_t s, int x_squeeze = 0, int S = 0, int y_scale = 0);
// scale multiplies the kernel (after the forward gain), flip reverses the taps: the transposed operators of the training graph
int fir_resample_nhwc_launch(const float* in, float* out, int B, int H, int W, int C, const float* taps4, int up, hipStream_t s,
                             float scale = 1.f, int flip = 0);
// out_x = FIR(in), out_h = FIR(act(in * nscale + nshift)) in one pass (the up / down BigGAN block's two resampled tensors)
int fir_resample2_nhwc_launch(const float* in, const float* nscale, const float* nshift, float* out_x, float* out_h, int B, int H, int W,
                              int C, const float* taps4, int up, int act, hipStream_t s);
// NCSN++ residual input pyramid (fir_pyramid.hip): the FIR + stride-2 3x3 conv as one folded 6x6 stride-2 conv.  taps4 == NULL: fir = False
// (F.pad(0, 1, 0, 1) + stride-2 conv).  Sources / data gradients are addressed as b * sb + (Y * H + X) * sp + c * sc (NHWC or NCHW).
int fir_pyr_fold_launch(const float* w, int Cin, int Cout, const float* taps4, float* gf, float* gt, hipStream_t s);
int fir_pyr_conv_launch(const float* x, int64_t sb, int sp, int64_t sc, int B, int H, int Cin, const float* gf, const float* bias,
                        const float* res, float* out, int Cout, bool fir, float scale, hipStream_t s);
int fir_pyr_dgrad_launch(const float* dy, const float* gt, float* dx, int64_t db, int dp, int64_t dc, int B, int H, int Cin, int nc, int Cout,
                         bool fir, float scale, hipStream_t s);
int fir_pyr_wgrad_slices(int B, int Cin, int Cout);
size_t fir_pyr_wgrad_scratch_floats(int B, int Cin, int Cout);
int fir_pyr_wgrad_launch(const float* x, int64_t sb, int sp, int64_t sc, int B, int H, int Cin, const float* dy, int Cout, const float* taps4,
                         bool fir, float* dw, float* scratch, hipStream_t s, int beta = 0);
int fourier_embedding_launch(const float* t, const float* W, float* out, int B, int E, hipStream_t s);
// per-operator convolution of the C ABI (ops_api.hip) with an optional NHWC residual added in the epilogue; GroupNorm backward with
// an optional addend (train_nhwc.hip): the fused forms the planned training graph (train_graph.h) uses
int conv2d_impl(const float* x, const float* weight, const float* bias, const float* res, const float* temb, float* y, int B, int Cin,
                int Cout, int H, int W, int ksize, int stride, int pad_mode, int up2, int precision, int layout, void* scratch, void* stream,
                const void* planes = nullptr);      // planes: the pre-split operand (conv2d_operand_planes() > 0), x is then not read
int groupnorm_act_backward_nhwc_add(const float* x, const float* gamma, const float* beta, const float* rs, const float* ms,
                                    const float* dy, const float* add, float* dx, float* dgamma_rows, float* dbeta_rows,
                                    int row_stride, int B, int C, int HW, int groups, int act, void* scratch, void* stream);
// the same over x = x0 [B, HW, C0] (| x1 [B, HW, C - C0]) with the gradient written per source; acc0 / acc1 = 1: that destination already
// holds a gradient (another consumer's) and takes this one in one fp32 addition.  One source: C0 = C, x1 = dx1 = NULL
struct GnBwdSplit {
  const float* x0 = nullptr;
  const float* x1 = nullptr;
  float* dx0 = nullptr;
  float* dx1 = nullptr;
  int C0 = 0, acc0 = 0, acc1 = 0;
};
int groupnorm_act_backward_nhwc_split(const GnBwdSplit& t, const float* gamma, const float* beta, const float* rs, const float* ms,
                                      const float* dy, const float* add, float* dgamma_rows, float* dbeta_rows, int row_stride, int B, int C,
                                      int HW, int groups, int act, void* scratch, void* stream);
int axpby_launch(const float* a, const float* b, float* out, float alpha, float beta, float gamma, float post, size_t n,
                 hipStream_t s);
int bias_add_nchw_launch(const float* x, const float* bias, float* out, int B, int C, size_t inner, int bias_stride, int act,
                         hipStream_t s);
int nchw_to_nhwc_launch(const float* in, float* out, int B, int C, int HW, int Cw, int ld, hipStream_t s);
int nhwc_to_nchw_launch(const float* in, float* out, int B, int C, int HW, int Cstride, hipStream_t s);
// csd_unet_config.x_squeeze at the training graph's boundary: img [B, C / 4, 2S, 2S] (img_ld floats per sample) <-> sq [B, C, S, S]
// (sq_ld floats per sample), sq[b, 4 ci + 2 dy + dx, i, j] = img[b, ci, 2i + dy, 2j + dx]
int sq_gather_launch(const float* img, size_t img_ld, float* sq, size_t sq_ld, int B, int C, int S, hipStream_t s);
int sq_scatter_launch(const float* sq, size_t sq_ld, float* img, size_t img_ld, int B, int C, int S, hipStream_t s);
// csd_unet_config.y_scale (bilin_up / bilin_down above) on [B, C] planes; a sample's planes start at b * src_ld / b * dst_ld floats.
// up: src [., C, s, s] (+ sig * noise, same layout and stride, or null) -> dst [., C, K s, K s]; down: src [., C, S, S] -> dst
// [., C, S / K, S / K]; down_adjoint: src = the gradient [., C, S / K, S / K] -> dst [., C, S, S] (every element written)
int bilinear_up_launch(const float* src, const float* noise, float sig, size_t src_ld, float* dst, size_t dst_ld, int B, int C, int s, int K,
                       hipStream_t st);
int bilinear_down_launch(const float* src, size_t src_ld, float* dst, size_t dst_ld, int B, int C, int S, int K, hipStream_t st);
int bilinear_down_adjoint_launch(const float* src, size_t src_ld, float* dst, size_t dst_ld, int B, int C, int S, int K, hipStream_t st);
int bridge_update_launch(const float* y0, float* state, const float* z, float w0, float w1, float sd, int has_prev, size_t n,
                         hipStream_t s);
int avgpool2_launch(const float* in, float* out, int B, int H, int W, int C, hipStream_t s);
int nearest_up2_nhwc_launch(const float* in, float* out, int B, int H, int W, int C, hipStream_t s);

// conv3d.hip: csd_conv3d_block in pieces, for a caller that packs a layer's weight once (the planned 3-D network, unet3d.h).
// conv3d_launch runs the kernel csd_conv3d_block would run (same brick, same NT) on `wpack` = what conv3d_pack_launch wrote
struct Conv3dCall {
  const float* x0 = nullptr;
  const float* x1 = nullptr;
  const void* wpack = nullptr;
  const float* bias = nullptr;
  const float* nscale = nullptr;
  const float* nshift = nullptr;
  const float* temb = nullptr;
  const float* res = nullptr;
  float* out = nullptr;
  int temb_stride = 0, act = 0;
  float out_scale = 1.f;
  int B = 0, C0 = 0, C1 = 0, Cout = 0, D = 0, H = 0, W = 0, precision = 0;
};
bool conv3d_is_direct(int precision, int C0);                   // the fp32 direct kernel (CSD_PREC_F32, or C0 no multiple of 16)
size_t conv3d_wpack_size(int Cin, int Cout, bool direct);      // bytes of one packed weight (MFMA: with the weight ring's slack)
// flip_t: `weight` is the forward layer's [Cin, Cout, 3, 3, 3] and the pack is its data gradient's, weight[ci][co][26 - tap] (the values of
// packing weight.flip(2, 3, 4).transpose(0, 1), without that copy)
int conv3d_pack_launch(const float* weight, void* wpack, int Cin, int Cout, bool direct, hipStream_t s, bool flip_t = false);
int conv3d_launch(const Conv3dCall& c, hipStream_t s);
// x, y (+ y_sigma * y_noise) NCDHW -> (2v - 1 unless centered) -> 3x3x3 convolution -> NDHWC; wpack in the direct layout
int conv3d_stem_launch(const float* x, const float* y, const float* y_noise, float y_sigma, const void* wpack, const float* bias, float* out,
                       int B, int Cx, int Cy, int Cout, int D, int H, int W, int centered, hipStream_t s);

// conv3d_grad.hip: csd_conv3d_wgrad with beta (1: dw = fl32(dw + V), V the value beta = 0 stores; the split-K order is the same);
// the stem's data gradient at the network boundary: dy [B, D, H, W, Cout] NDHWC, w [Cout, Cin, 3, 3, 3] -> dx [B, nx, D, H, W] NCDHW, the
// first nx input channels, times `scale` (2 for the 2v - 1 input map): one fp32 fmaf chain per output in tap-major, cout-minor order
// ci_off, Cin_dw (> 0): `a` is ONE source of a two-source layer, dw its [Cout, Cin_dw, 27] weight gradient, of which the input-channel
// slice ci_off .. ci_off + Cin is written (each element's sum is the one a single-source call of that source gives)
int conv3d_wgrad_beta(const float* a, const float* dy, float* dw, int B, int Cin, int Cout, int D, int H, int W, int precision, void* scratch,
                      void* stream, int beta, int ci_off = 0, int Cin_dw = 0);
int conv3d_stem_dx_launch(const float* dy, const float* w, float* dx, int B, int nx, int Cin, int Cout, int D, int H, int W, float scale,
                          hipStream_t s);

// wgrad_bf16.hip: weight gradient of a stride-1 3x3 / 1x1 convolution with split-bf16 operands (NHWC x, dy; partial [S][Cout][Cin][taps])
int wgrad_bf16_launch(const float* xh, const float* dyh, float* partial, int B, int H, int W, int Cin, int Cout, int ksize, int S,
                      int per_split, hipStream_t s);

// sampler.hip
// `net` may be the x-part of a wider network output: sample b starts at net + b*net_stride
int sumsq_rows_launch(const float* net, int64_t net_stride, const float* z, double* partial, int B,
                      int64_t per, int nchunk, hipStream_t s);
int langevin_update_launch(float* x, float* x_mean, const float* net, int64_t net_stride, const float* z,
                           const double* partial, int nchunk, float std, float snr, float alpha, int B,
                           int64_t per, hipStream_t s, int* nonfinite = nullptr);
int finite_check_launch(const float* x, size_t total, int* nonfinite, hipStream_t s);
int norm_sums_launch(const double* partial, int nchunk, float std, int B, float* sums, hipStream_t s);
int langevin_update_global_launch(float* x, float* x_mean, const float* net, int64_t net_stride, const float* z,
                                  const float* sums, int Bg, float std, float snr, float alpha, int B, int64_t per,
                                  hipStream_t s, int* nonfinite = nullptr);
int affine_net_update_launch(float* x, float* x_mean, const float* net, int64_t net_stride, const float* z, float std, float p,
                             float a, float c, int B, int64_t per, hipStream_t s);
int reverse_diffusion_update_launch(float* x, float* x_mean, const float* net, int64_t net_stride,
                                    const float* z, float std, float G, int B, int64_t per, hipStream_t s);
int reverse_diffusion_drift_update_launch(float* x, float* x_mean, const float* net, int64_t net_stride, const float* z, float std,
                                          float G, float a, float b, int drift, int sub_x, float kappa, float g_noise, int B,
                                          int64_t per, hipStream_t s);
int randn_launch(float* out, int64_t n, uint64_t seed, uint64_t stream_id, hipStream_t s);
// z == nullptr: the normals of (seed, stream_id) in registers (std == 0: no draw); x_mean may be nullptr
int inpaint_blend_launch(float* x, float* x_mean, const float* data, const float* mask, const float* z, float m, float std, size_t n,
                         uint64_t seed, uint64_t stream_id, hipStream_t s);
// colorization (include/csd.h: csd_colorize_blend): x [B, 3, hw] in place, gray0 [B, 1, hw], z a full-size tape tensor or nullptr;
// init: the initial state from the prior in x; matrix / inv_matrix: host 3 x 3 or nullptr = the default / the float64 inverse
int colorize_blend_launch(float* x, float* x_mean, const float* gray0, const float* z, float m, float std, int B, size_t hw, int init,
                          const float* matrix, const float* inv_matrix, uint64_t seed, uint64_t stream_id, hipStream_t s);
int colorize_gray0_launch(const float* gray, float* gray0, int B, size_t hw, const float* matrix, hipStream_t s);
int scale_rows_launch(float* out, const float* in, const float* scale, int divide, int B, int64_t per,
                      hipStream_t s);
// csrc/band.hip (csd_band_split / csd_band_merge; matrix: host 4 x 4 or NULL = Haar, strides in floats per sample)
int band_split_launch(const float* x, int64_t x_ld, float* bands, int64_t bands_ld, int B, int C, int S, const float* matrix, hipStream_t s);
int band_merge_launch(const float* lo, int64_t lo_ld, const float* hi, int64_t hi_ld, float* x, int64_t x_ld, int B, int C, int S,
                      const float* matrix, hipStream_t s);
int sumsq_nchunk(int64_t per);

}  // namespace csd
