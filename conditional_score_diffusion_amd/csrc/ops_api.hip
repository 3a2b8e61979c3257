// ops_api.hip - C ABI of the individual operators on the reference's NCHW fp32 tensors.
// Each wrapper moves the operands into the library's NHWC layout inside caller-provided scratch,
// runs the same kernels the network executor uses, and writes NCHW.  These exist for per-op parity
// tests and for callers that use the reference's functional ops directly; the network path never
// pays these layout changes.
#include <stdlib.h>
#include <string.h>

#include "common.h"

using namespace csd;

namespace {
inline int ceil8(int v) { return (v + 7) / 8 * 8; }
inline int ceil16(int v) { return (v + 15) / 16 * 16; }
}  // namespace

// ---- GroupNorm (+activation) ---------------------------------------------------------------------
// scratch of csd_groupnorm_act: x and y in NHWC | scale, shift [B, C] | the statistics partials.  The size query does not know `groups`:
// the partials are those of CSD_GN_SCRATCH_MAX_GROUPS groups, and the operator refuses more.
struct GnScratch { float *xh, *yh, *sc, *sh; double* partial; size_t bytes; };
static GnScratch gn_scratch(void* base, int B, int C, int HW) {
  GnScratch L = {};
  GNPlan g;
  if (gn_plan(&g, B, HW, C, 0, 1)) return L;
  g.G = CSD_GN_SCRATCH_MAX_GROUPS;
  ScratchCarver c(base);
  L.xh = c.take<float>((size_t)B * HW * C);
  L.yh = c.take<float>((size_t)B * HW * C);
  L.sc = c.take<float>((size_t)B * C);
  L.sh = c.take<float>((size_t)B * C);
  L.partial = c.take_exact<double>(gn_partial_bytes(g) / sizeof(double));
  L.bytes = c.bytes(kScratchSlack);
  return L;
}

extern "C" size_t csd_groupnorm_scratch_bytes(int B, int C, int H, int W) { return gn_scratch(nullptr, B, C, H * W).bytes; }

extern "C" int csd_groupnorm_act(const float* x, const float* gamma, const float* beta, float* y, int B, int C,
                                 int H, int W, int groups, float eps, int act, void* scratch, void* stream) {
  CSD_REQUIRE(groups <= CSD_GN_SCRATCH_MAX_GROUPS, "groupnorm: %d groups, csd_groupnorm_scratch_bytes covers up to %d", groups,
              CSD_GN_SCRATCH_MAX_GROUPS);
  CSD_REQUIRE(x && gamma && beta && y && scratch, "groupnorm: null argument");
  hipStream_t s = (hipStream_t)stream;
  GNPlan g;
  int rc = gn_plan(&g, B, H * W, C, 0, groups);
  if (rc) return rc;
  const GnScratch L = gn_scratch(scratch, B, C, H * W);
  if ((rc = nchw_to_nhwc_launch(x, L.xh, B, C, H * W, C, C, s))) return rc;
  if ((rc = gn_stats_launch(g, L.xh, nullptr, L.partial, s))) return rc;
  if ((rc = gn_finalize_launch(g, L.partial, gamma, beta, eps, L.sc, L.sh, s))) return rc;
  if ((rc = gn_apply_launch(L.xh, L.sc, L.sh, L.yh, B, H * W, C, act, s))) return rc;
  return nhwc_to_nchw_launch(L.yh, y, B, C, H * W, C, s);
}

// ---- convolution ------------------------------------------------------------------------------------
static int conv_api_plan(ConvPlan* p, int B, int Cin, int Cout, int H, int W, int ksize, int stride, int pad_mode,
                         int up2) {
  CSD_REQUIRE(ksize == 1 || ksize == 3, "conv2d: ksize must be 1 or 3");
  CSD_REQUIRE(stride == 1 || stride == 2, "conv2d: stride must be 1 or 2");
  CSD_REQUIRE(!(up2 && stride != 1), "conv2d: up2 requires stride 1");
  memset(p, 0, sizeof(*p));
  p->B = B; p->IH = H; p->IW = W;
  p->C0 = ceil8(Cin); p->C1 = 0; p->Cout = Cout;
  p->taps = ksize * ksize;
  p->stride = stride; p->up = up2 ? 1 : 0;
  if (stride == 2) {
    CSD_REQUIRE(pad_mode == 1 && ksize == 3, "conv2d: stride 2 is the reference Downsample: ksize 3, pad_mode 1");
    CSD_REQUIRE(H % 2 == 0 && W % 2 == 0, "conv2d: stride-2 input must have even size");
    p->pad = 0;
  } else {
    CSD_REQUIRE(pad_mode == 0, "conv2d: stride 1 uses symmetric padding (pad_mode 0)");
    p->pad = ksize / 2;
  }
  p->OH = (H << p->up) / stride; p->OW = (W << p->up) / stride;
  return conv_plan_tiles(p);
}

static int ceil32(int c) { return (c + 31) / 32 * 32; }
static size_t api_packed_floats(const ConvPlan& p, int Cin) {
  size_t n = scratch_floats(conv_packed_floats(p)) * 2;
  {
    ConvPlan q = p;
    q.C0 = Cin; q.C1 = 0;
    if (Cin % 32 == 0 && conv16q_supported(q, 2)) {
      const size_t m = scratch_floats(conv16q_packed_bytes(q, 2) / sizeof(float) + 1);
      if (m > n) n = m;
    }
  }
  if (p.taps == 1) {
    ConvPlan q = p;
    q.C0 = ceil32(Cin);
    const size_t m = scratch_floats(pw16_packed_bytes(q, 2) / sizeof(float) + 1);
    if (m > n) n = m;
  }
  {
    ConvPlan q = p;
    q.C0 = Cin; q.C1 = 0;
    if (Cin % 16 == 0 && convff_pipelined(q, 2)) {
      const size_t m = scratch_floats(convff_packed_bytes(q, 2) / sizeof(float) + 1);
      if (m > n) n = m;
    }
  }
  return n;
}

// scratch of csd_conv2d*: the NHWC source at ceil32(Cin) channels (or its fp16 operand planes) | the packed weight, sized for the
// largest packed layout (fp32 fragments; the fp16 hi+lo layout is the same size; pointwise fp16) | the padded bias | the NHWC output.
// The size query knows neither stride nor precision: the layout is that of the stride-1 fp32 plan for every call (a stride-2 output
// is smaller, no stride-2 weight is larger).
struct ConvScratch { float *xh, *wp, *bp, *yh; size_t bytes; };
static ConvScratch conv_scratch(void* base, int B, int Cin, int Cout, int H, int W, int ksize, int up2) {
  ConvScratch L = {};
  ConvPlan p;
  if (conv_api_plan(&p, B, Cin, Cout, H, W, ksize, 1, 0, up2)) return L;
  ScratchCarver c(base);
  L.xh = c.take<float>((size_t)B * H * W * ceil32(Cin));
  L.wp = c.take<float>(api_packed_floats(p, Cin));
  L.bp = c.take<float>((size_t)p.CoutPad);
  L.yh = c.take<float>((size_t)B * p.OH * p.OW * Cout);
  L.bytes = c.bytes(kScratchPrefetchSlack);
  return L;
}

extern "C" size_t csd_conv_scratch_bytes(int B, int Cin, int Cout, int H, int W, int ksize, int up2) {
  return conv_scratch(nullptr, B, Cin, Cout, H, W, ksize, up2).bytes;
}

// layout CSD_IN_NHWC: x is NHWC [B,H,W,Cin] (Cin must already be a multiple of the kernel's channel granule); CSD_OUT_NHWC: y is NHWC;
// CSD_WEIGHT_T: `weight` is the OIHW weight [Cin][Cout][k][k] of the transposed convolution - it is used transposed and spatially flipped
// (the data gradient of a convolution, without materialising the flipped weight)
// res: optional NHWC tensor of the output's shape added in the epilogue (y NHWC only) - the block's shortcut, the attention input;
// temb: optional [B, Cout] row added per sample (Dense_0(act(temb))[:, :, None, None])
int csd::conv2d_operand_planes(int B, int Cin, int Cout, int H, int W, int ksize, int stride, int pad_mode, int up2, int precision) {
  ConvPlan p;
  if (conv_api_plan(&p, B, Cin, Cout, H, W, ksize, stride, pad_mode, up2)) return 0;
  const int ns = precision_ns(precision);
  if (!ns || Cin % 32 != 0 || CSD_TUNE_ENV("CSD_NO_Q")) return 0;
  ConvPlan q = p;
  q.C0 = Cin; q.C1 = 0;
  if (convff_pipelined(q, ns)) return 0;             // (conv_xk splits the fp32 source itself)
  return (conv16q_supported(q, ns) && conv16q_plan_tiles(&q, ns) == CSD_OK) ? (ns >= 2 ? 2 : 1) : 0;
}

int csd::conv2d_impl(const float* x, const float* weight, const float* bias, const float* res, const float* temb, float* y, int B,
                     int Cin, int Cout, int H, int W, int ksize, int stride, int pad_mode, int up2, int precision, int layout, void* scratch, void* stream,
                     const void* planes) {
  CSD_REQUIRE(x && weight && y && scratch, "conv2d: null argument");
  CSD_REQUIRE(precision >= CSD_PREC_F32 && precision <= CSD_PREC_F16F8, "conv2d: bad precision id %d", precision);
  const bool in_nhwc = layout & CSD_IN_NHWC, out_nhwc = layout & CSD_OUT_NHWC;
  CSD_REQUIRE(!res || out_nhwc, "conv2d: a residual needs an NHWC output");
  hipStream_t s = (hipStream_t)stream;
  ConvPlan p;
  int rc = conv_api_plan(&p, B, Cin, Cout, H, W, ksize, stride, pad_mode, up2);
  if (rc) return rc;
  CSD_REQUIRE(!in_nhwc || Cin % 8 == 0, "conv2d: an NHWC input needs Cin %% 8 == 0 (got %d)", Cin);
  const ConvScratch L = conv_scratch(scratch, B, Cin, Cout, H, W, ksize, up2);
  if (!L.bytes) return CSD_ERR_INVALID;
  int ns = precision_ns(precision);
  bool pw = false, quad = false;
  if (ns == 2 && in_nhwc && out_nhwc && Cin % 16 == 0) {
    // NHWC fp32 source, fp32-class arithmetic, a layer shape conv_xk.hip covers (the training graph's 3x3 convolutions and their data
    // gradients on the >= 16^2 levels): the software-pipelined block convolution without its GroupNorm prologue - it splits the fp32
    // operand into fp16 hi | lo itself, so no operand planes are written or read
    ConvPlan q = p;
    q.C0 = Cin; q.C1 = 0;
    if (convff_pipelined(q, ns)) {
      CSD_REQUIRE(!planes, "conv2d: pre-split operand planes on a layer that does not take them");
      if ((rc = convff_plan_tiles(&q, ns))) return rc;
      if ((rc = convff_pack_weight(q, ns, weight, (layout & CSD_WEIGHT_T) ? 2 : 0, Cin, Cout, 0, L.wp, s))) return rc;
      ConvArgs a;
      memset(&a, 0, sizeof(a));
      a.src0 = x; a.wpack = L.wp; a.bias = bias; a.res = res; a.temb = temb; a.temb_stride = Cout;
      a.out = y; a.out_stride = Cout; a.out_nchw = 0; a.out_scale = 1.f;
      return convff_launch(q, ns, a, s);
    }
  }
  if (ns && in_nhwc && Cin % 32 == 0 && !CSD_TUNE_ENV("CSD_NO_Q")) {
    // NHWC source (the training graph): the quad schedule of the sampling path - one split pass writes the fp16 planes into the
    // scratch region an NCHW source would be transposed into, then conv_f16_q_kernel
    ConvPlan q = p;
    q.C0 = Cin; q.C1 = 0;
    if (conv16q_supported(q, ns) && conv16q_plan_tiles(&q, ns) == CSD_OK) { p = q; quad = true; }
  }
  if (ns && !quad) {   // fp16 MFMA kernel where it applies (3x3 stride 1, Cin padded to 16), else fp32 kernel
    ConvPlan q = p;
    q.C0 = ceil16(Cin);
    ConvPlan q1 = p;
    q1.C0 = ceil32(Cin);
    if ((!in_nhwc || Cin % 16 == 0) && conv16_supported(q) && conv16_plan_tiles(&q, ns) == CSD_OK) p = q;
    else if ((!in_nhwc || Cin % 32 == 0) && pw16_supported(q1, ns)) { p = q1; pw = true; }
    else ns = 0;
  }
  float* xh = L.xh;
  float* const xh_scratch = L.xh, *const wp = L.wp, *const bp = L.bp, *const yh = L.yh;
  if (in_nhwc) xh = const_cast<float*>(x);
  else if ((rc = nchw_to_nhwc_launch(x, xh, B, Cin, H * W, p.C0, p.C0, s))) return rc;
  const int wl = (layout & CSD_WEIGHT_T) ? 2 : 0;
  CSD_REQUIRE(!planes || quad, "conv2d: pre-split operand planes on a layer that does not take them");
  if (quad) {
    void* hi = planes ? const_cast<void*>(planes) : static_cast<void*>(xh_scratch);
    void* lo = ns == 2 ? static_cast<void*>(static_cast<char*>(hi) + (size_t)B * H * W * Cin * 2) : nullptr;
    if (!planes && (rc = gn_apply16_launch(x, nullptr, Cin, 0, nullptr, nullptr, hi, lo, B, H * W, CSD_ACT_NONE, s))) return rc;
    if ((rc = conv16q_pack_weight(p, ns, weight, wl, Cin, Cout, 0, wp, s))) return rc;
    const bool bias_inplace = bias && Cout == p.CoutPad && (reinterpret_cast<uintptr_t>(bias) & 15) == 0;   // no padded copy needed
    if (bias && !bias_inplace) {
      CSD_CHECK_HIP(hipMemsetAsync(bp, 0, (size_t)p.CoutPad * sizeof(float), s));
      CSD_CHECK_HIP(hipMemcpyAsync(bp, bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src0 = static_cast<const float*>(hi); a.src1 = static_cast<const float*>(lo); a.wpack = wp;
    a.bias = bias ? (bias_inplace ? bias : bp) : nullptr;
    a.res = res; a.temb = temb; a.temb_stride = Cout;
    a.out = out_nhwc ? y : yh;
    a.out_stride = Cout; a.out_nchw = 0; a.out_scale = 1.f;
    if ((rc = conv16q_launch(p, ns, a, s))) return rc;
    if (out_nhwc) return CSD_OK;
    return nhwc_to_nchw_launch(yh, y, B, Cout, p.OH * p.OW, Cout, s);
  }
  rc = pw ? pw16_pack_weight(p, ns, weight, wl ? 1 : 0, Cin, Cout, 0, wp, s)
          : ns ? conv16_pack_weight(p, ns, weight, wl, Cin, Cout, 0, wp, s) : conv_pack_weight(p, weight, wl, Cin, Cout, 0, wp, s);
  if (rc) return rc;
  const bool bias_inplace = bias && Cout == p.CoutPad && (reinterpret_cast<uintptr_t>(bias) & 15) == 0;
  if (bias && !bias_inplace) {
    CSD_CHECK_HIP(hipMemsetAsync(bp, 0, (size_t)p.CoutPad * sizeof(float), s));
    CSD_CHECK_HIP(hipMemcpyAsync(bp, bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.src0 = xh; a.wpack = wp; a.bias = bias ? (bias_inplace ? bias : bp) : nullptr; a.out = out_nhwc ? y : yh;
  a.res = res; a.temb = temb; a.temb_stride = Cout;
  a.out_stride = Cout; a.out_nchw = 0; a.out_scale = 1.f;
  if ((rc = pw ? pw16_launch(p, ns, a, s) : ns ? conv16_launch(p, ns, a, s) : conv_launch(p, a, s))) return rc;
  if (out_nhwc) return CSD_OK;
  return nhwc_to_nchw_launch(yh, y, B, Cout, p.OH * p.OW, Cout, s);
}

extern "C" int csd_conv2d(const float* x, const float* weight, const float* bias, float* y, int B, int Cin, int Cout,
                          int H, int W, int ksize, int stride, int pad_mode, int up2, int precision, void* scratch,
                          void* stream) {
  return conv2d_impl(x, weight, bias, nullptr, nullptr, y, B, Cin, Cout, H, W, ksize, stride, pad_mode, up2, precision, 0, scratch, stream);
}

extern "C" int csd_conv2d_ex(const float* x, const float* weight, const float* bias, float* y, int B, int Cin, int Cout,
                             int H, int W, int ksize, int stride, int pad_mode, int up2, int precision, int layout,
                             void* scratch, void* stream) {
  return conv2d_impl(x, weight, bias, nullptr, nullptr, y, B, Cin, Cout, H, W, ksize, stride, pad_mode, up2, precision, layout, scratch, stream);
}

// ---- the DDPM family's first layer as an operator: cat(x, y [+ sigma z]), 2v - 1, NCHW -> NHWC, 3x3 conv to Cout channels ----------
// fused = 1: stem.hip's one launch (stem_kernel up to 8 input channels, stem_wide_kernel for 9 .. 32); fused = 0: what the plan runs
// where the fused layer does not apply - assemble_input at the padded width, then the generic convolution.  The padded width follows
// the network's rule (unet_layout.h): up to 8 channels 8 (fp32) / 16 (fp16 modes), above 8 the next multiple of 16.
static int input_conv_cpad(int cin, int ns) { return cin > 8 ? wide_cpad(cin) : (ns ? 16 : 8); }
// scratch: that of a 32-input-channel 3x3 convolution, conv_scratch(B, 32, Cout, S, S, 3, 0): the assembled input at up to 32 channels
// | the packed weight of whichever kernel takes it (none is larger than the 32-channel layouts api_packed_floats covers) | the padded bias
// (y_scale = K >= 2: y and y_noise are [B, Cy, S / K, S / K] and the layer sees the bilinear upsample of y + y_sigma y_noise -
// csd_input_conv_kx, the first layer of a csd_unet_config.y_scale network)
static int input_conv_impl(const float* x, const float* y, const float* y_noise, float y_sigma, const float* weight, const float* bias,
                           float* out, double* stats, int B, int Cx, int Cy, int Cout, int S, int centered, int precision, int fused,
                           void* scratch, void* stream, int y_scale) {
  CSD_REQUIRE(x && weight && bias && out && scratch, "input_conv: null argument");
  CSD_REQUIRE(!y_scale || (y_scale >= 2 && Cy >= 1 && Cx + Cy <= 8 && S % y_scale == 0),
              "input_conv: y_scale = %d needs y channels, up to 8 assembled channels (got %d + %d) and S %% y_scale == 0 (S = %d)", y_scale,
              Cx, Cy, S);
  CSD_REQUIRE(B >= 1 && Cx >= 1 && Cy >= 0 && Cx + Cy <= CSD_MAX_IO_CHANNELS && Cout >= 1 && S >= 1, "input_conv: bad shape");
  CSD_REQUIRE((Cy == 0) == (y == nullptr), "input_conv: y must be given iff Cy > 0");
  CSD_REQUIRE(precision >= CSD_PREC_F32 && precision <= CSD_PREC_F16F8, "input_conv: bad precision id %d", precision);
  CSD_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "input_conv: scratch must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int ns = precision_ns(precision);
  const int cin = Cx + Cy, cpad = input_conv_cpad(cin, ns);
  const ConvScratch L = conv_scratch(scratch, B, 32, Cout, S, S, 3, 0);
  if (!L.bytes) return CSD_ERR_INVALID;
  float *const xh = L.xh, *const wp = L.wp, *const bp = L.bp;
  int rc;
  if (fused) {
    CSD_REQUIRE(ns && stem_supported(Cx, Cy, Cout, S, ns), "input_conv: the fused first layer does not cover %d+%d -> %d channels at %dx%d in this precision",
                Cx, Cy, Cout, S, S);
    if ((rc = stem_pack_weight(weight, cin, Cout, ns, wp, s))) return rc;
    CSD_REQUIRE(!y_scale || (Cx <= 4 && Cy <= 4), "input_conv: the fused first layer covers y_scale up to 4 + 4 channels (got %d + %d)", Cx, Cy);
    // (y_scale: the perturbed low-resolution y goes to the head of the scratch, which the fused path does not use otherwise)
    return stem_launch(x, y, y_noise, y_sigma, wp, bias, out, stats, B, Cx, Cy, Cout, S, centered, ns, s, 0, y_scale, xh);
  }
  CSD_REQUIRE(!stats, "input_conv: tile statistics come from the fused layer only");
  ConvPlan p;
  if ((rc = conv_api_plan(&p, B, cpad, Cout, S, S, 3, 1, 0, 0))) return rc;
  if (ns) {
    CSD_REQUIRE(conv16_supported(p), "input_conv: no fp16 kernel for %d padded channels", cpad);
    if ((rc = conv16_plan_tiles(&p, ns))) return rc;
  }
  if ((rc = assemble_input_launch(x, y, y_noise, y_sigma, xh, B, Cx, Cy, S * S, cpad, centered, s, 0, S, y_scale))) return rc;
  rc = ns ? conv16_pack_weight(p, ns, weight, 0, cin, Cout, 0, wp, s) : conv_pack_weight(p, weight, 0, cin, Cout, 0, wp, s);
  if (rc) return rc;
  CSD_CHECK_HIP(hipMemsetAsync(bp, 0, (size_t)p.CoutPad * sizeof(float), s));
  CSD_CHECK_HIP(hipMemcpyAsync(bp, bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.src0 = xh; a.wpack = wp; a.bias = bp; a.out = out;
  a.out_stride = Cout; a.out_nchw = 0; a.out_scale = 1.f;
  return ns ? conv16_launch(p, ns, a, s) : conv_launch(p, a, s);
}

extern "C" int csd_input_conv(const float* x, const float* y, const float* y_noise, float y_sigma, const float* weight, const float* bias,
                              float* out, double* stats, int B, int Cx, int Cy, int Cout, int S, int centered, int precision, int fused,
                              void* scratch, void* stream) {
  return input_conv_impl(x, y, y_noise, y_sigma, weight, bias, out, stats, B, Cx, Cy, Cout, S, centered, precision, fused, scratch, stream, 0);
}

extern "C" int csd_input_conv_kx(const float* x, const float* y, const float* y_noise, float y_sigma, const float* weight,
                                 const float* bias, float* out, double* stats, int B, int Cx, int Cy, int Cout, int S, int y_scale,
                                 int centered, int precision, int fused, void* scratch, void* stream) {
  CSD_REQUIRE(y_scale >= 2, "input_conv_kx: y_scale must be at least 2 (got %d)", y_scale);
  return input_conv_impl(x, y, y_noise, y_sigma, weight, bias, out, stats, B, Cx, Cy, Cout, S, centered, precision, fused, scratch, stream,
                         y_scale);
}

// ---- ResnetBlock convolution with the fused GroupNorm + SiLU prologue (conv_ff.hip) ---------------------------------
extern "C" size_t csd_conv3x3_block_scratch_bytes(int Cin, int Cout) {
  ConvPlan p;
  memset(&p, 0, sizeof(p));
  p.C0 = Cin; p.Cout = Cout;
  // (the shape is not known here: sized for the Winograd pack of conv_xk.hip - 12 instead of 9 fragment sets per 16 channels)
  return scratch_aligned_bytes(convff_packed_bytes(p, 2) / 3 * 4, kScratchPrefetchSlack);
}

extern "C" int csd_conv3x3_block(const float* x0, const float* x1, const float* weight, const float* bias, const float* nscale,
                                 const float* nshift, const float* temb, int temb_stride, const float* res, float out_scale,
                                 float* y, double* stats, int B, int C0, int C1, int Cout, int H, int W, int precision,
                                 void* scratch, void* stream) {
  CSD_REQUIRE(x0 && weight && y && scratch, "conv3x3_block: null argument");
  CSD_REQUIRE(precision == CSD_PREC_F16X3 || precision == CSD_PREC_F16 || precision == CSD_PREC_F16F8,
              "conv3x3_block: precision must be fp16x3, fp16 or fp16f8");
  hipStream_t s = (hipStream_t)stream;
  const int ns = precision == CSD_PREC_F16F8 ? 3 : precision_ns(precision);
  ConvPlan p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.IH = p.OH = H; p.IW = p.OW = W; p.C0 = C0; p.C1 = C1; p.Cout = Cout; p.taps = 9; p.stride = 1; p.pad = 1; p.up = 0;
  CSD_REQUIRE(convff_supported(p, ns), "conv3x3_block: unsupported shape (C %d+%d -> %d, %dx%d)", C0, C1, Cout, H, W);
  int rc = convff_plan_tiles(&p, ns);
  if (rc) return rc;
  void* wpack = scratch_aligned<void>(scratch);
  if ((rc = convff_pack_weight(p, ns, weight, 0, C0 + C1, Cout, 0, wpack, s))) return rc;
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.src0 = x0; a.src1 = x1; a.wpack = static_cast<const float*>(wpack); a.bias = bias; a.temb = temb; a.res = res;
  a.nscale = nscale; a.nshift = nshift; a.out = y; a.temb_stride = temb_stride; a.out_stride = Cout; a.out_coff = 0;
  a.out_nchw = 0; a.act = CSD_ACT_SWISH; a.out_scale = out_scale; a.stats = stats; a.dbg = nullptr;
  return convff_launch(p, ns, a, s);
}

// ---- attention ------------------------------------------------------------------------------------------
// scratch of csd_attention: q | k | v interleaved per pixel, NHWC [B, L, 3C] | the NHWC output
struct AttnScratch { float *qkv, *oh; size_t bytes; };
static AttnScratch attn_scratch(void* base, int B, int C, size_t L) {
  AttnScratch S;
  ScratchCarver c(base);
  S.qkv = c.take<float>((size_t)B * L * 3 * C);
  S.oh = c.take<float>((size_t)B * L * C);
  S.bytes = c.bytes(kScratchSlack);
  return S;
}

extern "C" size_t csd_attention_scratch_bytes(int B, int C, int H, int W) { return attn_scratch(nullptr, B, C, (size_t)H * W).bytes; }

extern "C" int csd_attention(const float* q, const float* k, const float* v, float* out, int B, int C, int H, int W,
                             void* scratch, void* stream) {
  CSD_REQUIRE(q && k && v && out && scratch, "attention: null argument");
  hipStream_t s = (hipStream_t)stream;
  const int L = H * W;
  const AttnScratch S = attn_scratch(scratch, B, C, (size_t)L);
  float *const qkv = S.qkv, *const oh = S.oh;
  int rc;
  if ((rc = nchw_to_nhwc_launch(q, qkv, B, C, L, C, 3 * C, s))) return rc;
  if ((rc = nchw_to_nhwc_launch(k, qkv + C, B, C, L, C, 3 * C, s))) return rc;
  if ((rc = nchw_to_nhwc_launch(v, qkv + 2 * C, B, C, L, C, 3 * C, s))) return rc;
  if ((rc = attention_launch(qkv, 3 * C, oh, B, L, C, s))) return rc;
  return nhwc_to_nchw_launch(oh, out, B, C, L, C, s);
}

// ---- small operators for graphs orchestrated above the C ABI (the NCSN++ adapter) ---------------------------
extern "C" int csd_linear(const float* in, const float* weight, const float* bias, float* out, int B, int K, int N,
                          int act_in, void* stream) {
  CSD_REQUIRE(in && weight && out && B > 0 && K > 0 && N > 0, "linear: bad arguments");
  return linear_launch(in, weight, bias, out, B, K, N, act_in, (hipStream_t)stream);
}

extern "C" int csd_fourier_embedding(const float* t, const float* W, float* out, int B, int E, void* stream) {
  CSD_REQUIRE(t && W && out && B > 0 && E > 0, "fourier_embedding: bad arguments");
  return fourier_embedding_launch(t, W, out, B, E, (hipStream_t)stream);
}

extern "C" int csd_axpby(const float* a, const float* b, float* out, float alpha, float beta, float gamma, float post,
                         int64_t n, void* stream) {
  CSD_REQUIRE(a && out && n > 0, "axpby: bad arguments");
  return axpby_launch(a, b, out, alpha, beta, gamma, post, (size_t)n, (hipStream_t)stream);
}

// csd_unet_config.y_scale's resamplers as operators: the device functions of the network's boundary kernels (common.h: bilin_up,
// bilin_down, bilin_down_adjoint) on n = B * C contiguous planes
extern "C" int csd_bilinear_up(const float* y, float* out, int64_t n, int side, int scale, void* stream) {
  CSD_REQUIRE(y && out && n > 0 && n <= INT32_MAX && side > 0, "bilinear_up: bad arguments");
  const size_t s2 = (size_t)side * side;
  return bilinear_up_launch(y, nullptr, 0.f, s2, out, s2 * scale * scale, (int)n, 1, side, scale, (hipStream_t)stream);
}

extern "C" int csd_bilinear_down(const float* v, float* out, int64_t n, int side, int scale, void* stream) {
  CSD_REQUIRE(v && out && n > 0 && n <= INT32_MAX && side > 0 && scale >= 2, "bilinear_down: bad arguments");
  const size_t s2 = (size_t)side * side;
  return bilinear_down_launch(v, s2, out, s2 / ((size_t)scale * scale), (int)n, 1, side, scale, (hipStream_t)stream);
}

extern "C" int csd_bilinear_down_adjoint(const float* g, float* out, int64_t n, int side, int scale, void* stream) {
  CSD_REQUIRE(g && out && n > 0 && n <= INT32_MAX && side > 0 && scale >= 2, "bilinear_down_adjoint: bad arguments");
  const size_t s2 = (size_t)side * side;
  return bilinear_down_adjoint_launch(g, s2 / ((size_t)scale * scale), out, s2, (int)n, 1, side, scale, (hipStream_t)stream);
}

extern "C" int csd_bias_add_nchw(const float* x, const float* bias, float* out, int B, int C, int64_t inner,
                                 int bias_stride, int act, void* stream) {
  CSD_REQUIRE(x && bias && out && B > 0 && C > 0 && inner > 0, "bias_add_nchw: bad arguments");
  return bias_add_nchw_launch(x, bias, out, B, C, (size_t)inner, bias_stride, act, (hipStream_t)stream);
}
