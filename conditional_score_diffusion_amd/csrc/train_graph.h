// train_graph.h - the training step of BOTH network families (arch 0: DDPM family, arch 1: NCSN++) as ONE planned graph behind the C
// ABI: csd_unet_train_forward / csd_unet_backward.  Included at the end of unet.hip (shares Net /
// Module / Param).  NCSN++ (models/ncsnpp.py:238-388, models/layerspp.py:44-91,212-274): BigGAN blocks with FIR up / down sampling of
// both branches (backward = the transposed FIR: the other direction's geometry with the flipped taps, op/upfirdn2d.py:20-87), the
// Conv_2 shortcut, (x + h) / sqrt(2), AttnBlockpp, Combine 'sum' of the input pyramid, the 'residual' input pyramid (fir_pyramid.hip),
// the output pyramid, Fourier or positional embedding, GroupNorm(min(C / 4, 32)).
//
// What it replaces: torch autograd over models/ddpm.py:149-213 + models/layers.py:524-675 in training mode (run_lib.py:55-73).
// The forward runs the reference's layer sequence on the NHWC operators of this library with nn.Dropout active and keeps
// exactly the tensors a gradient needs in the caller's workspace; the backward walks the recorded steps in reverse and
// writes every parameter gradient straight to the caller's pointers (one per parameter, csd_unet_param_info order) - no
// autograd graph, no per-layer host round trip, no transposed / concatenated weight copies (NIN weights are applied through
// the transposed-weight flag of csd_conv2d_ex, their gradients come from the weight-gradient kernel with swapped operands),
// Conv_0's bias gradient and the time-embedding gradient of a block share one reduction.
//
// Memory: [saved activations (forward, bump)] [gradients + temporaries (backward, bump with per-module release)]; the size
// is found by a dry run of the same code (csd_unet_train_workspace_bytes).
#pragma once

namespace csd {

struct TT { float* p = nullptr; int H = 0, C = 0; float* g = nullptr; };          // tensor [B, H, H, C]: data, gradient
enum TSKind { TS_STEM, TS_RES, TS_ATTN, TS_DOWN, TS_UP, TS_CAT, TS_HEAD, TS_COMBINE, TS_PYR, TS_RPYR };
struct TStep {
  TSKind kind;
  int mod = -1, in0 = -1, in1 = -1, out = -1;      // (TS_RPYR: in0 = the down block's h, in1 = the pyramid source tensor, -1 = the network input)
  // the saved tensors the backward reads; a step sets and reads only the ones its kind has
  float* op0 = nullptr;         // the step's first conv operand: TS_RES act(GroupNorm_0(x)) (FIR-resampled in an up / down block), TS_ATTN
                                // GroupNorm_0(x), TS_HEAD / TS_PYR act(GroupNorm(h)); rs0 / ms0: that GroupNorm's (rstd, -mean * rstd) [B, C]
  float *rs0 = nullptr, *ms0 = nullptr;
  float *c0 = nullptr, *a1 = nullptr, *rs1 = nullptr, *ms1 = nullptr;      // TS_RES: Conv_0(.) + Dense_0 row; dropout(act(GroupNorm_1(c0)))
  float *mask = nullptr, *xr = nullptr;      // TS_RES: the dropout mask (p > 0); the FIR-resampled block input (the shortcut's operand)
  float *qkv = nullptr, *attn = nullptr;     // TS_ATTN: q | k | v [B, H, H, 3C]; the attention core's output (NIN_3's operand)
  float* pyr = nullptr;         // TS_COMBINE: the input pyramid's level (NCHW), Conv_0's operand
  uint64_t drop_id = 0;
  int flag = 0;                 // TS_PYR: PYR_* bits
};
enum {
  PYR_ADDS_COARSER = 1,         // the level adds FIR-up of the coarser level (in1)
  PYR_CALLER_OUT = 2            // the finest level: the forward writes the caller's `out`, the backward reads d_out
};

// what a convolution (TG::conv) or a weight gradient (TG::wgrad) sets beside its operands and extents; a call names what differs
static constexpr int NHWC = CSD_IN_NHWC | CSD_OUT_NHWC;
struct TConv {
  int k = 3, stride = 1;
  int dpad = 0, up2 = 0;        // the Downsample's (0, 1, 0, 1) padding; nearest x2 in front of the convolution
  int layout = NHWC;            // conv: | CSD_WEIGHT_T for a data gradient (wgrad adds CSD_SPLIT_BF16 by the precision)
  const float *res = nullptr, *temb = nullptr;      // conv: NHWC tensor / per-sample [B, Cout] row added in the epilogue
  const void* planes = nullptr; // conv: the operand's fp16 planes (conv2d_operand_planes)
  bool temp = false;            // wgrad: dw is a temporary of the backward, not a parameter slot: stored, also by an accumulating backward
};
static const char* const QKV_W[3] = {"NIN_0.W", "NIN_1.W", "NIN_2.W"};      // the attention block's q, k, v projections
static const char* const QKV_B[3] = {"NIN_0.b", "NIN_1.b", "NIN_2.b"};

struct TrainState {
  bool valid = false;
  int B = 0;
  void* ws = nullptr;
  size_t fwd_top = 0;
  float p_drop = 0.f;
  uint64_t call = 0;            // the forward's call_index: csd_unet_backward must name it
  std::vector<TT> t;
  std::vector<TStep> steps;
  float *xin = nullptr, *emb = nullptr, *temb1 = nullptr, *temb2 = nullptr, *temb2_act = nullptr;
  int lin0 = 0, emb_dim = 0, fourier_mod = -1;      // module index of the embedding MLP's first Linear; width of the embedding; NCSN++ Fourier module
};

// one recorded forward per (network handle, workspace): two forwards of one network may be alive at once (a monitoring forward
// between a training forward and its backward) as long as each has its own workspace - and a backward names the call_index of the
// forward it belongs to, so a workspace that was re-used in between is an error, never a silently wrong gradient
static std::map<std::pair<const Net*, const void*>, TrainState> g_train;
// gradient-ready marks of a handle (csd_unet_backward_marks): event k is recorded on the backward's stream as soon as every gradient
// of the modules with all_modules index >= first_module[k] is final; `epoch` counts the backward calls that recorded all of them
struct GradMarks {
  std::vector<std::pair<int, hipEvent_t>> marks;     // sorted by first_module, descending (the order they become ready)
  uint64_t epoch = 0;
};
static std::map<const Net*, GradMarks> g_marks;
static std::mutex g_train_mu;                         // (the map only; a handle itself is driven by one thread at a time)
static TrainState& train_state_of(const Net* n, const void* ws) {
  std::lock_guard<std::mutex> lk(g_train_mu);
  return g_train[std::make_pair(n, ws)];
}
static TrainState* train_state_find(const Net* n, const void* ws) {
  std::lock_guard<std::mutex> lk(g_train_mu);
  auto it = g_train.find(std::make_pair(n, ws));
  return it == g_train.end() ? nullptr : &it->second;
}
static void train_state_erase_one(const Net* n, const void* ws, const uint64_t* call = nullptr) {
  std::lock_guard<std::mutex> lk(g_train_mu);
  auto it = g_train.find(std::make_pair(n, ws));
  // (a release that names its forward's call index drops the record of THAT forward only: a finalizer that runs late - its context sat
  // in a reference cycle - may find the allocator has handed the same address to a newer forward whose backward is still pending)
  if (it != g_train.end() && (!call || it->second.call == *call)) g_train.erase(it);
}
// records whose forward has been consumed (or failed) and whose workspace is not `keep`: a long run with monitoring forwards in
// private workspaces must not grow the map without bound (each record holds pointers into a workspace that may be gone)
static void train_state_purge_stale(const Net* n, const void* keep) {
  std::lock_guard<std::mutex> lk(g_train_mu);
  for (auto it = g_train.begin(); it != g_train.end();)
    it = (it->first.first == n && it->first.second != keep && !it->second.valid) ? g_train.erase(it) : std::next(it);
}
static void train_state_erase(const Net* n) {
  std::lock_guard<std::mutex> lk(g_train_mu);
  for (auto it = g_train.begin(); it != g_train.end();) it = it->first.first == n ? g_train.erase(it) : std::next(it);
  g_marks.erase(n);
}

__global__ void concat_c_kernel(const float4* __restrict__ a, int ca4, const float4* __restrict__ b, int cb4,
                                float4* __restrict__ out, size_t npix) {
  const int c4 = ca4 + cb4;
  const size_t n = npix * c4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t px = i / c4;
    const int c = (int)(i - px * c4);
    out[i] = c < ca4 ? a[px * ca4 + c] : b[px * cb4 + (c - ca4)];
  }
}

__global__ void split_c_kernel(const float4* __restrict__ in, int ca4, int cb4, float4* __restrict__ a,
                               float4* __restrict__ b, size_t npix) {
  const int c4 = ca4 + cb4;
  const size_t n = npix * c4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t px = i / c4;
    const int c = (int)(i - px * c4);
    const float4 v = in[i];
    if (c < ca4) a[px * ca4 + c] = v; else b[px * cb4 + (c - ca4)] = v;
  }
}

// rows of `width` floats: dst[r*dpitch + j] (=|+=) src[r*spitch + j]   (q|k|v weight concatenation and its inverse; beta = 1: the
// accumulating backward's scatter of the concatenated gradient into the three parameter slots)
__global__ void copy2d_kernel(const float* __restrict__ src, int spitch, float* __restrict__ dst, int dpitch, int width, int rows, int beta) {
  const size_t n = (size_t)width * rows;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / width;
    const int j = (int)(i - r * width);
    const float v = src[r * spitch + j];
    dst[r * dpitch + j] = beta ? dst[r * dpitch + j] + v : v;
  }
}

// rows of `width` floats, scaled: dst[r*dpitch + j] = scale * src[r*spitch + j]   (the x-channel slice of an input-layer weight for the
// data gradient of the network input; scale 2 = the 2x - 1 input map of non-centred data)
__global__ void wslice_kernel(const float* __restrict__ src, int spitch, float* __restrict__ dst, int dpitch, int width, int rows, float scale) {
  const size_t n = (size_t)width * rows;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / width;
    const int j = (int)(i - r * width);
    dst[r * dpitch + j] = scale * src[r * spitch + j];
  }
}

struct TG {
  Net& n;
  TrainState& st;
  int B;
  hipStream_t s;
  bool dry;
  const float* const* P;
  float* const* G;
  float* base;
  size_t top = 0, peak = 0;
  int prec, act;
  float p_drop = 0.f;
  uint64_t seed = 0, call = 0;
  int drop_count = 0;
  GradMarks* gm = nullptr;      // backward only
  size_t gm_next = 0;
  bool pg = true;               // backward: parameter gradients wanted (false: csd_unet_backward_ex with grads == NULL)
  int gacc = 0;                 // backward: 1 = every parameter slot G[i] += its gradient (csd_unet_backward_acc), 0 = G[i] = its gradient
  bool want_dx = false;         // backward: d loss / d x wanted (d_x = the caller's [B, x_channels, S, S] NCHW buffer)
  float* d_x = nullptr;
  float* dpyr = nullptr;        // NCSN++ input pyramid: x-channel gradient [B, cx, side, side] NCHW of the finest level combined so far
  float* dres0 = nullptr;       // NCSN++ 'residual' pyramid: its level-0 convolution's x-channel data gradient [B, cx, S, S] NCHW (stem_dx adds it)
  // every gradient of the modules with index >= `from` has been enqueued: record the marks that this completes
  int marks_reached(int from) {
    if (!gm || dry) return CSD_OK;
    while (gm_next < gm->marks.size() && gm->marks[gm_next].first >= from) {
      CSD_CHECK_HIP(hipEventRecord(gm->marks[gm_next].second, s));
      ++gm_next;
    }
    return CSD_OK;
  }

  TG(Net& net, TrainState& state, int B_, hipStream_t s_, bool dry_, const float* const* P_, float* const* G_, float* ws)
      : n(net), st(state), B(B_), s(s_), dry(dry_), P(P_), G(G_), base(ws), prec(net.cfg.precision), act(net.cfg.act) {}

  float* alloc(size_t nfl) {
    nfl = (nfl + 63) / 64 * 64;
    float* p = base + top;
    top += nfl;
    peak = std::max(peak, top);
    return p;
  }
  float* alloc_bytes(size_t bytes) { return alloc((bytes + 3) / 4); }
  int G_of(int C) const { return n.cfg.arch == 1 ? std::min(C / 4, 32) : 32; }      // GroupNorm groups (layerspp.py:67,219,231)
  float skip_scale() const { return (n.cfg.arch == 1 && n.cfg.skip_rescale) ? 0.70710678118654752440f : 1.f; }
  size_t act_n(int H, int C) const { return (size_t)B * H * H * C; }
  const float* W(int mod, const char* sub) const { const int i = n.P(mname(mod, sub)); return (dry || i < 0) ? nullptr : P[i]; }
  // (G == NULL: csd_unet_backward_ex without parameter gradients - every consumer of DW() is skipped then, but its arguments are evaluated)
  float* DW(int mod, const char* sub) const { const int i = n.P(mname(mod, sub)); return (dry || i < 0 || !G) ? nullptr : G[i]; }

#define TG_RUN(expr)                       \
  do {                                     \
    if (!dry) {                            \
      const int _rc = (expr);              \
      if (_rc) return _rc;                 \
    }                                      \
  } while (0)

  // ---- operator wrappers (scratch is a temporary above `top`) ---------------------------------------------------------
  int conv(const float* x, const float* w, const float* b, float* y, int Cin, int Cout, int H, const TConv& a = {}) {
    const size_t m = top;
    float* sc = alloc_bytes(csd_conv_scratch_bytes(B, Cin, Cout, H, H, a.k, a.up2));
    TG_RUN(conv2d_impl(x, w, b, a.res, a.temb, y, B, Cin, Cout, H, H, a.k, a.stride, a.dpad, a.up2, prec, a.layout, sc, s, a.planes));
    top = m;
    return CSD_OK;
  }
  int wgrad(const float* x, const float* dy, float* dw, int Cin, int Cout, int H, const TConv& a = {}) {
    if (!pg) return CSD_OK;
    const size_t m = top;
    float* sc = alloc_bytes(csd_conv_wgrad_scratch_bytes(B, Cin, Cout, H, H, a.k, a.stride, a.up2));
    TG_RUN(conv2d_wgrad_beta(x, dy, dw, B, Cin, Cout, H, H, a.k, a.stride, a.dpad, a.up2,
                             a.layout | (prec == CSD_PREC_F32 ? 0 : CSD_SPLIT_BF16), sc, s, a.temp ? 0 : gacc));
    top = m;
    return CSD_OK;
  }
  // (mask != null: nn.Dropout of the activated tensor in the same pass; the mask csd_dropout would draw for (seed, drop_id))
  // (planes != null: the fp16 operand planes of y for the conv that follows, written by the same pass - conv2d_operand_planes())
  int gn(const float* x, const float* gamma, const float* beta, float* y, float* rs, float* ms, int C, int H, int a, float* mask = nullptr,
         uint64_t drop_id = 0, void* planes = nullptr, int plane_count = 0) {
    const size_t m = top;
    float* sc = alloc_bytes(csd_groupnorm_nhwc_scratch_bytes(B, C, H * H));
    TG_RUN(groupnorm_act_dropout_nhwc(x, gamma, beta, y, rs, ms, mask, p_drop, seed, drop_id, B, C, H * H, G_of(C), 1e-6f, a, sc, s, planes,
                                      plane_count));
    top = m;
    return CSD_OK;
  }
  // dx, dgamma / dbeta written to their parameter slots
  int gn_bwd(const float* x, const float* gamma, const float* beta, const float* rs, const float* ms, const float* dy, float* dx,
             float* dgamma, float* dbeta, int C, int H, int a, const float* add = nullptr) {
    const size_t m = top;
    float* grow = alloc((size_t)B * C);
    float* brow = alloc((size_t)B * C);
    float* sc = alloc_bytes(csd_groupnorm_nhwc_scratch_bytes(B, C, H * H));
    TG_RUN(groupnorm_act_backward_nhwc_add(x, gamma, beta, rs, ms, dy, add, dx, grow, brow, C, B, C, H * H, G_of(C), a, sc, s));
    if (pg) TG_RUN(sum_rows2(grow, dgamma, brow, dbeta, B, C, s, gacc));
    top = m;
    return CSD_OK;
  }
  int copy(const float* src, float* dst, size_t nfl) {
    CSD_CHECK_HIP(hipMemcpyAsync(dst, src, nfl * sizeof(float), hipMemcpyDeviceToDevice, s));
    return CSD_OK;
  }
  // out[b, c] = sum over pixels of dy [B, H*H, C]
  int sum_pixels(const float* dy, float* out, int C, int H) {
    const size_t m = top;
    float* sc = alloc_bytes(csd_sum_pixels_scratch_bytes(B, H * H, C));
    TG_RUN(csd_sum_pixels_nhwc(dy, out, B, H * H, C, sc, s));
    top = m;
    return CSD_OK;
  }
  // conv bias: batch + pixel sum of an NHWC gradient (temp: db is a temporary of the backward, as TConv::temp)
  int bias_grad(const float* dy, float* db, int C, int H, bool temp = false) {
    if (!pg) return CSD_OK;
    const size_t m = top;
    float* bc = alloc((size_t)B * C);
    int rc = sum_pixels(dy, bc, C, H);
    if (rc) return rc;
    TG_RUN(sum_rows_beta(bc, db, B, C, temp ? 0 : gacc, s));
    top = m;
    return CSD_OK;
  }
  int add_into(float* dst, const float* src, size_t nfl) { TG_RUN(csd_axpby(dst, src, dst, 1.f, 1.f, 0.f, 1.f, (int64_t)nfl, s)); return CSD_OK; }
  // FIR resampling by 2 of [Bn, H, H, C] (upsample_2d / downsample_2d, up_or_down_sampling.py:196-257).  adjoint: the gradient of
  // the OTHER direction's forward = this geometry with the flipped taps and the other gain (op/upfirdn2d.py:20-87: up and down
  // swapped, kernel flipped, pads g_pad): d upsample = down geometry x 4, d downsample = up geometry / 4.
  int fir(const float* x, float* y, int Bn, int H, int C, bool up_geometry, bool adjoint) {
    TG_RUN(fir_resample_nhwc_launch(x, y, Bn, H, H, C, n.cfg.fir_kernel, up_geometry ? 1 : 0, s,
                                    adjoint ? (up_geometry ? 0.25f : 4.f) : 1.f, adjoint ? 1 : 0));
    return CSD_OK;
  }
  int scale_into(const float* src, float* dst, float f, size_t nfl) { TG_RUN(csd_axpby(src, nullptr, dst, f, 0.f, 0.f, 1.f, (int64_t)nfl, s)); return CSD_OK; }
  int launch_blocks(size_t n) const { return (int)std::min<size_t>((n + 255) / 256, 256 * 16); }

  // gradient routing: the first contribution becomes the tensor's gradient buffer, later ones are added
  int contribute(int tid, float* g) {
    TT& t = st.t[tid];
    if (!t.g) { t.g = g; return CSD_OK; }
    return add_into(t.g, g, act_n(t.H, t.C));
  }
  int new_tensor(int H, int C, bool allocate = true) {
    TT t;
    t.H = H; t.C = C;
    if (allocate) t.p = alloc(act_n(H, C));
    st.t.push_back(t);
    return (int)st.t.size() - 1;
  }

  // the 'residual' pyramid's source: level 0 = the NCHW network input st.xin, later levels = the previous combined h (NHWC)
  struct PyrSrc { const float* p; int64_t sb; int sp; int64_t sc; };
  PyrSrc pyr_src(int tid, int H, int C) const {
    if (tid < 0) return PyrSrc{st.xin, (int64_t)C * H * H, 1, (int64_t)H * H};
    return PyrSrc{st.t[tid].p, (int64_t)H * H * C, C, 1};
  }
  const float* pyr_taps() const { return n.cfg.progressive_input == 2 ? n.cfg.fir_kernel : nullptr; }

  // =====================================================================================================================
  // forward (models/ddpm.py:149-213 with model.train())
  // =====================================================================================================================
  // The residual block of both families is one block: ResnetBlockDDPM (models/layers.py:632-675) is ResnetBlockBigGANpp
  // (models/layerspp.py:242-274) with no resampling, the NIN shortcut and scale 1.  What differs, from the module and the config:
  struct ResForm {
    bool up = false, down = false;                   // FIR resampling of both branches in front of Conv_0 / the shortcut
    // the 1x1 shortcut on the (resampled) block input; sc_w == null: the identity.  NIN_0.W is [cin, cout]: applied through the
    // transposed-weight flag, its data gradient is the plain OIHW conv of dout (W read as [O = cin, I = cout]) and its weight gradient
    // dW[i, o] = sum_p x[p, i] dout[p, o] the 1x1 weight gradient with the operands swapped.  Conv_2.weight is OIHW.
    const char *sc_w = nullptr, *sc_b = nullptr;
    int sc_layout = NHWC, sc_dgrad_layout = NHWC;
    bool sc_swap = false;
    float scale = 1.f;                               // out = (shortcut + h) * scale
    bool dense = false;                              // Dense_0(act(temb)) rides in Conv_0's epilogue (time-conditional networks)
    bool resample() const { return up || down; }
    int out_side(int H) const { return up ? 2 * H : (down ? H / 2 : H); }
  };
  ResForm res_form(const Module& m) const {
    ResForm f;
    f.up = m.up != 0; f.down = m.down != 0;
    f.scale = skip_scale();
    f.dense = n.cfg.conditional != 0;
    if (m.cin == m.cout && !f.resample()) return f;
    if (n.cfg.arch == 1) { f.sc_w = "Conv_2.weight"; f.sc_b = "Conv_2.bias"; f.sc_dgrad_layout = NHWC | CSD_WEIGHT_T; }
    else { f.sc_w = "NIN_0.W"; f.sc_b = "NIN_0.b"; f.sc_layout = NHWC | CSD_WEIGHT_T; f.sc_swap = true; }
    return f;
  }

  // h = act(GroupNorm_0(x)); up / down: h, x = FIR(h), FIR(x); h = Conv_0(h) + Dense_0(act(temb)); h = Conv_1(dropout(act(GroupNorm_1(h))));
  // x = shortcut(x) if the shape changes; (x + h) * scale
  int res_fwd(const Module& m, int in, int* out_tid) {
    const ResForm f = res_form(m);
    const int H = st.t[in].H, cin = m.cin, cout = m.cout, Ho = f.out_side(H);
    const float* h = st.t[in].p;
    TStep sp;
    sp.kind = TS_RES; sp.mod = m.idx; sp.in0 = in;
    // persistent tensors first (the backward reads them), temporaries - the convs' operand planes, the shortcut - above them
    float* a0 = sp.op0 = alloc(act_n(H, cin));       // act(GroupNorm_0(x))
    sp.rs0 = alloc((size_t)B * cin); sp.ms0 = alloc((size_t)B * cin);
    if (f.resample()) { sp.op0 = alloc(act_n(Ho, cin)); sp.xr = alloc(act_n(Ho, cin)); }
    sp.c0 = alloc(act_n(Ho, cout));
    sp.a1 = alloc(act_n(Ho, cout));
    sp.rs1 = alloc((size_t)B * cout); sp.ms1 = alloc((size_t)B * cout);
    ++drop_count;
    sp.drop_id = (call << 16) + (uint64_t)drop_count;
    if (p_drop > 0.f) sp.mask = alloc(act_n(Ho, cout));
    sp.out = new_tensor(Ho, cout);
    float* o = st.t[sp.out].p;
    const float* xs = f.resample() ? sp.xr : h;      // the shortcut's operand
    int rc;
    {
      const size_t mk = top;
      // the GroupNorm's apply pass also writes the fp16 operand planes Conv_0 would otherwise split a0 into in a pass of its own
      const int np0 = f.resample() ? 0 : conv2d_operand_planes(B, cin, cout, H, H, 3, 1, 0, 0, prec);
      float* pl0 = np0 ? alloc_bytes((size_t)np0 * B * H * H * cin * 2) : nullptr;
      rc = gn(h, W(m.idx, "GroupNorm_0.weight"), W(m.idx, "GroupNorm_0.bias"), a0, sp.rs0, sp.ms0, cin, H, act, nullptr, 0, pl0, np0);
      if (rc) return rc;
      if (f.resample()) {
        rc = fir(a0, sp.op0, B, H, cin, f.up, false); if (rc) return rc;
        rc = fir(h, sp.xr, B, H, cin, f.up, false); if (rc) return rc;
      }
      float* d = nullptr;
      if (f.dense) {                                 // the time-embedding row rides in Conv_0's epilogue
        d = alloc((size_t)B * cout);
        // (act(temb) is computed once per forward: every block's Dense_0 used to redo it inside its own latency-bound launch)
        TG_RUN(csd_linear(st.temb2_act, W(m.idx, "Dense_0.weight"), W(m.idx, "Dense_0.bias"), d, B, 4 * n.cfg.nf, cout, CSD_ACT_NONE, s));
      }
      rc = conv(sp.op0, W(m.idx, "Conv_0.weight"), W(m.idx, "Conv_0.bias"), sp.c0, cin, cout, Ho, {.temb = d, .planes = pl0});
      if (rc) return rc;
      top = mk;
    }
    {
      const size_t mk = top;
      const int np1 = conv2d_operand_planes(B, cout, cout, Ho, Ho, 3, 1, 0, 0, prec);
      float* pl1 = np1 ? alloc_bytes((size_t)np1 * B * Ho * Ho * cout * 2) : nullptr;
      rc = gn(sp.c0, W(m.idx, "GroupNorm_1.weight"), W(m.idx, "GroupNorm_1.bias"), sp.a1, sp.rs1, sp.ms1, cout, Ho, act, sp.mask, sp.drop_id,
              pl1, np1);                             // (dropout in the apply pass)
      if (rc) return rc;
      const float* shortcut = h;
      if (f.sc_w) {
        float* sc = alloc(act_n(Ho, cout));
        rc = conv(xs, W(m.idx, f.sc_w), W(m.idx, f.sc_b), sc, cin, cout, Ho, {.k = 1, .layout = f.sc_layout});
        if (rc) return rc;
        shortcut = sc;
      }
      rc = conv(sp.a1, W(m.idx, "Conv_1.weight"), W(m.idx, "Conv_1.bias"), o, cout, cout, Ho, {.res = shortcut, .planes = pl1});   // + shortcut in the epilogue
      if (rc) return rc;
      if (f.scale != 1.f) { rc = scale_into(o, o, f.scale, act_n(Ho, cout)); if (rc) return rc; }
      top = mk;
    }
    st.steps.push_back(sp);
    *out_tid = sp.out;
    return CSD_OK;
  }

  // the q | k | v weight of ONE contraction, [NIN_0.W | NIN_1.W | NIN_2.W] ([C, 3C]) into wc, and (bc != null) its bias [3C] into bc
  int qkv_weight(int mod, int C, float* wc, float* bc) {
    for (int j = 0; j < 3 && !dry; ++j) {
      hipLaunchKernelGGL(copy2d_kernel, dim3(launch_blocks((size_t)C * C)), dim3(256), 0, s, W(mod, QKV_W[j]), C, wc + j * C, 3 * C, C, C, 0);
      CSD_LAUNCH_CHECK();
      if (bc) TG_RUN(copy(W(mod, QKV_B[j]), bc + j * C, C));
    }
    return CSD_OK;
  }

  int attn_fwd(const Module& m, int in, int* out_tid) {
    const int H = st.t[in].H, C = m.cin;
    const float* h = st.t[in].p;
    TStep sp;
    sp.kind = TS_ATTN; sp.mod = m.idx; sp.in0 = in;
    sp.op0 = alloc(act_n(H, C));
    sp.rs0 = alloc((size_t)B * C); sp.ms0 = alloc((size_t)B * C);
    int rc = gn(h, W(m.idx, "GroupNorm_0.weight"), W(m.idx, "GroupNorm_0.bias"), sp.op0, sp.rs0, sp.ms0, C, H, CSD_ACT_NONE);
    if (rc) return rc;
    sp.qkv = alloc(act_n(H, 3 * C));
    {
      const size_t mk = top;
      float* wc = alloc((size_t)C * 3 * C);
      float* bc = alloc(3 * C);
      rc = qkv_weight(m.idx, C, wc, bc); if (rc) return rc;
      rc = conv(sp.op0, wc, bc, sp.qkv, C, 3 * C, H, {.k = 1, .layout = NHWC | CSD_WEIGHT_T});
      if (rc) return rc;
      top = mk;
    }
    sp.attn = alloc(act_n(H, C));
    TG_RUN(csd_attention_nhwc_prec(sp.qkv, sp.attn, B, H * H, C, prec, s));      // (the arithmetic of the mode, as csd_unet_forward)
    sp.out = new_tensor(H, C);
    float* o = st.t[sp.out].p;
    rc = conv(sp.attn, W(m.idx, "NIN_3.W"), W(m.idx, "NIN_3.b"), o, C, C, H, {.k = 1, .layout = NHWC | CSD_WEIGHT_T, .res = h});      // + h in the epilogue
    if (rc) return rc;
    if (skip_scale() != 1.f) { rc = scale_into(o, o, skip_scale(), act_n(H, C)); if (rc) return rc; }      // AttnBlockpp: (x + h) / sqrt(2)
    st.steps.push_back(sp);
    *out_tid = sp.out;
    return CSD_OK;
  }

  int cat_fwd(int a, int b, int* out_tid) {
    const int H = st.t[a].H, Ca = st.t[a].C, Cb = st.t[b].C;
    const int out = new_tensor(H, Ca + Cb);
    if (!dry) {
      const size_t npix = (size_t)B * H * H;
      hipLaunchKernelGGL(concat_c_kernel, dim3(launch_blocks(npix * (Ca + Cb) / 4)), dim3(256), 0, s,
                         reinterpret_cast<const float4*>(st.t[a].p), Ca / 4, reinterpret_cast<const float4*>(st.t[b].p), Cb / 4,
                         reinterpret_cast<float4*>(st.t[out].p), npix);
      CSD_LAUNCH_CHECK();
    }
    TStep sp;
    sp.kind = TS_CAT; sp.in0 = a; sp.in1 = b; sp.out = out;
    st.steps.push_back(sp);
    *out_tid = out;
    return CSD_OK;
  }

  // act(GroupNorm(h)) + conv, NHWC in, NCHW out: the head (pyr == null) or one level of the NCSN++ output pyramid - pyramid =
  // Conv(act(GroupNorm(h))) + pyramid_upsample(pyramid) (ncsnpp.py:340-352; *pyr: tensor id of the coarser level, NCHW data; level 0 writes `out`)
  int out_fwd(const Module& mg, int h, float* out, int* pyr) {
    const Module& mc = n.mods[mg.idx + 1];
    const int H = st.t[h].H, C = mg.cin, co = n.cfg.out_channels;
    TStep sp;
    sp.kind = pyr ? TS_PYR : TS_HEAD; sp.mod = mg.idx; sp.in0 = h;
    sp.op0 = alloc(act_n(H, C));
    sp.rs0 = alloc((size_t)B * C); sp.ms0 = alloc((size_t)B * C);
    int rc = gn(st.t[h].p, W(mg.idx, "weight"), W(mg.idx, "bias"), sp.op0, sp.rs0, sp.ms0, C, H, act); if (rc) return rc;
    if (pyr) {
      sp.out = new_tensor(H, co, false);
      st.t[sp.out].p = out = mg.level == 0 ? out : alloc((size_t)B * co * H * H);
      sp.in1 = *pyr;
      sp.flag = (*pyr >= 0 ? PYR_ADDS_COARSER : 0) | (mg.level == 0 ? PYR_CALLER_OUT : 0);
    }
    rc = conv(sp.op0, W(mc.idx, "weight"), W(mc.idx, "bias"), out, C, co, H, {.layout = CSD_IN_NHWC}); if (rc) return rc;      // NCHW out
    if (pyr && *pyr >= 0) {
      const size_t mk = top;
      float* up = alloc((size_t)B * co * H * H);
      rc = fir(st.t[*pyr].p, up, B * co, H / 2, 1, true, false); if (rc) return rc;
      rc = add_into(out, up, (size_t)B * co * H * H); if (rc) return rc;
      top = mk;
    }
    st.steps.push_back(sp);
    if (pyr) *pyr = sp.out;
    return CSD_OK;
  }

  // one walk over Net::mods for both families (models/ddpm.py:149-213, models/ncsnpp.py:238-388 with model.train())
  int forward(const float* x, const float* y, const float* labels, float* out) {
    const csd_unet_config& c = n.cfg;
    const bool pp = c.arch == 1;
    const int S = c.image_size, cx = c.x_channels, cy = c.y_channels, cio = cx + cy, nf = c.nf;
    st.t.clear(); st.steps.clear();
    drop_count = 0;
    st.lin0 = 0; st.emb_dim = nf; st.fourier_mod = -1;
    // network input: cat(x, y) NCHW (models/ddpm.py:275-298 wrappers), 2h - 1 for data in [0, 1] (:163-168; ncsnpp.py:266-268)
    const size_t hw = (size_t)S * S;
    st.xin = alloc((size_t)B * cio * hw);
    // x_squeeze: x, out (and d_out, d_x of the backward) are images at the C ABI; the graph itself runs on the squeezed NCHW tensors, so
    // the copy of x into the network input gathers, and the head writes a workspace tensor that is scattered into the caller's `out`
    // y_scale = K: y arrives at S / K and is upsampled into the network input (bilin_up); the head writes a workspace tensor whose y
    // channels are downsampled into the caller's `out` (the x block is copied) - the layouts of include/csd.h
    const bool sq = c.x_squeeze != 0, ys = c.y_scale != 0;
    float* const out_caller = out;
    if (sq || ys) out = alloc((size_t)B * c.out_channels * hw);
    if (!dry) {
      if (sq) TG_RUN(sq_gather_launch(x, cx * hw, st.xin, cio * hw, B, cx, S, s));
      else CSD_CHECK_HIP(hipMemcpy2DAsync(st.xin, cio * hw * 4, x, cx * hw * 4, cx * hw * 4, B, hipMemcpyDeviceToDevice, s));
      if (ys) TG_RUN(bilinear_up_launch(y, nullptr, 0.f, cy * (hw / ((size_t)c.y_scale * c.y_scale)), st.xin + cx * hw, cio * hw, B, cy,
                                        S / c.y_scale, c.y_scale, s));
      else if (cy) CSD_CHECK_HIP(hipMemcpy2DAsync(st.xin + cx * hw, cio * hw * 4, y, cy * hw * 4, cy * hw * 4, B, hipMemcpyDeviceToDevice, s));
      if (!c.centered) TG_RUN(csd_axpby(st.xin, nullptr, st.xin, 2.f, 0.f, -1.f, 1.f, (int64_t)((size_t)B * cio * hw), s));
    }
    std::vector<int> hs;                             // skip stack (tensor ids)
    int h = -1;                                      // the current tensor
    const float* pyr_in = st.xin;                    // input pyramid (NCHW = [B * cio] single-channel images for the FIR pass)
    int pyr_side = S;
    int pyr_tid = -1;                                // 'residual': the pyramid source tensor (-1: the network input st.xin)
    int pyr = -1;                                    // output pyramid: tensor id of the previous (coarser) level, NCHW data
    for (const Module& m : n.mods) {
      int rc = CSD_OK;
      switch (m.role) {
        case R_EMB_FOURIER:                          // Gaussian Fourier features of the label (layerspp.py:32-41; W is a fixed buffer)
          st.fourier_mod = m.idx;
          st.emb_dim = 2 * nf;
          st.emb = alloc((size_t)B * 2 * nf);
          TG_RUN(csd_fourier_embedding(labels, W(m.idx, "W"), st.emb, B, nf, s));
          break;
        case R_EMB_LINEAR0:                          // (timestep embedding +) 2-layer MLP (models/ddpm.py:153-160)
          st.lin0 = m.idx;
          if (st.fourier_mod < 0) {
            st.emb = alloc((size_t)B * nf);
            TG_RUN(csd_timestep_embedding(labels, st.emb, B, nf, s));
          }
          st.temb1 = alloc((size_t)B * 4 * nf); st.temb2 = alloc((size_t)B * 4 * nf);
          TG_RUN(csd_linear(st.emb, W(m.idx, "weight"), W(m.idx, "bias"), st.temb1, B, st.emb_dim, 4 * nf, CSD_ACT_NONE, s));
          break;
        case R_EMB_LINEAR1:
          TG_RUN(csd_linear(st.temb1, W(m.idx, "weight"), W(m.idx, "bias"), st.temb2, B, 4 * nf, 4 * nf, act, s));
          st.temb2_act = alloc((size_t)B * 4 * nf);
          TG_RUN(csd_act(st.temb2, nullptr, st.temb2_act, act, (int64_t)B * 4 * nf, s));
          break;
        case R_STEM: {                               // NCHW in, NHWC out
          h = new_tensor(S, nf);
          rc = conv(st.xin, W(m.idx, "weight"), W(m.idx, "bias"), st.t[h].p, cio, nf, S, {.layout = CSD_OUT_NHWC});
          if (rc) return rc;
          TStep sp;
          sp.kind = TS_STEM; sp.mod = m.idx; sp.out = h;
          st.steps.push_back(sp);
          break;
        }
        case R_UP_BLOCK:
          rc = cat_fwd(h, hs.back(), &h); if (rc) return rc;
          hs.pop_back();
          [[fallthrough]];
        case R_DOWN_BLOCK: case R_MID_RES_IN: case R_MID_RES_OUT:
          rc = res_fwd(m, h, &h);
          break;
        case R_ATTN: case R_MID_ATTN:
          rc = attn_fwd(m, h, &h);
          break;
        case R_DOWNSAMPLE: case R_UPSAMPLE: {
          if (pp) { rc = res_fwd(m, h, &h); break; }      // the BigGAN down / up block
          // Downsample: pad (0,1,0,1) + stride-2 conv (models/layers.py:619-625); Upsample: nearest x2 + conv (:600-604)
          const bool down = m.role == R_DOWNSAMPLE;
          const int H = st.t[h].H, C = m.cin;
          const int o = new_tensor(m.out_side, C);
          rc = conv(st.t[h].p, W(m.idx, "Conv_0.weight"), W(m.idx, "Conv_0.bias"), st.t[o].p, C, C, H,
                    down ? TConv{.stride = 2, .dpad = 1} : TConv{.up2 = 1});
          if (rc) return rc;
          TStep sp;
          sp.kind = down ? TS_DOWN : TS_UP; sp.mod = m.idx; sp.in0 = h; sp.out = o;
          st.steps.push_back(sp);
          h = o;
          break;
        }
        case R_COMBINE: {                            // pyramid_downsample + Combine 'sum': Conv_0(pyramid) + h (layerspp.py:44-59)
          const int side = st.t[h].H, C = m.cout;
          float* pn = alloc((size_t)B * cio * side * side);
          rc = fir(pyr_in, pn, B * cio, pyr_side, 1, false, false); if (rc) return rc;
          pyr_in = pn; pyr_side = side;
          const int o = new_tensor(side, C);
          rc = conv(pn, W(m.idx, "Conv_0.weight"), W(m.idx, "Conv_0.bias"), st.t[o].p, cio, C, side, {.k = 1, .layout = CSD_OUT_NHWC}); if (rc) return rc;
          rc = add_into(st.t[o].p, st.t[h].p, act_n(side, C)); if (rc) return rc;
          TStep sp;
          sp.kind = TS_COMBINE; sp.mod = m.idx; sp.in0 = h; sp.out = o; sp.pyr = pn;
          st.steps.push_back(sp);
          h = o;
          break;
        }
        case R_PYR_DOWN: {                           // 'residual' (ncsnpp.py:300-307): h = (Downsample(pyramid) + h) * skip scale; pyramid = h
          const int side = st.t[h].H, C = m.cout;
          const int o = new_tensor(side, C);
          {
            const size_t mk = top;
            float* gf = alloc((size_t)36 * m.cin * C);
            const PyrSrc ps = pyr_src(pyr_tid, 2 * side, m.cin);
            TG_RUN(fir_pyr_fold_launch(W(m.idx, pyr_sub(c, false)), m.cin, C, pyr_taps(), gf, nullptr, s));
            TG_RUN(fir_pyr_conv_launch(ps.p, ps.sb, ps.sp, ps.sc, B, 2 * side, m.cin, gf, W(m.idx, pyr_sub(c, true)), st.t[h].p, st.t[o].p, C,
                                       c.progressive_input == 2, skip_scale(), s));
            top = mk;
          }
          TStep sp;
          sp.kind = TS_RPYR; sp.mod = m.idx; sp.in0 = h; sp.in1 = pyr_tid; sp.out = o;
          st.steps.push_back(sp);
          h = pyr_tid = o;
          break;
        }
        case R_PYR_GN:
          rc = out_fwd(m, h, out, &pyr);
          break;
        case R_HEAD_GN:
          rc = out_fwd(m, h, out, nullptr);
          break;
        case R_PYR_CONV: case R_HEAD_CONV:
          break;                                     // (with its GroupNorm)
      }
      if (rc) return rc;
      if (m.push) hs.push_back(h);
    }
    CSD_REQUIRE(hs.empty(), "train_forward: the skip stack is not empty behind the last module");
    if (sq && !dry) {
      const size_t ld = (size_t)c.out_channels * hw;
      TG_RUN(sq_scatter_launch(out, ld, out_caller, ld, B, cx, S, s));
      if (c.out_channels > cx)
        CSD_CHECK_HIP(hipMemcpy2DAsync(out_caller + cx * hw, ld * 4, out + cx * hw, ld * 4, (c.out_channels - cx) * hw * 4, B,
                                       hipMemcpyDeviceToDevice, s));
    }
    if (ys && !dry) {
      const size_t ld = (size_t)c.out_channels * hw, ldo = out_sample_elems(c);
      CSD_CHECK_HIP(hipMemcpy2DAsync(out_caller, ldo * 4, out, ld * 4, cx * hw * 4, B, hipMemcpyDeviceToDevice, s));
      if (c.out_channels > cx)
        TG_RUN(bilinear_down_launch(out + cx * hw, ld, out_caller + cx * hw, ldo, B, c.out_channels - cx, S, c.y_scale, s));
    }
    st.fwd_top = top;
    return CSD_OK;
  }

  // =====================================================================================================================
  // backward
  // =====================================================================================================================
  // Linear y = act_in(x) W^T + b with x [B, K], W [N, K]: dW, db from dy; dact (gradient w.r.t. act_in(x)) is ADDED to dact_acc
  int linear_bwd(const float* x, int act_in, const float* w, const float* dy, float* dw, float* db, float* dact_acc, int K, int N) {
    const size_t m = top;
    const float* a = x;
    if (act_in != CSD_ACT_NONE) {
      float* ax = alloc((size_t)B * K);
      TG_RUN(csd_act(x, nullptr, ax, act_in, (int64_t)B * K, s));
      a = ax;
    }
    TG_RUN(bgemm_beta(dy, a, dw, N, K, B, 1, N, K, 1, K, 1, 1.f, gacc, s));              // dW[n,k] (=|+=) sum_b dy[b,n] a[b,k]
    TG_RUN(sum_rows_beta(dy, db, B, N, gacc, s));
    if (dact_acc) {
      float* da = alloc((size_t)B * K);
      TG_RUN(csd_bgemm(dy, w, da, B, K, N, N, 1, K, 1, K, 1, 1, 0, 0, 0, 1.f, s));       // da[b,k] = sum_n dy[b,n] W[n,k]
      int rc = add_into(dact_acc, da, (size_t)B * K);
      if (rc) return rc;
    }
    top = m;
    return CSD_OK;
  }

  int res_bwd(const TStep& sp, float* dtemb_act) {
    const Module& m = n.mods[sp.mod];
    const ResForm f = res_form(m);
    const TT& tin = st.t[sp.in0];
    const int H = tin.H, cin = m.cin, cout = m.cout, Ho = f.out_side(H);
    const float* h = tin.p;
    const float* xs = f.resample() ? sp.xr : h;      // the shortcut's operand
    float* dh = alloc(act_n(H, cin));                // gradient w.r.t. the block input (kept until its producer has consumed it)
    const size_t mk = top;
    int rc;
    float* dout = st.t[sp.out].g;
    if (f.scale != 1.f) {                            // out = (x + h) / sqrt(2)
      float* ds = alloc(act_n(Ho, cout));
      rc = scale_into(dout, ds, f.scale, act_n(Ho, cout)); if (rc) return rc;
      dout = ds;
    }
    // Conv_1
    rc = wgrad(sp.a1, dout, DW(m.idx, "Conv_1.weight"), cout, cout, Ho); if (rc) return rc;
    rc = bias_grad(dout, DW(m.idx, "Conv_1.bias"), cout, Ho); if (rc) return rc;
    float* d1 = alloc(act_n(Ho, cout));
    rc = conv(dout, W(m.idx, "Conv_1.weight"), nullptr, d1, cout, cout, Ho, {.layout = NHWC | CSD_WEIGHT_T}); if (rc) return rc;
    if (sp.mask) TG_RUN(csd_mul(d1, sp.mask, d1, (int64_t)act_n(Ho, cout), s));
    // GroupNorm_1 + act
    float* d1b = alloc(act_n(Ho, cout));
    rc = gn_bwd(sp.c0, W(m.idx, "GroupNorm_1.weight"), W(m.idx, "GroupNorm_1.bias"), sp.rs1, sp.ms1, d1, d1b, DW(m.idx, "GroupNorm_1.weight"),
                DW(m.idx, "GroupNorm_1.bias"), cout, Ho, act);
    if (rc) return rc;
    d1 = d1b;
    // Conv_0 bias and the time-embedding row share the per-(sample, channel) pixel sums of d1
    if (pg) {
      float* dd = alloc((size_t)B * cout);
      rc = sum_pixels(d1, dd, cout, Ho); if (rc) return rc;
      TG_RUN(sum_rows_beta(dd, DW(m.idx, "Conv_0.bias"), B, cout, gacc, s));
      if (f.dense) {
        rc = linear_bwd(st.temb2_act, CSD_ACT_NONE, W(m.idx, "Dense_0.weight"), dd, DW(m.idx, "Dense_0.weight"), DW(m.idx, "Dense_0.bias"), dtemb_act,
                        4 * n.cfg.nf, cout);
        if (rc) return rc;
      }
    }
    rc = wgrad(sp.op0, d1, DW(m.idx, "Conv_0.weight"), cin, cout, Ho); if (rc) return rc;
    float* d0 = alloc(act_n(Ho, cin));
    rc = conv(d1, W(m.idx, "Conv_0.weight"), nullptr, d0, cout, cin, Ho, {.layout = NHWC | CSD_WEIGHT_T}); if (rc) return rc;
    if (f.resample()) {                              // through the FIR of the h branch: the other direction's geometry, flipped taps
      float* d0l = alloc(act_n(H, cin));
      rc = fir(d0, d0l, B, Ho, cin, !f.up, true); if (rc) return rc;
      d0 = d0l;
    }
    const float* add = dout;                         // the identity shortcut's gradient; it joins dh inside the GroupNorm_0 backward
    if (f.sc_w) {
      rc = f.sc_swap ? wgrad(dout, xs, DW(m.idx, f.sc_w), cout, cin, Ho, {.k = 1}) : wgrad(xs, dout, DW(m.idx, f.sc_w), cin, cout, Ho, {.k = 1});
      if (rc) return rc;
      rc = bias_grad(dout, DW(m.idx, f.sc_b), cout, Ho); if (rc) return rc;
      float* dsc = alloc(act_n(Ho, cin));
      rc = conv(dout, W(m.idx, f.sc_w), nullptr, dsc, cout, cin, Ho, {.k = 1, .layout = f.sc_dgrad_layout}); if (rc) return rc;
      if (f.resample()) {
        float* dscl = alloc(act_n(H, cin));
        rc = fir(dsc, dscl, B, Ho, cin, !f.up, true); if (rc) return rc;
        dsc = dscl;
      }
      add = dsc;
    }
    rc = gn_bwd(h, W(m.idx, "GroupNorm_0.weight"), W(m.idx, "GroupNorm_0.bias"), sp.rs0, sp.ms0, d0, dh, DW(m.idx, "GroupNorm_0.weight"),
                DW(m.idx, "GroupNorm_0.bias"), cin, H, act, add);
    if (rc) return rc;
    top = mk;
    return contribute(sp.in0, dh);
  }

  // the head or one level of the output pyramid (out_fwd): conv weight gradient, NCHW bias sum, transposed conv, GroupNorm backward;
  // a pyramid level that added FIR-up of the coarser level hands that level its gradient
  int out_bwd(const TStep& sp, const float* d_out) {
    const Module& mg = n.mods[sp.mod];
    const Module& mc = n.mods[sp.mod + 1];
    const TT& tin = st.t[sp.in0];
    const int H = tin.H, C = mg.cin, Co = n.cfg.out_channels;
    const float* dP = (sp.kind == TS_HEAD || (sp.flag & PYR_CALLER_OUT)) ? d_out : st.t[sp.out].g;
    float* dh = alloc(act_n(H, C));
    float* dprev = (sp.flag & PYR_ADDS_COARSER) ? alloc((size_t)B * Co * (H / 2) * (H / 2)) : nullptr;
    const size_t mk = top;
    int rc = wgrad(sp.op0, dP, DW(mc.idx, "weight"), C, Co, H, {.layout = CSD_IN_NHWC}); if (rc) return rc;
    if (pg) {                                        // bias: NCHW gradient -> per-(sample, channel) sums -> batch sum
      float* bc = alloc((size_t)B * Co);
      TG_RUN(csd_sum_inner(dP, bc, (int64_t)B * Co, (int64_t)H * H, s));
      TG_RUN(sum_rows_beta(bc, DW(mc.idx, "bias"), B, Co, gacc, s));
    }
    float* dg = alloc(act_n(H, C));
    rc = conv(dP, W(mc.idx, "weight"), nullptr, dg, Co, C, H, {.layout = CSD_OUT_NHWC | CSD_WEIGHT_T}); if (rc) return rc;      // NCHW in
    rc = gn_bwd(tin.p, W(mg.idx, "weight"), W(mg.idx, "bias"), sp.rs0, sp.ms0, dg, dh, DW(mg.idx, "weight"), DW(mg.idx, "bias"), C, H, act);
    if (rc) return rc;
    if (dprev) { rc = fir(dP, dprev, B * Co, H, 1, false, true); if (rc) return rc; }      // d pyramid_upsample
    top = mk;
    rc = contribute(sp.in0, dh); if (rc) return rc;
    if (dprev) st.t[sp.in1].g = dprev;               // (the coarser level's only consumer)
    return CSD_OK;
  }

  int attn_bwd(const TStep& sp) {
    const Module& m = n.mods[sp.mod];
    const TT& tin = st.t[sp.in0];
    const int H = tin.H, C = m.cin;
    const float* h = tin.p;
    float* dout = st.t[sp.out].g;
    float* dh = alloc(act_n(H, C));
    const size_t mk = top;
    int rc;
    if (skip_scale() != 1.f) {                       // AttnBlockpp: out = (x + h) / sqrt(2)
      float* ds = alloc(act_n(H, C));
      rc = scale_into(dout, ds, skip_scale(), act_n(H, C)); if (rc) return rc;
      dout = ds;
    }
    // NIN_3
    rc = wgrad(dout, sp.attn, DW(m.idx, "NIN_3.W"), C, C, H, {.k = 1}); if (rc) return rc;
    rc = bias_grad(dout, DW(m.idx, "NIN_3.b"), C, H); if (rc) return rc;
    float* da = alloc(act_n(H, C));
    rc = conv(dout, W(m.idx, "NIN_3.W"), nullptr, da, C, C, H, {.k = 1}); if (rc) return rc;
    // attention core
    float* dqkv = alloc(act_n(H, 3 * C));
    {
      const size_t m2 = top;
      float* sc = alloc_bytes(csd_attention_backward_scratch_bytes(B, C, H * H, 1));
      TG_RUN(csd_attention_backward_nhwc(sp.qkv, da, dqkv, B, H * H, C, sc, s));
      top = m2;
    }
    // q | k | v contraction: gradients of the concatenated weight, scattered back to NIN_0..2
    float* wc = alloc((size_t)C * 3 * C);
    float* dwc = alloc((size_t)C * 3 * C);
    float* dbc = alloc(3 * C);
    rc = wgrad(dqkv, sp.op0, dwc, 3 * C, C, H, {.k = 1, .temp = true}); if (rc) return rc;      // dW[i, o] with o over 3C
    rc = bias_grad(dqkv, dbc, 3 * C, H, true); if (rc) return rc;
    rc = qkv_weight(m.idx, C, wc, nullptr); if (rc) return rc;
    for (int j = 0; j < 3 && !dry && pg; ++j) {
      hipLaunchKernelGGL(copy2d_kernel, dim3(launch_blocks((size_t)C * C)), dim3(256), 0, s, dwc + j * C, 3 * C, DW(m.idx, QKV_W[j]), C, C, C, gacc);
      CSD_LAUNCH_CHECK();
      if (gacc) {                                    // (the bias slice: one row of the same kernel; the overwrite form stays a device copy)
        hipLaunchKernelGGL(copy2d_kernel, dim3(launch_blocks((size_t)C)), dim3(256), 0, s, dbc + j * C, C, DW(m.idx, QKV_B[j]), C, C, 1, 1);
        CSD_LAUNCH_CHECK();
      } else {
        TG_RUN(copy(dbc + j * C, DW(m.idx, QKV_B[j]), C));
      }
    }
    rc = conv(dqkv, wc, nullptr, da, 3 * C, C, H, {.k = 1}); if (rc) return rc;    // dt = dqkv . Wcat^T (Wcat read as OIHW [C, 3C])
    rc = gn_bwd(h, W(m.idx, "GroupNorm_0.weight"), W(m.idx, "GroupNorm_0.bias"), sp.rs0, sp.ms0, da, dh, DW(m.idx, "GroupNorm_0.weight"),
                DW(m.idx, "GroupNorm_0.bias"), C, H, CSD_ACT_NONE, dout);
    if (rc) return rc;
    top = mk;
    return contribute(sp.in0, dh);
  }

  // ---- d loss / d x: the network input is cat(x, y) NCHW (2h - 1 when not centred); only its x channels take a gradient ------------
  float in_scale() const { return n.cfg.centered ? 1.f : 2.f; }
  // the x-channel columns [rows, cx * k2] of an input-layer weight [rows, cio * k2], times in_scale(): the transposed-weight
  // convolution (layout bit 2) with this slice writes the x channels only, the 2x - 1 map folded in (a power of two: exact)
  int x_weight_slice(const float* w, int rows, int k2, float** out) {
    const int cx = n.cfg.x_channels, cio = cx + n.cfg.y_channels;
    float* ws = alloc((size_t)rows * cx * k2);
    *out = ws;
    if (!dry) {
      hipLaunchKernelGGL(wslice_kernel, dim3(launch_blocks((size_t)rows * cx * k2)), dim3(256), 0, s, w, cio * k2, ws, cx * k2, cx * k2, rows,
                         in_scale());
      CSD_LAUNCH_CHECK();
    }
    return CSD_OK;
  }
  // d pyramid_l = Conv_0^T(dh_l) + FIR-down^T(d pyramid_{l+1})  (input_skip: pyramid_l = FIR-down(pyramid_{l-1}), pyramid_0 = the input)
  int pyramid_dx(const Module& m, const TT& to) {
    const int cx = n.cfg.x_channels, side = to.H;
    const size_t np = (size_t)B * cx * side * side;
    float* g = alloc(np);                            // kept until the next finer level (or the stem) has read it
    const size_t mk = top;
    float* w = nullptr;
    int rc = x_weight_slice(W(m.idx, "Conv_0.weight"), m.cout, 1, &w); if (rc) return rc;
    rc = conv(to.g, w, nullptr, g, m.cout, cx, side, {.k = 1, .layout = CSD_IN_NHWC | CSD_WEIGHT_T}); if (rc) return rc;
    if (dpyr) {
      float* u = alloc(np);
      rc = fir(dpyr, u, B * cx, side / 2, 1, true, true); if (rc) return rc;
      rc = add_into(g, u, np); if (rc) return rc;
    }
    top = mk;
    dpyr = g;
    return CSD_OK;
  }
  // the first 3x3 conv's data gradient, NHWC nf channels -> NCHW x channels, + FIR-down^T of the input pyramid's gradient
  int stem_dx(const Module& m, const TT& to) {
    const int cx = n.cfg.x_channels, S = to.H;
    const size_t np = (size_t)B * cx * S * S;
    const size_t mk = top;
    float* const d_x_caller = d_x;
    if (n.cfg.x_squeeze) d_x = alloc(np);            // (the squeezed gradient; scattered into the caller's image below)
    float* w = nullptr;
    int rc = x_weight_slice(W(m.idx, "weight"), n.cfg.nf, 9, &w); if (rc) return rc;
    rc = conv(to.g, w, nullptr, d_x, n.cfg.nf, cx, S, {.layout = CSD_IN_NHWC | CSD_WEIGHT_T}); if (rc) return rc;
    if (dpyr) {
      float* u = alloc(np);
      rc = fir(dpyr, u, B * cx, S / 2, 1, true, true); if (rc) return rc;
      rc = add_into(d_x, u, np); if (rc) return rc;
    }
    if (dres0) { rc = add_into(d_x, dres0, np); if (rc) return rc; }
    if (n.cfg.x_squeeze) {
      TG_RUN(sq_scatter_launch(d_x, (size_t)cx * S * S, d_x_caller, (size_t)cx * S * S, B, cx, S, s));
      d_x = d_x_caller;
    }
    top = mk;
    return CSD_OK;
  }

  int backward(const float* d_out) {
    const csd_unet_config& c = n.cfg;
    const int nf = c.nf;
    top = st.fwd_top;
    int rc;
    if (c.x_squeeze) {                               // d_out arrives in the layout of `out`: gather its x block, copy the rest
      const int S = c.image_size, cx = c.x_channels;
      const size_t hw = (size_t)S * S, ld = (size_t)c.out_channels * hw;
      float* dn = alloc((size_t)B * ld);
      if (!dry) {
        TG_RUN(sq_gather_launch(d_out, ld, dn, ld, B, cx, S, s));
        if (c.out_channels > cx)
          CSD_CHECK_HIP(hipMemcpy2DAsync(dn + cx * hw, ld * 4, d_out + cx * hw, ld * 4, (c.out_channels - cx) * hw * 4, B,
                                         hipMemcpyDeviceToDevice, s));
      }
      d_out = dn;
    }
    if (c.y_scale) {                                 // d_out arrives in the layout of `out`: copy its x block, the adjoint of bilin_down for the rest
      const int S = c.image_size, cx = c.x_channels;
      const size_t hw = (size_t)S * S, ld = (size_t)c.out_channels * hw, ldo = out_sample_elems(c);
      float* dn = alloc((size_t)B * ld);
      if (!dry) {
        CSD_CHECK_HIP(hipMemcpy2DAsync(dn, ld * 4, d_out, ldo * 4, cx * hw * 4, B, hipMemcpyDeviceToDevice, s));
        if (c.out_channels > cx)
          TG_RUN(bilinear_down_adjoint_launch(d_out + cx * hw, ldo, dn + cx * hw, ld, B, c.out_channels - cx, S, c.y_scale, s));
      }
      d_out = dn;
    }
    float* dtemb_act = nullptr;                      // sum over the blocks of dDense . W: gradient w.r.t. act(temb2)
    dpyr = nullptr;
    dres0 = nullptr;
    if (c.conditional && pg) {
      dtemb_act = alloc((size_t)B * 4 * nf);
      if (!dry) CSD_CHECK_HIP(hipMemsetAsync(dtemb_act, 0, (size_t)B * 4 * nf * sizeof(float), s));
    }
    // the marks may follow the steps only if the recorded steps walk the modules in ascending order (they do: the forward consumes
    // all_modules front to back) - otherwise every mark waits for the end of the backward
    bool ordered = true;
    {
      int last = -1;
      for (const TStep& sp : st.steps) {
        if (sp.mod < 0) continue;
        const int idx = n.mods[sp.mod].idx;
        if (idx < last) ordered = false;
        last = idx;
      }
    }
    for (int i = (int)st.steps.size() - 1; i >= 0; --i) {
      const TStep& sp = st.steps[i];
      if (i + 1 < (int)st.steps.size() && ordered && st.steps[i + 1].mod >= 0) {      // step i + 1 and everything after it is complete
        rc = marks_reached(n.mods[st.steps[i + 1].mod].idx); if (rc) return rc;
      }
      switch (sp.kind) {
        case TS_HEAD: case TS_PYR: rc = out_bwd(sp, d_out); if (rc) return rc; break;
        case TS_RES: rc = res_bwd(sp, dtemb_act); if (rc) return rc; break;
        case TS_COMBINE: {                           // out = Conv_0(pyramid) + h: h's gradient is dout; the pyramid's only when d_x is wanted
          const Module& m = n.mods[sp.mod];
          const TT& to = st.t[sp.out];
          const int cio = c.x_channels + c.y_channels;
          rc = wgrad(sp.pyr, to.g, DW(m.idx, "Conv_0.weight"), cio, m.cout, to.H, {.k = 1, .layout = CSD_OUT_NHWC}); if (rc) return rc;
          rc = bias_grad(to.g, DW(m.idx, "Conv_0.bias"), m.cout, to.H); if (rc) return rc;
          if (want_dx) { rc = pyramid_dx(m, to); if (rc) return rc; }
          rc = contribute(sp.in0, to.g); if (rc) return rc;
          break;
        }
        case TS_RPYR: {                              // out = (Downsample(src) + h) * k: d h = d Downsample = k dout
          const Module& m = n.mods[sp.mod];
          const TT& to = st.t[sp.out];
          const int side = to.H, Hs = 2 * side, Cin = m.cin, C = m.cout, cx = c.x_channels;
          const bool fir = c.progressive_input == 2;
          float* dh = to.g;
          if (skip_scale() != 1.f) { dh = alloc(act_n(side, C)); rc = scale_into(to.g, dh, skip_scale(), act_n(side, C)); if (rc) return rc; }
          // the source's gradient: always into the previous level's combined h (the parameter gradients upstream depend on it); at level 0
          // into d_x only when it is wanted (the x channels, times the 2x - 1 input map's 2 when not centred)
          float* dsrc = sp.in1 >= 0 ? alloc(act_n(Hs, Cin)) : nullptr;
          if (sp.in1 < 0 && want_dx) dres0 = alloc((size_t)B * cx * Hs * Hs);
          const size_t mk = top;
          const PyrSrc ps = pyr_src(sp.in1, Hs, Cin);
          rc = bias_grad(dh, DW(m.idx, pyr_sub(c, true)), C, side); if (rc) return rc;
          if (pg) {
            float* part = alloc(fir_pyr_wgrad_scratch_floats(B, Cin, C));
            TG_RUN(fir_pyr_wgrad_launch(ps.p, ps.sb, ps.sp, ps.sc, B, Hs, Cin, dh, C, pyr_taps(), fir, DW(m.idx, pyr_sub(c, false)), part, s, gacc));
          }
          if (dsrc || (sp.in1 < 0 && want_dx)) {
            float* gt = alloc((size_t)36 * Cin * C);
            TG_RUN(fir_pyr_fold_launch(W(m.idx, pyr_sub(c, false)), Cin, C, pyr_taps(), nullptr, gt, s));
            if (dsrc) TG_RUN(fir_pyr_dgrad_launch(dh, gt, dsrc, (int64_t)Hs * Hs * Cin, Cin, 1, B, Hs, Cin, Cin, C, fir, 1.f, s));
            else TG_RUN(fir_pyr_dgrad_launch(dh, gt, dres0, (int64_t)cx * Hs * Hs, 1, (int64_t)Hs * Hs, B, Hs, Cin, cx, C, fir, in_scale(), s));
          }
          top = mk;
          rc = contribute(sp.in0, dh); if (rc) return rc;
          if (dsrc) { rc = contribute(sp.in1, dsrc); if (rc) return rc; }
          break;
        }
        case TS_ATTN: rc = attn_bwd(sp); if (rc) return rc; break;
        case TS_CAT: {
          const TT& ta = st.t[sp.in0];
          const TT& tb = st.t[sp.in1];
          float* da = alloc(act_n(ta.H, ta.C));
          float* db = alloc(act_n(tb.H, tb.C));
          if (!dry) {
            const size_t npix = (size_t)B * ta.H * ta.H;
            hipLaunchKernelGGL(split_c_kernel, dim3(launch_blocks(npix * (ta.C + tb.C) / 4)), dim3(256), 0, s,
                               reinterpret_cast<const float4*>(st.t[sp.out].g), ta.C / 4, tb.C / 4, reinterpret_cast<float4*>(da),
                               reinterpret_cast<float4*>(db), npix);
            CSD_LAUNCH_CHECK();
          }
          rc = contribute(sp.in0, da); if (rc) return rc;
          rc = contribute(sp.in1, db); if (rc) return rc;
          break;
        }
        case TS_UP: {                                // nearest x2 + conv: dx = 2x2 block sums of the full-resolution data gradient
          const Module& m = n.mods[sp.mod];
          const TT& tin = st.t[sp.in0];
          const int H = tin.H, C = m.cin;
          float* dout = st.t[sp.out].g;
          float* dh = alloc(act_n(H, C));
          const size_t mk = top;
          rc = wgrad(tin.p, dout, DW(m.idx, "Conv_0.weight"), C, C, H, {.up2 = 1}); if (rc) return rc;
          rc = bias_grad(dout, DW(m.idx, "Conv_0.bias"), C, 2 * H); if (rc) return rc;
          float* full = alloc(act_n(2 * H, C));
          rc = conv(dout, W(m.idx, "Conv_0.weight"), nullptr, full, C, C, 2 * H, {.layout = NHWC | CSD_WEIGHT_T}); if (rc) return rc;
          TG_RUN(csd_sumpool2_nhwc(full, dh, B, H, H, C, s));
          top = mk;
          rc = contribute(sp.in0, dh); if (rc) return rc;
          break;
        }
        case TS_DOWN: {                              // stride-2 conv: dy zero-inserted on the odd grid positions, then a pad-1 conv
          const Module& m = n.mods[sp.mod];
          const TT& tin = st.t[sp.in0];
          const int H = tin.H, C = m.cin;
          float* dout = st.t[sp.out].g;
          float* dh = alloc(act_n(H, C));
          const size_t mk = top;
          rc = wgrad(tin.p, dout, DW(m.idx, "Conv_0.weight"), C, C, H, {.stride = 2, .dpad = 1}); if (rc) return rc;
          rc = bias_grad(dout, DW(m.idx, "Conv_0.bias"), C, H / 2); if (rc) return rc;
          float* z = alloc(act_n(H, C));
          TG_RUN(csd_zero_insert_odd_nhwc(dout, z, B, H / 2, H / 2, C, s));
          rc = conv(z, W(m.idx, "Conv_0.weight"), nullptr, dh, C, C, H, {.layout = NHWC | CSD_WEIGHT_T}); if (rc) return rc;
          top = mk;
          rc = contribute(sp.in0, dh); if (rc) return rc;
          break;
        }
        case TS_STEM: {
          const Module& m = n.mods[sp.mod];
          const TT& to = st.t[sp.out];
          const int cio = c.x_channels + c.y_channels;
          rc = wgrad(st.xin, to.g, DW(m.idx, "weight"), cio, nf, to.H, {.layout = CSD_OUT_NHWC}); if (rc) return rc;
          rc = bias_grad(to.g, DW(m.idx, "bias"), nf, to.H); if (rc) return rc;
          if (want_dx) { rc = stem_dx(m, to); if (rc) return rc; }
          break;
        }
      }
    }
    if (c.conditional && pg) {                       // temb MLP (models/ddpm.py:153-160)
      const size_t mk = top;
      float* d2 = alloc((size_t)B * 4 * nf);         // gradient w.r.t. temb2 = act'(temb2) * dtemb_act
      TG_RUN(csd_act(st.temb2, dtemb_act, d2, act, (int64_t)B * 4 * nf, s));
      float* dact1 = alloc((size_t)B * 4 * nf);
      if (!dry) CSD_CHECK_HIP(hipMemsetAsync(dact1, 0, (size_t)B * 4 * nf * sizeof(float), s));
      const int l0 = st.lin0, l1 = st.lin0 + 1;
      rc = linear_bwd(st.temb1, act, W(l1, "weight"), d2, DW(l1, "weight"), DW(l1, "bias"), dact1, 4 * nf, 4 * nf); if (rc) return rc;
      float* d1 = alloc((size_t)B * 4 * nf);
      TG_RUN(csd_act(st.temb1, dact1, d1, act, (int64_t)B * 4 * nf, s));
      rc = linear_bwd(st.emb, CSD_ACT_NONE, W(l0, "weight"), d1, DW(l0, "weight"), DW(l0, "bias"), nullptr, st.emb_dim, 4 * nf); if (rc) return rc;
      // the Fourier W is a fixed buffer of the reference (requires_grad = False): its slot reads zero - and an accumulating backward adds
      // that zero: the slot is left as it is
      if (st.fourier_mod >= 0 && !dry && !gacc)
        CSD_CHECK_HIP(hipMemsetAsync(DW(st.fourier_mod, "W"), 0, (size_t)nf * sizeof(float), s));
      top = mk;
    }
    return marks_reached(-1);                        // (the embedding MLP holds the lowest module indices: everything is final now)
  }
#undef TG_RUN
};

// arch 2 (train_graph3d.h, included behind this file): the dry run's peak in floats, the forward and the backward on a TrainState
static size_t train3d_workspace_peak(Net& net, int B, float dropout_p);
static int train3d_forward(Net& net, TrainState& st, int B, hipStream_t s, const float* const* params, float* ws, float p_drop, uint64_t seed,
                           uint64_t call, const float* x, const float* y, const float* labels, float* out);
static int train3d_backward(Net& net, TrainState& st, int B, hipStream_t s, const float* const* params, float* const* grads, float* ws,
                            float* d_x, int accumulate, GradMarks* gm, const float* d_out);

static int train_check(const csd_unet* net) {
  CSD_REQUIRE(net, "train: null handle");
  const csd_unet_config& c = net->net.cfg;
  // (arch 2, the 3-D networks: train_graph3d.h, for a handle created with planned_train = 1; what build_modules3d refused never became a
  // handle.  They have no probability-flow right-hand side and no device-loop inpainting: the likelihood refuses them in Python)
  CSD_REQUIRE(c.arch != 2 || c.planned_train, "train graph: this handle of the 3-D networks (arch 2) was created without "
                                              "csd_unet_config.planned_train: it has no planned training graph or input gradient and "
                                              "trains on the per-operator path (the probability-flow right-hand side is not wired to 3-D)");
  CSD_REQUIRE(c.arch == 0 || c.arch == 1 || c.arch == 2, "train graph: arch %d has no planned training graph", c.arch);
  if (c.arch == 0) CSD_REQUIRE(c.resamp_with_conv, "train graph: resamp_with_conv = False is not provided");
  CSD_REQUIRE((c.x_channels + c.y_channels) >= 1, "train graph: no input channels");
  return CSD_OK;
}

}  // namespace csd

extern "C" size_t csd_unet_train_workspace_bytes(csd_unet* net, int B, float dropout_p) {
  if (!net || train_check(net) || B < 1) return 0;
  if (is3d(net->net)) {
    const size_t peak = train3d_workspace_peak(net->net, B, dropout_p);
    return peak ? peak * sizeof(float) + 256 : 0;
  }
  TrainState st;
  TG g(net->net, st, B, nullptr, true, nullptr, nullptr, reinterpret_cast<float*>(uintptr_t(256)));
  g.p_drop = dropout_p;
  g.want_dx = true;                                  // (sized for the largest backward: every parameter gradient and d_x)
  if (g.forward(nullptr, nullptr, nullptr, nullptr)) return 0;
  if (g.backward(nullptr)) return 0;
  return g.peak * sizeof(float) + 256;
}

extern "C" int csd_unet_train_forward(csd_unet* net, const float* const* params, void* workspace, size_t workspace_bytes,
                                      const float* x, const float* y, const float* labels, float* out, int B, float dropout_p,
                                      uint64_t dropout_seed, uint64_t call_index, void* stream) {
  int rc = train_check(net);
  if (rc) return rc;
  CSD_REQUIRE(params && workspace && x && out && B >= 1, "train_forward: null argument");
  CSD_REQUIRE((net->net.cfg.y_channels == 0) == (y == nullptr), "train_forward: y must be given iff y_channels > 0");
  CSD_REQUIRE(!net->net.cfg.conditional || labels, "train_forward: labels required for a conditional network");
  CSD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "train_forward: workspace must be 256-byte aligned");
  CSD_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "train_forward: dropout_p %g out of range", dropout_p);
  const size_t need = csd_unet_train_workspace_bytes(net, B, dropout_p);
  if (workspace_bytes < need) {
    set_error("train_forward: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    return CSD_ERR_WORKSPACE;
  }
  for (size_t i = 0; i < net->net.params.size(); ++i)
    CSD_REQUIRE(params[i], "train_forward: parameter %zu (%s) is null", i, net->net.params[i].name.c_str());
  train_state_purge_stale(&net->net, workspace);
  TrainState& st = train_state_of(&net->net, workspace);
  st.valid = false;
  if (is3d(net->net)) {
    rc = train3d_forward(net->net, st, B, (hipStream_t)stream, params, static_cast<float*>(workspace), dropout_p, dropout_seed, call_index, x,
                         y, labels, out);
  } else {
    TG g(net->net, st, B, (hipStream_t)stream, false, params, nullptr, static_cast<float*>(workspace));
    g.p_drop = dropout_p; g.seed = dropout_seed; g.call = call_index;
    rc = g.forward(x, y, labels, out);
  }
  if (rc) return rc;
  st.valid = true; st.B = B; st.ws = workspace; st.p_drop = dropout_p; st.call = call_index;
  return CSD_OK;
}

extern "C" int csd_unet_train_release(csd_unet* net, const void* workspace) {
  int rc = train_check(net);
  if (rc) return rc;
  train_state_erase_one(&net->net, workspace);
  return CSD_OK;
}

extern "C" int csd_unet_train_release_call(csd_unet* net, const void* workspace, uint64_t call_index) {
  int rc = train_check(net);
  if (rc) return rc;
  train_state_erase_one(&net->net, workspace, &call_index);
  return CSD_OK;
}

extern "C" int csd_unet_backward(csd_unet* net, const float* const* params, float* const* grads, void* workspace,
                                 size_t workspace_bytes, const float* d_out, int B, uint64_t call_index, void* stream) {
  CSD_REQUIRE(grads, "backward: null argument");
  return csd_unet_backward_ex(net, params, grads, nullptr, workspace, workspace_bytes, d_out, B, call_index, stream);
}

extern "C" int csd_unet_backward_ex(csd_unet* net, const float* const* params, float* const* grads, float* d_x, void* workspace,
                                    size_t workspace_bytes, const float* d_out, int B, uint64_t call_index, void* stream) {
  return csd_unet_backward_acc(net, params, grads, d_x, workspace, workspace_bytes, d_out, B, call_index, 0, 1, stream);
}

extern "C" int csd_unet_backward_acc(csd_unet* net, const float* const* params, float* const* grads, float* d_x, void* workspace,
                                     size_t workspace_bytes, const float* d_out, int B, uint64_t call_index, int accumulate,
                                     int record_marks, void* stream) {
  int rc = train_check(net);
  if (rc) return rc;
  CSD_REQUIRE((accumulate == 0 || accumulate == 1) && (record_marks == 0 || record_marks == 1),
              "backward_acc: accumulate (%d) and record_marks (%d) are 0 or 1", accumulate, record_marks);
  CSD_REQUIRE(!accumulate || grads, "backward_acc: accumulate = 1 needs parameter gradients (grads) to add to");
  CSD_REQUIRE(params && workspace && d_out, "backward: null argument");
  CSD_REQUIRE(grads || d_x, "backward_ex: neither parameter gradients (grads) nor the input gradient (d_x) requested");
  if (d_x) {
    const csd_unet_config& c = net->net.cfg;
    CSD_REQUIRE(c.x_channels >= 1, "backward_ex: d_x needs x_channels >= 1");
    CSD_REQUIRE(c.arch == 0 || (c.progressive_input >= 0 && c.progressive_input <= 3),
                "backward_ex: d_x is not provided for progressive_input id %d", c.progressive_input);
  }
  TrainState* sp = train_state_find(&net->net, workspace);
  if (!sp || !sp->valid || sp->B != B || sp->ws != workspace) {
    set_error("backward: no matching csd_unet_train_forward (same handle, workspace and batch) precedes this call");
    return CSD_ERR_STATE;
  }
  TrainState& st = *sp;
  if (st.call != call_index) {
    set_error("backward: the workspace holds the activations of csd_unet_train_forward call %llu, not of call %llu (a later forward "
              "re-used it before this backward ran)", (unsigned long long)st.call, (unsigned long long)call_index);
    return CSD_ERR_STATE;
  }
  const size_t need = csd_unet_train_workspace_bytes(net, B, st.p_drop);
  if (workspace_bytes < need) {
    set_error("backward: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    return CSD_ERR_WORKSPACE;
  }
  for (size_t i = 0; i < net->net.params.size(); ++i)
    CSD_REQUIRE(params[i] && (!grads || grads[i]), "backward: parameter / gradient pointer %zu (%s) is null", i, net->net.params[i].name.c_str());
  for (auto& t : st.t) t.g = nullptr;
  GradMarks* gm = nullptr;
  if (grads && record_marks) {                                       // (the gradient-ready marks describe parameter gradients: none without them)
    std::lock_guard<std::mutex> lk(g_train_mu);
    auto it = g_marks.find(&net->net);
    gm = it == g_marks.end() ? nullptr : &it->second;
  }
  if (is3d(net->net)) {
    rc = train3d_backward(net->net, st, B, (hipStream_t)stream, params, grads, static_cast<float*>(workspace), d_x, accumulate, gm, d_out);
  } else {
    TG g(net->net, st, B, (hipStream_t)stream, false, params, grads, static_cast<float*>(workspace));
    g.pg = grads != nullptr;
    g.gacc = accumulate;
    g.want_dx = d_x != nullptr;
    g.d_x = d_x;
    g.gm = gm;
    rc = g.backward(d_out);
  }
  if (!rc && gm) ++gm->epoch;
  st.valid = false;                                  // the saved activations are consumed (gradient buffers overwrote nothing, but one backward per forward)
  return rc;
}

// ---- gradient-ready marks + the event / stream helpers a data-parallel caller needs to overlap its all-reduce with the backward ----
extern "C" int csd_unet_backward_marks(csd_unet* net, const int* first_module, void* const* events, int n) {
  int rc = csd::train_check(net);
  if (rc) return rc;
  CSD_REQUIRE(n >= 0 && (n == 0 || (first_module && events)), "backward_marks: null argument");
  std::lock_guard<std::mutex> lk(csd::g_train_mu);
  if (n == 0) { csd::g_marks.erase(&net->net); return CSD_OK; }
  csd::GradMarks& gm = csd::g_marks[&net->net];
  gm.marks.clear();
  for (int k = 0; k < n; ++k) {
    CSD_REQUIRE(events[k], "backward_marks: event %d is null", k);
    gm.marks.emplace_back(first_module[k], static_cast<hipEvent_t>(events[k]));
  }
  std::stable_sort(gm.marks.begin(), gm.marks.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
  return CSD_OK;
}
extern "C" uint64_t csd_unet_backward_marks_epoch(csd_unet* net) {
  if (!net) return 0;
  std::lock_guard<std::mutex> lk(csd::g_train_mu);
  auto it = csd::g_marks.find(&net->net);
  return it == csd::g_marks.end() ? 0 : it->second.epoch;
}
extern "C" void* csd_event_create(void) {
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
  return e;
}
extern "C" int csd_event_destroy(void* event) {
  if (event) CSD_CHECK_HIP(hipEventDestroy(static_cast<hipEvent_t>(event)));
  return CSD_OK;
}
extern "C" int csd_stream_wait_event(void* stream, void* event) {
  CSD_REQUIRE(event, "stream_wait_event: null event");
  CSD_CHECK_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(event), 0));
  return CSD_OK;
}
extern "C" int csd_event_query(void* event) {      /* 1: complete, 0: not yet, < 0: error */
  CSD_REQUIRE(event, "event_query: null event");
  const hipError_t e = hipEventQuery(static_cast<hipEvent_t>(event));
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  csd::set_error("event_query: %s", hipGetErrorString(e));
  return CSD_ERR_HIP;
}
