// unet.hip - graph executor for the DDPM-family score network + the fused PC sampling loop,
// and the C-ABI entry points around them.
//
// Replaces (reference, behaviour only): models/ddpm.py:80-213 (DDPM.__init__/forward),
// :275-298 (paired wrappers), the per-step glue of sampling/conditional.py:180-226 and
// sampling/unconditional.py:194-226.  The module list is rebuilt from the config values exactly
// as DDPM.__init__ does, so parameter names/indices equal the reference state_dict
// ("all_modules.{i}.Conv_0.weight" ...).  Execution is a flat, pre-planned list of kernel
// launches on ONE stream: no per-step host objects, no allocation, no synchronisation.
//
// One translation unit in pieces: this file (structs, the topology = build_modules, the parameter table, the C ABI of the network),
// pc_loop.h (the fused PC sampler: its noise-draw schedule, the loop, the csd_pc_* entries and the cascade), unet_layout.h (ConvKernel per layer, packed-weight layout + pack_all), unet_plan.h (Builder: the walk's state and one step() per module; build_plan; a batch chunk is planned by a Builder of its own), unet_run.h (run_plan), unet3d.h (the 3-D DDPM
// family, arch 2: topology, packed layout, plan and executor on conv3d.hip's kernels), train_graph.h (training forward / backward; train_graph3d.h: the 3-D family's),
// plan_digest.h (csd_unet_debug_digest).
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

#include "common.h"

namespace csd {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }

// ---------------------------------------------------------------------------------------------
// in-library profiler: HIP events around every launch of the network / sampler, recorded on the
// SAME stream the kernels run on (bench.py's roofline numbers come from here)
// ---------------------------------------------------------------------------------------------
struct ProfRec { hipEvent_t a, b; int cls; double flops, bytes, abytes; };
struct Profiler {
  bool on = false;
  unsigned mask = ~0u;        // launch classes that get events (bit = CSD_PROF_* id)
  int step_stride = 1;        // csd_pc_sample: only every step_stride-th PC step is bracketed
  bool step_on = true;
  std::vector<ProfRec> recs;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
  size_t used = 0;
};
// per calling thread: a host thread that drives its own handle / stream profiles its own launches (csd_profile_* carry no handle)
static thread_local Profiler g_prof;

struct ProfScope {
  hipStream_t s;
  hipEvent_t b = nullptr;
  ProfScope(int cls, double flops, double bytes, hipStream_t s_, double abytes = -1.0) : s(s_) {
    if (!g_prof.on || !g_prof.step_on || !((g_prof.mask >> cls) & 1u)) return;
    if (g_prof.used == g_prof.pool.size()) {
      hipEvent_t e0, e1;
      if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return;
      g_prof.pool.push_back({e0, e1});
    }
    auto& pr = g_prof.pool[g_prof.used++];
    (void)hipEventRecord(pr.first, s);
    b = pr.second;
    g_prof.recs.push_back({pr.first, pr.second, cls, flops, bytes, abytes < 0 ? bytes : abytes});
  }
  ~ProfScope() {
    if (b) (void)hipEventRecord(b, s);
  }
};

// ---------------------------------------------------------------------------------------------
// parameters
// ---------------------------------------------------------------------------------------------
struct Param {
  std::string name;
  int ndim;
  int64_t shape[5];        // (5-D: the 3-D family's convolution weights)
  int64_t numel;
  const float* ptr = nullptr;
};

enum ModKind { M_LINEAR, M_CONV3, M_RES, M_ATTN, M_DOWN, M_UP, M_GN, M_FOURIER, M_COMBINE, M_PYR };      // M_PYR: the 'residual' input pyramid's Downsample
// what a module does in the U-Net.  build_modules is the only place that knows the order of the network: the packed layout, the plan and
// the training forward are each ONE loop over Net::mods with a switch on the role
enum Role {
  R_EMB_FOURIER, R_EMB_LINEAR0, R_EMB_LINEAR1,      // time embedding: Gaussian Fourier features (NCSN++, optional), the two Linear layers
  R_STEM,
  R_DOWN_BLOCK, R_ATTN,                             // (R_ATTN: behind a block of either path)
  R_DOWNSAMPLE,                                     // M_DOWN (conv or average pool) / BigGAN `down` block
  R_COMBINE, R_PYR_DOWN,                            // NCSN++ input pyramid behind a downsample: Combine 'sum' / the 'residual' Downsample
  R_MID_RES_IN, R_MID_ATTN, R_MID_RES_OUT,
  R_UP_BLOCK,
  R_PYR_GN, R_PYR_CONV,                             // NCSN++ output pyramid of a level (level 0: it writes the network's output)
  R_UPSAMPLE,                                       // M_UP (conv or nearest) / BigGAN `up` block
  R_HEAD_GN, R_HEAD_CONV
};
struct Module {
  ModKind kind;
  int idx;
  int cin = 0, cout = 0;   // res / conv3 / linear ; attn/down/up/gn use cin as "channels"
  int up = 0, down = 0;    // NCSN++ ResnetBlockBigGANpp: FIR resampling of h and x inside the block
  Role role = R_STEM;
  int level = 0;           // U-Net level l
  int side = 0, out_side = 0;      // side of the map it reads (image_size >> l; R_COMBINE: the level below's, R_PYR_DOWN: the pyramid source's) / writes
  int skip = 0;            // R_UP_BLOCK: channels of the skip tensor it pops (its input is h | skip: c0 = cin - skip, c1 = skip)
  bool push = false;       // its output goes on the skip stack
  bool last_up = false;    // the last module of its level on the up path, in front of the level's output pyramid / upsample / the head
};

// the schedule a packed convolution runs on: chosen ONCE, in build_packed_layout (unet_layout.h); pack_all, the Builder, run_plan,
// split_conv3x3_classes and digest_layout switch on it
enum class ConvKernel {
  F32,             // conv_f32.hip: fp32 operands (the fp32 precision, and the layers no fp16 kernel takes)
  F16_LC,          // conv_f16*.hip: the fp16 kernel with its loader / consumer variant
  PW16,            // conv_pw16.hip: the pointwise fp16 kernel
  PW16_TAPS,       // ... on a 3x3 convolution with tap_cout (<= 6) output channels in its tap-partial form: proto is the POINTWISE
                   // contraction to 9 * tap_cout partial channels, a 9-tap gather (OP_TAPSUM) finishes it
  QUAD,            // conv_f16_q.hip: the quad-wave fp16 kernel
  QUAD_UP4,        // ... on the nearest-x2 Upsample conv in its phase-decomposed form (4 x 2x2 taps; UP4)
  FUSED,           // conv_ff.hip / conv_fx.hip / conv_xk.hip: the fused-prologue family - fp32 sources, no gn_apply16 pass
  STEM             // stem.hip: the first layer fused with the input assembly: x, y (NCHW) -> nf channels NHWC
};
static inline bool is_quad(ConvKernel k) { return k == ConvKernel::QUAD || k == ConvKernel::QUAD_UP4; }
static inline bool is_pw16(ConvKernel k) { return k == ConvKernel::PW16 || k == ConvKernel::PW16_TAPS; }

// one packed convolution weight (+bias): where it lives inside the packed buffer
struct PackedConv {
  ConvPlan proto;          // channel-level fields only (C0,C1,Cout,taps,KC,NT,CoutPad)
  size_t w_off = 0, b_off = 0;   // float offsets in the packed buffer
  ConvKernel kernel = ConvKernel::F32;
  int ns = 0;                    // operand planes of the fp16 kernels' layout: 1 / 2, 3: fp16 hi*hi + fp8 corrections (0: ConvKernel::F32)
  int tap_cout = 0;              // ConvKernel::PW16_TAPS: the layer's own output channels
  struct Src { int param_w, param_b, layout, cout_src, cout_off, cin_src; };
  std::vector<Src> srcs;
};

struct Net;

// ---------------------------------------------------------------------------------------------
// execution plan for one batch size
// ---------------------------------------------------------------------------------------------
enum OpKind { OP_ASSEMBLE, OP_STEM, OP_TEMB, OP_FOURIER, OP_FIR, OP_FIR2, OP_GN_APPLY32, OP_LINEAR, OP_GN_STATS, OP_GN_FINAL, OP_GN_FINAL_TILES, OP_GN_APPLY16, OP_GN_FUSED16, OP_GN_STATFIN, OP_CONV, OP_ATTN, OP_AVGPOOL,
              OP_UPNEAR, OP_TO_NCHW, OP_TAPSUM, OP_PYRCONV,
              OP_FORK, OP_JOIN };     // batch-chunk region (build_plan): the chunk streams start behind / the main stream resumes behind them

static const size_t NONE = (size_t)-1;

// what the sources of an OP_CONV hold
enum class ConvSrc {
  F32,             // fp32 tensors (src0 | src1)
  PLANES16,        // the fp16 planes an OP_GN_APPLY16 / OP_GN_FUSED16 wrote: src0 = hi, src1 = lo (ns >= 2)
  SPLIT_STAGING    // one fp32 tensor that the quad kernel splits into fp16 operands while it stages it
};

// one launch of the plan.  Every field is named for what it is; a kind fills the ones its launch takes (the comment behind a field
// says which), run_plan (unet_run.h) reads them by name.  Offsets are floats into the workspace unless stated; NONE: absent
struct Op {
  // ---- shared by every kind (all that fold_small_gn_pairs, interleave_chunks and the chunk stamping of build_plan touch) ----
  OpKind kind;
  int cls = CSD_PROF_OTHER;           // profiling class
  double flops = 0, bytes = 0;        // algorithmic flops of this launch; bytes THIS kernel has to move
  double abytes = -1;                 // SURVEY 8(d) bytes of the layer (input + output tensor, fp32) where they differ from `bytes`
  int nb = 0;                         // batch of THIS launch (0: the plan's) - the ops of a batch chunk carry the chunk's size
  int stream = 0;                     // 0: the caller's stream; k > 0: chunk stream k - 1 (between an OP_FORK and its OP_JOIN)
  int chunk = 0;                      // k + 1 for the ops of batch chunk k (chunk 0 runs on the caller's stream)
  int side = 0;                       // 1: launched on the side stream (after the main stream's work so far); 2: the main stream waits for it first
  // ---- tensors ----
  size_t src0 = NONE, src1 = NONE;    // sources (src1: the second of a virtual concat; OP_CONV from ConvSrc::PLANES16: the hi / lo planes)
  size_t out = NONE;                  // destination (OP_GN_APPLY16 / OP_GN_FUSED16: the hi plane; OP_FIR2: FIR(act(GroupNorm(x))))
  size_t out2 = NONE;                 // OP_GN_APPLY16 / OP_GN_FUSED16: the lo plane; OP_FIR2: FIR(x); OP_STEM: room for the perturbed y of a y_scale network
  size_t res = NONE;                  // OP_CONV / OP_TAPSUM / OP_PYRCONV: the tensor the epilogue adds
  size_t nscale = NONE, nshift = NONE;      // GroupNorm scale / shift per (sample, channel): OP_GN_FINAL / OP_GN_FINAL_TILES / OP_GN_STATFIN write
                                            // them; OP_CONV, OP_GN_APPLY16, OP_GN_APPLY32 and OP_FIR2 read them
  size_t stats = NONE, stats1 = NONE; // GroupNorm partial sums (doubles): OP_CONV / OP_STEM (per tile) and OP_GN_STATS write `stats`,
                                      // OP_GN_FINAL reads it; OP_GN_FINAL_TILES reads source 0's and source 1's
  size_t temb_base = NONE;            // OP_CONV: offset of dense_all (the epilogue's time-embedding source) ...
  size_t temb_col = NONE;             // ... the layer's first column inside it (NONE: no time embedding) ...
  int temb_stride = 0;                // ... and its row length
  size_t pk_w = NONE, pk_b = NONE;    // float offsets in the PACKED buffer: weight / bias (the GroupNorm kinds: gamma / beta; OP_FOURIER: W)
  // ---- OP_CONV (cp: also its geometry) / OP_STEM ----
  ConvPlan cp;
  ConvKernel kernel = ConvKernel::F32;
  ConvSrc src_form = ConvSrc::F32;
  int ns = 0;                         // PackedConv::ns of the layer
  int out_external = 0;               // OP_CONV / OP_TAPSUM: writes the caller's NCHW output
  float out_scale = 1.f;              // OP_CONV / OP_TAPSUM / OP_PYRCONV: the epilogue's factor
  int act = 0;                        // activation the launch applies (behind the GroupNorm where there is one)
  int out_act = 0;                    // OP_LINEAR: the activation every consumer would apply to this output, applied ONCE by the producer (the
                                      // consumers used to recompute it per workgroup: 396 x 24.6 k SiLUs in the Dense_0 launch)
  // ---- the other kinds' extents ----
  GNPlan gp;                          // OP_GN_STATS / OP_GN_FINAL / OP_GN_STATFIN / OP_GN_FUSED16 (OP_GN_FINAL_TILES: G only)
  int C0 = 0, C1 = 0;                 // channels of src0 / src1 (OP_LINEAR: input features; OP_TEMB / OP_FOURIER: nf)
  int Cout = 0;                       // OP_STEM / OP_TAPSUM / OP_PYRCONV: output channels; OP_LINEAR: output features
  int H = 0, W = 0;                   // extent of the SOURCE map (OP_FIR*, OP_AVGPOOL, OP_UPNEAR, OP_PYRCONV, OP_TAPSUM)
  int hw = 0;                         // pixels per sample (the GroupNorm kinds; OP_ATTN: tokens)
  int tiles0 = 0, tiles1 = 0;         // OP_GN_FINAL_TILES: partials per sample in stats / stats1
  int pix = 0;                        // OP_PYRCONV: floats per source pixel (>= C0: the padded input)
  bool up = false;                    // OP_FIR / OP_FIR2: upsample (else downsample)
  bool fir = false;                   // OP_PYRCONV: the FIR-folded 6x6 weight (else the plain stride-2 3x3)
  bool per_channel = false;           // OP_GN_STATS: per-channel partials in the tile-partial layout (G = 1) for OP_GN_FINAL_TILES
  bool fp8_lo = false;                // OP_GN_APPLY16 / OP_GN_FUSED16: the lo plane holds e4m3 byte pairs (ns == 3)
  int n_chunks = 0;                   // OP_FORK / OP_JOIN
};

struct Plan {
  int B = 0;
  std::vector<Op> ops;
  size_t ws_floats = 0;
  size_t ys_out = NONE;               // y_scale: the head's full-resolution output [B, out_channels, S, S], behind every other tensor
  int64_t launches = 0;
  double flops = 0, bytes = 0;
};

// ---- arch 2 (unet3d.h): one packed convolution weight, one launch (or GroupNorm launch pair) of the plan, the plan of one batch size ----
struct Conv3Slot {
  int param_w = -1, param_b = -1;
  int cin = 0, c0 = 0, cout = 0;      // c0: channels of the first source (decides the kernel, like csd_conv3d_block's C0)
  bool direct = false;
  size_t off = 0;                     // float offset in the packed buffer
};
enum Op3Kind { O3_TEMB, O3_LINEAR, O3_STEM, O3_GN, O3_CONV, O3_POOL, O3_UP, O3_TO_NCDHW };
struct Op3 {
  Op3Kind kind;
  size_t a = NONE, b = NONE, out = NONE;       // workspace float offsets: sources (b: the virtual concat's second), destination
  size_t ns = NONE, nh = NONE;                 // GroupNorm scale / shift: O3_GN writes them, O3_CONV reads them
  size_t res = NONE, partial = NONE;           // conv: residual; GroupNorm: its fp64 partial sums
  size_t temb_col = NONE;                      // conv: first column of its Dense_0 rows inside dense_all
  size_t pk_w = NONE, pk_b = NONE;             // linear over packed (concatenated) weights: float offsets in the packed buffer
  int slot = -1;                               // conv / stem: its Conv3Slot
  int pw = -1, pb = -1;                        // parameter indices: linear weight / bias, GroupNorm gamma / beta
  int C0 = 0, C1 = 0, Cout = 0, D = 0, H = 0, W = 0, K = 0, N = 0, act = 0;
  bool out_external = false;                   // writes the caller's output
  int cls = CSD_PROF_OTHER;
  double flops = 0, bytes = 0;
};
struct Plan3 {
  int B = 0;
  std::vector<Op3> ops;
  size_t ws_floats = 0;
  size_t dense_off = NONE;                     // [B, dense_total]: Dense_0(act(temb)) of every residual block
  int64_t launches = 0;
  double flops = 0, bytes = 0;
};

class Arena {
 public:
  Arena() {}
  explicit Arena(size_t base) : base_(base) {}       // a sub-arena: offsets start at `base` (a block reserved in the parent)
  size_t alloc(size_t nfloats) { return base_ + alloc_local(nfloats); }
  void release(size_t off) {
    if (off == NONE || off < base_ || off - base_ >= top_) return;      // (not ours: e.g. a slice of a parent tensor handed into a chunk)
    release_local(off - base_);
  }
  size_t peak() const { return peak_; }

 private:
  size_t base_ = 0;
  size_t alloc_local(size_t nfloats) {
    nfloats = (nfloats + 63) / 64 * 64;   // 256-byte granules
    // best fit in the free list
    int best = -1;
    for (int i = 0; i < (int)free_.size(); ++i)
      if (free_[i].second >= nfloats && (best < 0 || free_[i].second < free_[best].second)) best = i;
    size_t off;
    if (best >= 0) {
      off = free_[best].first;
      if (free_[best].second == nfloats) free_.erase(free_.begin() + best);
      else { free_[best].first += nfloats; free_[best].second -= nfloats; }
    } else {
      // extend the top (merge with a trailing free block if there is one)
      off = top_;
      for (int i = 0; i < (int)free_.size(); ++i)
        if (free_[i].first + free_[i].second == top_) { off = free_[i].first; free_.erase(free_.begin() + i); break; }
      top_ = off + nfloats;
    }
    live_[off] = nfloats;
    peak_ = std::max(peak_, top_);
    return off;
  }
  void release_local(size_t off) {
    auto it = live_.find(off);
    if (it == live_.end()) return;
    size_t n = it->second;
    live_.erase(it);
    // coalesce
    for (int i = 0; i < (int)free_.size();) {
      if (free_[i].first + free_[i].second == off) { off = free_[i].first; n += free_[i].second; free_.erase(free_.begin() + i); }
      else if (off + n == free_[i].first) { n += free_[i].second; free_.erase(free_.begin() + i); }
      else ++i;
    }
    free_.push_back({off, n});
  }
  std::vector<std::pair<size_t, size_t>> free_;
  std::map<size_t, size_t> live_;
  size_t top_ = 0, peak_ = 0;
};

struct Net {
  csd_unet_config cfg;
  std::vector<Module> mods;
  std::vector<Param> params;
  std::map<std::string, int> pindex;
  // packed layout
  std::vector<PackedConv> pconvs;
  std::map<std::string, int> pconv_by_name;          // "3.Conv_0", "13.qkv", "13.NIN_3", "2" ...
  struct Copy { int param; size_t off; };            // raw fp32 copies (linear, GN affine, dense)
  std::vector<Copy> copies;
  std::map<std::string, size_t> copy_off;
  std::map<int, size_t> pyr_fold_off;               // M_PYR module idx -> its folded 6x6 stride-2 weight (fir_pyramid.hip layout)
  size_t packed_floats = 0;
  size_t dense_all_off = 0, dense_all_bias_off = 0;  // concatenated Dense_0 of every res block
  int dense_total = 0;
  std::map<int, int> dense_col;                      // module idx -> first column
  bool packed_once = false;
  struct CopyDesc* copy_tab = nullptr;      // device table of pack_all's raw copies (+ its host copy and the event behind the upload)
  size_t copy_tab_cap = 0;
  std::vector<struct CopyDesc> copy_host;
  hipEvent_t copy_ev = nullptr;
  std::map<int, std::unique_ptr<Plan>> plans;
  // arch 2 (unet3d.h)
  std::vector<Conv3Slot> slots3;
  std::map<std::string, int> slot3_by_name;          // "3.Conv_0", "2" ...
  std::map<int, std::unique_ptr<Plan3>> plans3;
  int in_cpad = 8;
  // second stream for the ResnetBlock shortcut contraction (independent of the block's GroupNorm -> conv chain until the second conv
  // adds it): an HBM-bound pointwise kernel that fills the CUs a 3x3 launch leaves idle in its last round
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool side_ready() {
    if (side) return true;
    if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) { side = nullptr; return false; }
    if (hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) != hipSuccess) {
      (void)hipStreamDestroy(side);
      side = nullptr;
      return false;
    }
    return true;
  }
  // batch-chunk streams (build_plan: the <= 20^2 levels of a big batch run as CHUNKS concurrent sub-batches - their kernels are bound by
  // per-launch latency, not by throughput, and a sample's bits do not depend on the batch it runs in)
  static constexpr int MAX_CHUNKS = 4;
  hipStream_t cstream[MAX_CHUNKS] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_cfork = nullptr, ev_cjoin[MAX_CHUNKS] = {nullptr, nullptr, nullptr, nullptr};
  bool chunks_ready(int n_extra) {      // the first n_extra chunk streams exist (created on demand: a stream occupies a hardware queue)
    for (int k = 0; k < n_extra && k < MAX_CHUNKS; ++k) {
      if (cstream[k]) continue;
      if (hipStreamCreateWithFlags(&cstream[k], hipStreamNonBlocking) != hipSuccess) { cstream[k] = nullptr; return false; }
      if (hipEventCreateWithFlags(&ev_cjoin[k], hipEventDisableTiming) != hipSuccess) return false;
    }
    return ev_cfork != nullptr || hipEventCreateWithFlags(&ev_cfork, hipEventDisableTiming) == hipSuccess;
  }
  ~Net() {
    if (copy_ev) { (void)hipEventSynchronize(copy_ev); (void)hipEventDestroy(copy_ev); }
    if (copy_tab) (void)hipFree(copy_tab);
    for (int k = 0; k < MAX_CHUNKS; ++k) {
      if (cstream[k]) { (void)hipStreamSynchronize(cstream[k]); (void)hipStreamDestroy(cstream[k]); }
      if (ev_cjoin[k]) (void)hipEventDestroy(ev_cjoin[k]);
    }
    if (ev_cfork) (void)hipEventDestroy(ev_cfork);
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
  }

  int add_param(const std::string& name, std::initializer_list<int64_t> shape) {
    Param p;
    p.name = name;
    p.ndim = (int)shape.size();
    p.numel = 1;
    int i = 0;
    for (auto s : shape) { p.shape[i++] = s; p.numel *= s; }
    for (; i < 5; ++i) p.shape[i] = 1;
    params.push_back(p);
    pindex[name] = (int)params.size() - 1;
    return (int)params.size() - 1;
  }
  int P(const std::string& name) const {
    auto it = pindex.find(name);
    return it == pindex.end() ? -1 : it->second;
  }
};

static std::string mname(int idx, const char* sub) {
  char buf[96];
  if (sub && sub[0]) snprintf(buf, sizeof(buf), "all_modules.%d.%s", idx, sub);
  else snprintf(buf, sizeof(buf), "all_modules.%d", idx);
  return buf;
}

static const char* pyr_sub(const csd_unet_config& c, bool bias) {      // layerspp.Downsample: Conv2d_0 (fir) or Conv_0 (fir = False)
  return c.progressive_input == 2 ? (bias ? "Conv2d_0.bias" : "Conv2d_0.weight") : (bias ? "Conv_0.bias" : "Conv_0.weight");
}
static int ncsnpp_groups(int c) { return std::min(c / 4, 32); }     // layerspp.py:67,219,231; ncsnpp.py:200-233

static bool is_attn(const csd_unet_config& c, int res) {
  for (int i = 0; i < c.n_attn; ++i) if (c.attn_resolutions[i] == res) return true;
  return false;
}

// ---- module list + parameter table: mirrors DDPM.__init__ (models/ddpm.py:96-147) and, for arch 1, NCSNpp.__init__
// (models/ncsnpp.py:44-236) for resblock_type 'biggan', fir = True, progressive in {none, output_skip}, progressive_input in {none,
// input_skip, residual}, progressive_combine 'sum'.  One U-Net; the families differ in the Fourier entry, in how a level is left (M_DOWN /
// M_UP vs. BigGAN down / up blocks), in the input pyramid behind a downsample and in the output pyramid in front of an upsample ----
static int build_modules(Net& n) {
  const csd_unet_config& c = n.cfg;
  CSD_REQUIRE(c.arch == 0 || c.arch == 1, "unet: arch %d not supported (0 = DDPM family, 1 = NCSN++)", c.arch);
  const bool pp = c.arch == 1;
  if (!pp) {
    CSD_REQUIRE(c.n_levels >= 1 && c.n_levels <= CSD_MAX_LEVELS, "unet: bad n_levels %d", c.n_levels);
    CSD_REQUIRE(c.nf % 32 == 0, "unet: nf=%d must be a multiple of 32 (GroupNorm(32) + 32-wide MFMA tiles)", c.nf);
    CSD_REQUIRE(c.image_size % (1 << (c.n_levels - 1)) == 0, "unet: image_size %d not divisible by 2^%d",
                c.image_size, c.n_levels - 1);
    // (the input is assembled into in_cpad <= 32 channels: unet_layout.h; the head's NCHW store covers one 32-cout tile)
    CSD_REQUIRE(c.x_channels >= 1 && c.y_channels >= 0 && c.x_channels + c.y_channels <= CSD_MAX_IO_CHANNELS,
                "unet: x+y channels must be <= %d (got %d+%d)", CSD_MAX_IO_CHANNELS, c.x_channels, c.y_channels);
    CSD_REQUIRE(c.out_channels >= 1 && c.out_channels <= CSD_MAX_IO_CHANNELS, "unet: out_channels must be in 1 .. %d (got %d)",
                CSD_MAX_IO_CHANNELS, c.out_channels);
    CSD_REQUIRE(c.act >= CSD_ACT_SWISH && c.act <= CSD_ACT_ELU, "unet: bad activation id %d", c.act);
    CSD_REQUIRE(c.precision >= CSD_PREC_F32 && c.precision <= CSD_PREC_F16F8, "unet: bad precision id %d", c.precision);
  } else {
    CSD_REQUIRE(c.n_levels >= 1 && c.n_levels <= CSD_MAX_LEVELS, "ncsnpp: bad n_levels %d", c.n_levels);
    CSD_REQUIRE(c.nf % 8 == 0, "ncsnpp: nf=%d must be a multiple of 8", c.nf);
    CSD_REQUIRE(c.image_size % (1 << (c.n_levels - 1)) == 0, "ncsnpp: image_size %d not divisible by 2^%d", c.image_size,
                c.n_levels - 1);
    // (as for the DDPM family: the input is assembled into in_cpad <= 32 channels; the output pyramid and the head store one 32-cout tile.
    // More than 8 channels are provided for the paired networks - ncsnpp_paired, ncsnpp_2xSR: y_channels > 0; the unconditional network
    // keeps its limit of 8 and its message)
    CSD_REQUIRE(c.x_channels >= 1 && c.y_channels >= 0, "ncsnpp: bad channel counts %d+%d", c.x_channels, c.y_channels);
    if (c.y_channels > 0)
      CSD_REQUIRE(c.x_channels + c.y_channels <= CSD_MAX_IO_CHANNELS, "ncsnpp: x+y channels must be <= %d (got %d+%d)", CSD_MAX_IO_CHANNELS,
                  c.x_channels, c.y_channels);
    else
      CSD_REQUIRE(c.x_channels <= 8, "ncsnpp: x+y channels must be <= 8 for a network without a condition (got %d; the paired networks "
                  "take up to %d)", c.x_channels, CSD_MAX_IO_CHANNELS);
    CSD_REQUIRE(c.out_channels == c.x_channels + c.y_channels, "ncsnpp: the network maps its %d input channels to as many outputs",
                c.x_channels + c.y_channels);
    CSD_REQUIRE(c.act >= CSD_ACT_SWISH && c.act <= CSD_ACT_ELU, "ncsnpp: bad activation id %d", c.act);
    CSD_REQUIRE(c.precision >= CSD_PREC_F32 && c.precision <= CSD_PREC_F16F8, "ncsnpp: bad precision id %d", c.precision);
    CSD_REQUIRE(c.conditional, "ncsnpp: only time-conditional networks are supported");
    CSD_REQUIRE(c.progressive >= 0 && c.progressive <= 1, "ncsnpp: progressive id %d is not supported (output 'residual' is not)",
                c.progressive);
    CSD_REQUIRE(c.progressive_input >= 0 && c.progressive_input <= 3, "ncsnpp: bad progressive_input id %d", c.progressive_input);
    CSD_REQUIRE(c.n_fir == 4, "ncsnpp: a 4-tap FIR kernel is required (got %d taps)", c.n_fir);
  }
  if (c.x_squeeze) {      // the 2x super-resolution networks: x is the image [B, x_channels / 4, 2S, 2S] (include/csd.h)
    CSD_REQUIRE(c.x_squeeze == 1, "unet: x_squeeze must be 0 or 1 (got %d)", c.x_squeeze);
    CSD_REQUIRE(c.x_channels % 4 == 0, "unet: x_squeeze needs x_channels %% 4 == 0 (got x_channels = %d)", c.x_channels);
    CSD_REQUIRE(c.image_size <= 1024, "unet: x_squeeze is provided up to image_size 1024 (got %d)", c.image_size);
    CSD_REQUIRE(c.out_channels >= c.x_channels, "unet: x_squeeze needs out_channels >= x_channels (got %d < %d)", c.out_channels,
                c.x_channels);
  }
  const int nf = c.nf, channels = c.x_channels + c.y_channels, last = c.n_levels - 1;
  const bool fourier = pp && c.embedding_type == 1, pyr_out = pp && c.progressive == 1;
  const int pin = pp ? c.progressive_input : 0;
  auto add = [&](ModKind k, Role role, int level, int cin, int cout) -> Module& {
    Module m;
    m.kind = k; m.idx = (int)n.mods.size(); m.role = role; m.level = level; m.cin = cin; m.cout = cout;
    m.side = m.out_side = c.image_size >> level;
    n.mods.push_back(m);
    return n.mods.back();
  };
  if (fourier) add(M_FOURIER, R_EMB_FOURIER, 0, nf, 2 * nf);
  if (c.conditional) {
    add(M_LINEAR, R_EMB_LINEAR0, 0, fourier ? 2 * nf : nf, 4 * nf);
    add(M_LINEAR, R_EMB_LINEAR1, 0, 4 * nf, 4 * nf);
  }
  add(M_CONV3, R_STEM, 0, channels, nf).push = true;
  std::vector<int> hs_c{nf};      // channels on the skip stack
  int in_ch = nf, pyr_ch = channels;
  for (int l = 0; l <= last; ++l) {
    for (int b = 0; b < c.num_res_blocks; ++b) {
      add(M_RES, R_DOWN_BLOCK, l, in_ch, nf * c.ch_mult[l]);
      in_ch = nf * c.ch_mult[l];
      if (is_attn(c, c.image_size >> l)) add(M_ATTN, R_ATTN, l, in_ch, in_ch);
      n.mods.back().push = true;
      hs_c.push_back(in_ch);
    }
    if (l != last) {
      Module& d = add(pp ? M_RES : M_DOWN, R_DOWNSAMPLE, l, in_ch, in_ch);
      d.down = pp ? 1 : 0;
      d.out_side = d.side / 2;
      if (pin == 1) add(M_COMBINE, R_COMBINE, l + 1, channels, in_ch);
      if (pin >= 2) {                                                  // ncsnpp.py:171-173
        add(M_PYR, R_PYR_DOWN, l, pyr_ch, in_ch).out_side = (c.image_size >> l) / 2;
        pyr_ch = in_ch;
      }
      n.mods.back().push = true;
      hs_c.push_back(in_ch);
    }
  }
  add(M_RES, R_MID_RES_IN, last, in_ch, in_ch);
  add(M_ATTN, R_MID_ATTN, last, in_ch, in_ch);
  add(M_RES, R_MID_RES_OUT, last, in_ch, in_ch);
  for (int l = last; l >= 0; --l) {
    for (int b = 0; b < c.num_res_blocks + 1; ++b) {
      add(M_RES, R_UP_BLOCK, l, in_ch + hs_c.back(), nf * c.ch_mult[l]).skip = hs_c.back();
      hs_c.pop_back();
      in_ch = nf * c.ch_mult[l];
    }
    if (is_attn(c, c.image_size >> l)) add(M_ATTN, R_ATTN, l, in_ch, in_ch);
    n.mods.back().last_up = true;
    if (pyr_out) { add(M_GN, R_PYR_GN, l, in_ch, in_ch); add(M_CONV3, R_PYR_CONV, l, in_ch, c.out_channels); }
    if (l != 0) {
      Module& u = add(pp ? M_RES : M_UP, R_UPSAMPLE, l, in_ch, in_ch);
      u.up = pp ? 1 : 0;
      u.out_side = u.side * 2;
    }
  }
  if (!pyr_out) { add(M_GN, R_HEAD_GN, 0, in_ch, in_ch); add(M_CONV3, R_HEAD_CONV, 0, in_ch, c.out_channels); }

  // parameter table in state_dict order
  const int temb = 4 * nf;
  for (auto& m : n.mods) {
    switch (m.kind) {
      case M_FOURIER:
        n.add_param(mname(m.idx, "W"), {m.cin});
        break;
      case M_LINEAR:
        n.add_param(mname(m.idx, "weight"), {m.cout, m.cin});
        n.add_param(mname(m.idx, "bias"), {m.cout});
        break;
      case M_CONV3:
        n.add_param(mname(m.idx, "weight"), {m.cout, m.cin, 3, 3});
        n.add_param(mname(m.idx, "bias"), {m.cout});
        break;
      case M_GN:
        n.add_param(mname(m.idx, "weight"), {m.cin});
        n.add_param(mname(m.idx, "bias"), {m.cin});
        break;
      case M_DOWN:
      case M_UP:
        if (c.resamp_with_conv) {
          n.add_param(mname(m.idx, "Conv_0.weight"), {m.cin, m.cin, 3, 3});
          n.add_param(mname(m.idx, "Conv_0.bias"), {m.cin});
        }
        break;
      case M_COMBINE:
        n.add_param(mname(m.idx, "Conv_0.weight"), {m.cout, m.cin, 1, 1});
        n.add_param(mname(m.idx, "Conv_0.bias"), {m.cout});
        break;
      case M_PYR:
        n.add_param(mname(m.idx, pyr_sub(c, false)), {m.cout, m.cin, 3, 3});
        n.add_param(mname(m.idx, pyr_sub(c, true)), {m.cout});
        break;
      case M_ATTN:
        n.add_param(mname(m.idx, "GroupNorm_0.weight"), {m.cin});
        n.add_param(mname(m.idx, "GroupNorm_0.bias"), {m.cin});
        for (int j = 0; j < 4; ++j) {
          char w[32], b[32];
          snprintf(w, sizeof(w), "NIN_%d.W", j);
          snprintf(b, sizeof(b), "NIN_%d.b", j);
          n.add_param(mname(m.idx, w), {m.cin, m.cin});
          n.add_param(mname(m.idx, b), {m.cin});
        }
        break;
      case M_RES:
        n.add_param(mname(m.idx, "GroupNorm_0.weight"), {m.cin});
        n.add_param(mname(m.idx, "GroupNorm_0.bias"), {m.cin});
        n.add_param(mname(m.idx, "Conv_0.weight"), {m.cout, m.cin, 3, 3});
        n.add_param(mname(m.idx, "Conv_0.bias"), {m.cout});
        if (c.conditional) {
          n.add_param(mname(m.idx, "Dense_0.weight"), {m.cout, temb});
          n.add_param(mname(m.idx, "Dense_0.bias"), {m.cout});
        }
        n.add_param(mname(m.idx, "GroupNorm_1.weight"), {m.cout});
        n.add_param(mname(m.idx, "GroupNorm_1.bias"), {m.cout});
        n.add_param(mname(m.idx, "Conv_1.weight"), {m.cout, m.cout, 3, 3});
        n.add_param(mname(m.idx, "Conv_1.bias"), {m.cout});
        if (m.cin != m.cout || m.up || m.down) {      // shortcut: NIN_0 (W [in, out]) / NCSN++ Conv_2 (1x1, OIHW)
          if (pp) {
            n.add_param(mname(m.idx, "Conv_2.weight"), {m.cout, m.cin, 1, 1});
            n.add_param(mname(m.idx, "Conv_2.bias"), {m.cout});
          } else {
            n.add_param(mname(m.idx, "NIN_0.W"), {m.cin, m.cout});
            n.add_param(mname(m.idx, "NIN_0.b"), {m.cout});
          }
        }
        break;
    }
  }
  return CSD_OK;
}

// floats of one sample of `out` / d_out / the sampler's net_out: out_channels planes, or with y_scale = K (arch 0 / 1) the x block at
// S x S followed by the other channels downsampled to S / K (include/csd.h)
static inline size_t out_sample_elems(const csd_unet_config& c) {
  const size_t hw = c.arch == 2 ? (size_t)c.vol[0] * c.vol[1] * c.vol[2] : (size_t)c.image_size * c.image_size;
  if (!c.y_scale) return (size_t)c.out_channels * hw;
  return (size_t)c.x_channels * hw + (size_t)(c.out_channels - c.x_channels) * (hw / ((size_t)c.y_scale * c.y_scale));
}

}  // namespace csd

#include "unet_layout.h"
#include "unet_plan.h"
#include "unet_run.h"
#include "unet3d.h"

// =====================================================================================================
// C ABI
// =====================================================================================================
using namespace csd;

struct csd_unet {
  Net net;
};

#include "train_graph.h"
#include "train_graph3d.h"
#include "plan_digest.h"

extern "C" int csd_profile_select(unsigned class_mask, int step_stride) {
  g_prof.mask = class_mask;
  g_prof.step_stride = step_stride > 0 ? step_stride : 1;
  g_prof.step_on = true;
  return CSD_OK;
}

extern "C" int csd_profile_start(void) {
  g_prof.on = true;
  g_prof.recs.clear();
  g_prof.used = 0;
  return CSD_OK;
}

extern "C" int csd_profile_stop(int n_classes, double* ms, int64_t* launches, double* flops, double* bytes) {
  return csd_profile_stop_ex(n_classes, ms, launches, flops, bytes, nullptr);
}

extern "C" int csd_profile_stop_ex(int n_classes, double* ms, int64_t* launches, double* flops, double* bytes, double* alg_bytes) {
  g_prof.on = false;
  CSD_REQUIRE(n_classes >= CSD_PROF_NUM_CLASSES && ms && launches && flops && bytes, "profile_stop: bad arguments");
  for (int i = 0; i < n_classes; ++i) { ms[i] = 0; launches[i] = 0; flops[i] = 0; bytes[i] = 0; if (alg_bytes) alg_bytes[i] = 0; }
  if (g_prof.recs.empty()) return CSD_OK;
  for (auto& r : g_prof.recs) CSD_CHECK_HIP(hipEventSynchronize(r.b));      // (the records may sit on several streams: batch chunks)
  for (auto& r : g_prof.recs) {
    float t = 0.f;
    CSD_CHECK_HIP(hipEventElapsedTime(&t, r.a, r.b));
    ms[r.cls] += t;
    launches[r.cls] += 1;
    flops[r.cls] += r.flops;
    bytes[r.cls] += r.bytes;
    if (alg_bytes) alg_bytes[r.cls] += r.abytes;
  }
  g_prof.recs.clear();
  g_prof.used = 0;
  return CSD_OK;
}

extern "C" const char* csd_version(void) { return "csd-hip 0.1 (gfx950)"; }
extern "C" const char* csd_last_error(void) { return get_error(); }

extern "C" size_t csd_unet_config_size(void) { return sizeof(csd_unet_config); }

extern "C" int csd_unet_create(const csd_unet_config* cfg, csd_unet** out) {
  CSD_REQUIRE(cfg && out, "unet_create: null argument");
  std::unique_ptr<csd_unet> h(new csd_unet());
  h->net.cfg = *cfg;
  CSD_REQUIRE(!cfg->x_squeeze || cfg->arch == 0 || cfg->arch == 1,
              "unet_create: x_squeeze = %d is provided for arch 0 / 1, not for the 3-D networks (arch %d)", cfg->x_squeeze, cfg->arch);
  CSD_REQUIRE(!cfg->x_squeeze || cfg->arch != 1 || cfg->y_channels > 0,
              "unet_create: x_squeeze = %d on arch 1 is provided for the paired networks (ncsnpp_2xSR: y_channels > 0), not without a condition",
              cfg->x_squeeze);
  if (cfg->y_scale) {      // the direct Kx super-resolution networks: y is [B, y_channels, S / K, S / K] (include/csd.h)
    CSD_REQUIRE(cfg->y_scale >= 2, "unet_create: y_scale must be 0 or >= 2 (got %d)", cfg->y_scale);
    CSD_REQUIRE(cfg->arch == 0 || cfg->arch == 1, "unet_create: y_scale = %d is provided for arch 0 / 1, not for the 3-D networks (arch %d)",
                cfg->y_scale, cfg->arch);
    CSD_REQUIRE(!cfg->x_squeeze, "unet_create: y_scale = %d and x_squeeze = %d exclude each other", cfg->y_scale, cfg->x_squeeze);
    CSD_REQUIRE(cfg->y_channels > 0, "unet_create: y_scale = %d needs a conditioning image (y_channels = %d)", cfg->y_scale, cfg->y_channels);
    CSD_REQUIRE(cfg->image_size > 0 && cfg->image_size % cfg->y_scale == 0, "unet_create: y_scale = %d must divide image_size = %d",
                cfg->y_scale, cfg->image_size);
    CSD_REQUIRE(cfg->x_channels + cfg->y_channels <= 8, "unet_create: y_scale = %d is provided up to 8 assembled channels (got %d + %d)",
                cfg->y_scale, cfg->x_channels, cfg->y_channels);
    CSD_REQUIRE(cfg->out_channels >= cfg->x_channels, "unet_create: y_scale = %d needs out_channels >= x_channels (got %d < %d)",
                cfg->y_scale, cfg->out_channels, cfg->x_channels);
  }
  int rc = cfg->arch == 2 ? build_modules3d(h->net) : build_modules(h->net);
  if (rc) return rc;
  rc = cfg->arch == 2 ? build_packed_layout3d(h->net) : build_packed_layout(h->net);
  if (rc) return rc;
  *out = h.release();
  return CSD_OK;
}

extern "C" void csd_unet_destroy(csd_unet* net) {
  if (net) {
    train_state_erase(&net->net);
  }
  delete net;
}

extern "C" int csd_unet_num_params(const csd_unet* net) { return net ? (int)net->net.params.size() : 0; }

extern "C" int csd_unet_param_info(const csd_unet* net, int index, const char** name, int* ndim, int64_t shape[]) {
  CSD_REQUIRE(net && index >= 0 && index < (int)net->net.params.size(), "param_info: index %d out of range", index);
  const Param& p = net->net.params[index];
  if (name) *name = p.name.c_str();
  if (ndim) *ndim = p.ndim;
  if (shape) for (int i = 0; i < (is3d(net->net) ? 5 : 4); ++i) shape[i] = p.shape[i];
  return CSD_OK;
}

extern "C" int csd_unet_set_param(csd_unet* net, const char* name, const void* dev_ptr, int64_t numel) {
  CSD_REQUIRE(net && name && dev_ptr, "set_param: null argument");
  const int i = net->net.P(name);
  if (i < 0) { set_error("set_param: unknown parameter '%s'", name); return CSD_ERR_NOT_FOUND; }
  Param& p = net->net.params[i];
  CSD_REQUIRE(p.numel == numel, "set_param: '%s' expects %lld elements, got %lld", name, (long long)p.numel,
              (long long)numel);
  CSD_REQUIRE((reinterpret_cast<uintptr_t>(dev_ptr) & 3) == 0, "set_param: '%s' is not 4-byte aligned", name);
  p.ptr = static_cast<const float*>(dev_ptr);
  return CSD_OK;
}

extern "C" size_t csd_unet_packed_bytes(const csd_unet* net) { return net ? net->net.packed_floats * sizeof(float) : 0; }

extern "C" int csd_unet_pack(csd_unet* net, void* packed, void* stream) {
  CSD_REQUIRE(net && packed, "pack: null argument");
  CSD_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 255) == 0, "pack: packed buffer must be 256-byte aligned");
  if (is3d(net->net)) return pack_all3d(net->net, static_cast<float*>(packed), (hipStream_t)stream);
  return pack_all(net->net, static_cast<float*>(packed), (hipStream_t)stream);
}

extern "C" size_t csd_unet_workspace_bytes(csd_unet* net, int B) {
  if (!net) return 0;
  if (is3d(net->net)) {
    Plan3* p3 = nullptr;
    return build_plan3d(net->net, B, &p3) ? 0 : p3->ws_floats * sizeof(float);
  }
  Plan* pl = nullptr;
  if (build_plan(net->net, B, &pl)) return 0;
  return pl->ws_floats * sizeof(float);
}

extern "C" int csd_unet_stats(csd_unet* net, int B, int64_t* launches, double* flops, double* bytes) {
  CSD_REQUIRE(net, "stats: null handle");
  if (is3d(net->net)) {
    Plan3* p3 = nullptr;
    const int rc3 = build_plan3d(net->net, B, &p3);
    if (rc3) return rc3;
    if (launches) *launches = p3->launches;
    if (flops) *flops = p3->flops;
    if (bytes) *bytes = p3->bytes;
    return CSD_OK;
  }
  Plan* pl = nullptr;
  int rc = build_plan(net->net, B, &pl);
  if (rc) return rc;
  if (launches) *launches = pl->launches;
  if (flops) *flops = pl->flops;
  if (bytes) *bytes = pl->bytes;
  return CSD_OK;
}

// one validated "evaluate the network at batch B" of a handle: the 2-D plan (arch 0 / 1) or the 3-D plan (arch 2)
struct Evaluator {
  Net* n = nullptr;
  Plan* pl = nullptr;
  Plan3* p3 = nullptr;
  int run(const float* pk, float* ws, const float* x, const float* y, const float* labels, float* out, const float* y_noise, float y_sigma,
          hipStream_t s) const {
    if (p3) return run_plan3d(*n, *p3, pk, ws, x, y, labels, out, y_noise, y_sigma, s);
    return run_plan(*n, *pl, pk, ws, x, y, labels, out, y_noise, y_sigma, s);
  }
};

static int check_forward_args(csd_unet* net, const void* packed, void* ws, size_t ws_bytes, int B, Evaluator* ev) {
  CSD_REQUIRE(net && packed && ws, "forward: null argument");
  if (!net->net.packed_once) { set_error("forward: csd_unet_pack has not been called"); return CSD_ERR_STATE; }
  CSD_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "forward: workspace must be 256-byte aligned");
  ev->n = &net->net;
  int rc = is3d(net->net) ? build_plan3d(net->net, B, &ev->p3) : build_plan(net->net, B, &ev->pl);
  if (rc) return rc;
  const size_t need = (ev->p3 ? ev->p3->ws_floats : ev->pl->ws_floats) * sizeof(float);
  if (ws_bytes < need) {
    set_error("forward: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    return CSD_ERR_WORKSPACE;
  }
  return CSD_OK;
}

extern "C" int csd_unet_forward(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes,
                                const float* x, const float* y, const float* labels, float* out, int B,
                                const float* y_noise, float y_sigma, void* stream) {
  Evaluator ev;
  int rc = check_forward_args(net, packed, workspace, workspace_bytes, B, &ev);
  if (rc) return rc;
  CSD_REQUIRE(x && out, "forward: null x/out");
  CSD_REQUIRE((net->net.cfg.y_channels == 0) == (y == nullptr), "forward: y must be given iff y_channels > 0");
  CSD_REQUIRE(!net->net.cfg.conditional || labels, "forward: labels required for a conditional network");
  return ev.run(static_cast<const float*>(packed), static_cast<float*>(workspace), x, y, labels, out, y_noise, y_sigma,
                (hipStream_t)stream);
}

// the fused PC sampler, its draw schedule and the cascade (needs Evaluator and check_forward_args above)
#include "pc_loop.h"
