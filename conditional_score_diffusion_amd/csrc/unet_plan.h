// unet_plan.h - the inference plan of a network for one batch size: a flat list of kernel launches with every workspace offset fixed
// (Builder: one method per module kind, step() for one module of Net::mods with the walk's state in Builder::w; build_plan: one walk
// over Net::mods, a batch chunk through a Builder of its own).  Included by unet.hip.
#pragma once

namespace csd {

// ---- plan for batch B ---------------------------------------------------------------------------
struct Builder {
  Net& n;
  Plan& pl;
  Arena ar;
  int B;
  size_t gn_partial = NONE, nscale = NONE, nshift = NONE;   // shared scratch
  size_t dense_all = NONE;
  int rc = CSD_OK;
  // tensors whose producing conv left per-tile GroupNorm partials behind: workspace offset -> (partials, tiles per sample)
  struct TileStats { size_t off; int tpi; };
  std::map<size_t, TileStats> tile_stats;
  // what gn() planned: nothing (no GroupNorm in front of the consumer), a finalize over tile partials, or the streaming statistics /
  // finalize pair pl.ops[stats_op], pl.ops[stats_op + 1].  Either way the scale / shift are in nscale / nshift behind it
  struct Norm {
    enum Kind { ABSENT, TILES, STREAMED } kind = ABSENT;
    size_t stats_op = NONE;
    explicit operator bool() const { return kind != ABSENT; }
  };
  // what step() carries from one module of Net::mods to the next
  struct Walk {
    std::vector<size_t> hs;             // skip stack
    size_t h = NONE;                    // the current tensor
    bool h_on_stack = true;             // ... is hs.back(): its consumer must not release it
    size_t as_out = NONE;               // the assembled input (NONE: the fused first layer reads x, y itself)
    size_t pyr_in = NONE;               // NCSN++ input pyramid (level 0: the in_cpad-channel padded NHWC input)
    int pyr_side = 0, pyr_pix = 0;
    size_t pyr = NONE, pyr_up = NONE;   // NCSN++ output pyramid [B, side, side, channels] of the level below / its FIR upsampling
    Norm out_norm;                      // the GroupNorm R_PYR_GN / R_HEAD_GN planned for the conv behind it
  } w;

  Builder(Net& n_, Plan& p_, int B_, Arena ar_ = Arena()) : n(n_), pl(p_), ar(ar_), B(B_) {}

  // every workspace allocation goes through here: a new tensor at an offset invalidates what was known about the old one
  size_t alloc_(size_t nfloats) {
    const size_t off = ar.alloc(nfloats);
    tile_stats.erase(off);
    return off;
  }

  // every op enters the plan here (OP_FORK / OP_JOIN: no launch of their own)
  void emit(const Op& o, int launches = 1) { pl.ops.push_back(o); pl.launches += launches; }
  // algorithmic flops / bytes of the op emit() has just taken
  void count(double flops, double bytes) {
    pl.flops += flops; pl.bytes += bytes;
    pl.ops.back().flops = flops; pl.ops.back().bytes = bytes;
  }

  // GroupNorm statistics of (src0|src1) -> nscale/nshift
  Norm gn(size_t src0, size_t src1, int c0, int c1, int hw, const std::string& gname, const std::string& bname) {
    const int G = n.cfg.arch == 1 ? ncsnpp_groups(c0 + c1) : 32;
    if (src1 != NONE && (tile_stats.count(src0) != 0) != (tile_stats.count(src1) != 0)) {
      // a concatenated input of which ONE half carries epilogue partials (the skip tensor next to an Upsample output): the streaming pass
      // reads only the other half and leaves per-channel partials in the same layout (it used to re-read both: 1.26 GB at 160^2 x 192)
      const bool first = tile_stats.count(src0) == 0;
      const size_t src = first ? src0 : src1;
      const int cs = first ? c0 : c1;
      Op s;
      s.kind = OP_GN_STATS;
      if (gn_plan(&s.gp, B, hw, cs, 0, 1)) { rc = CSD_ERR_INVALID; return Norm{Norm::TILES}; }
      s.src0 = src; s.per_channel = true;
      s.stats = alloc_((size_t)B * s.gp.nchunk * cs * 2 * 2);      // doubles; never released (small)
      s.cls = CSD_PROF_GN_STATS; s.bytes = (double)B * hw * cs * 4;
      emit(s);
      tile_stats[src] = TileStats{s.stats, s.gp.nchunk};
    }
    const auto t0 = tile_stats.find(src0);
    const auto t1 = src1 == NONE ? tile_stats.end() : tile_stats.find(src1);
    if (t0 != tile_stats.end() && (src1 == NONE || t1 != tile_stats.end())) {
      // both sources were written by convs that accumulated the statistics in their epilogue: no pass over the tensor
      Op f;
      f.kind = OP_GN_FINAL_TILES;
      f.stats = t0->second.off; f.tiles0 = t0->second.tpi; f.C0 = c0;
      f.stats1 = src1 == NONE ? NONE : t1->second.off; f.tiles1 = src1 == NONE ? 0 : t1->second.tpi; f.C1 = c1;
      f.hw = hw;
      f.gp.G = G;
      f.pk_w = n.copy_off.at(gname); f.pk_b = n.copy_off.at(bname);
      f.nscale = nscale; f.nshift = nshift;
      f.cls = CSD_PROF_GN_FINAL;
      emit(f);
      pl.bytes += 2.0 * B * hw * (c0 + c1) * 4;   // SURVEY 8(d) algorithmic bytes are those of the unfused op
      return Norm{Norm::TILES};
    }
    Op s;
    s.kind = OP_GN_STATS;
    if (gn_plan(&s.gp, B, hw, c0, c1, G)) { rc = CSD_ERR_INVALID; return Norm{Norm::TILES}; }
    s.src0 = src0; s.src1 = src1; s.stats = gn_partial;
    s.cls = CSD_PROF_GN_STATS; s.bytes = (double)B * hw * (c0 + c1) * 4;
    const size_t stats_op = pl.ops.size();
    emit(s);
    Op f;
    f.kind = OP_GN_FINAL;
    f.gp = s.gp;
    f.stats = gn_partial; f.pk_w = n.copy_off.at(gname); f.pk_b = n.copy_off.at(bname);
    f.nscale = nscale; f.nshift = nshift;
    f.cls = CSD_PROF_GN_FINAL;
    emit(f);
    pl.bytes += 2.0 * B * hw * (c0 + c1) * 4;   // GroupNorm reads + writes its tensor
    return Norm{Norm::STREAMED, stats_op};
  }

  // the arguments of conv() beside the layer's key
  struct ConvIn {
    size_t src0 = NONE, src1 = NONE;      // sources (src1: the second of a virtual concat)
    int ih = 0, iw = 0;                   // extent of the source map
    int stride = 1, pad = 0, up = 0;
    Norm norm;                            // reads act(GroupNorm(sources)): what gn() returned for them
    int act = CSD_ACT_NONE;
    size_t residual = NONE;               // added by the epilogue
    size_t temb_col = NONE;               // first column of the block's Dense_0 rows inside dense_all
    bool external_nchw = false;           // writes the caller's NCHW output
    int real_cin = -1;                    // input channels the flop count takes (a zero-padded input)
    float out_scale = 1.f;                // the epilogue's factor (NCSN++ skip_rescale: (x + h)/sqrt(2))
    size_t out_to = NONE;                 // writes here instead of allocating (a batch chunk's slice of the region's output tensor)
  };

  int fail(const char* what) { set_error("%s", what); rc = CSD_ERR_INVALID; return rc; }

  // tap-partial form (conv_pw16.hip): pointwise contraction of act(GN(x)) to 9 * cout partial channels, then the 9-tap gather
  size_t conv_taps(const PackedConv& pc, const ConvIn& in) {
    const int ih = in.ih, iw = in.iw;
    if (!in.norm || in.src1 != NONE || in.stride != 1 || in.up || in.pad != 1 || in.temb_col != NONE || in.out_to != NONE) {
      fail("tap-partial conv on an unsupported layer"); return NONE;      // (out_to: the head is never inside a chunk region)
    }
    if (in.act != CSD_ACT_SWISH) {      // (pw16_kernel's prologue knows SiLU only: build_packed_layout keeps every other head off this form)
      set_error("tap-partial conv: activation %d is not supported (SiLU only)", in.act); rc = CSD_ERR_INVALID; return NONE;
    }
    Op o;
    o.kind = OP_CONV;
    o.cp = pc.proto;
    o.cp.B = B; o.cp.IH = o.cp.OH = ih; o.cp.IW = o.cp.OW = iw;
    o.cp.stride = 1; o.cp.pad = 0; o.cp.up = 0;
    o.ns = pc.ns; o.kernel = pc.kernel;
    o.src0 = in.src0; o.pk_w = pc.w_off;          // (the bias joins in the gather)
    o.nscale = nscale; o.nshift = nshift;
    o.act = in.act;
    o.temb_base = dense_all; o.temb_stride = n.dense_total;
    const size_t part = alloc_((size_t)B * ih * iw * o.cp.Cout);
    o.out = part;
    o.cls = CSD_PROF_CONV1X1;                  // (profiler classes follow the kernels: a pointwise contraction + a small gather)
    emit(o);
    const size_t out_elems = (size_t)B * ih * iw * pc.tap_cout;
    count(2.0 * out_elems * o.cp.C0 * 9, ((double)B * ih * iw * o.cp.C0 + (double)out_elems) * 4);
    pl.ops.back().bytes = (double)B * ih * iw * (o.cp.C0 + o.cp.Cout) * 4.0;
    Op g;
    g.kind = OP_TAPSUM;
    g.src0 = part; g.pk_b = pc.b_off; g.res = in.residual;
    g.H = ih; g.W = iw; g.Cout = pc.tap_cout;
    g.out_scale = in.out_scale;
    g.out_external = in.external_nchw ? 1 : 0;
    g.out = in.external_nchw ? NONE : alloc_(out_elems);
    g.cls = CSD_PROF_OTHER;
    g.bytes = (double)B * ih * iw * (o.cp.Cout + pc.tap_cout) * 4.0;
    emit(g);
    ar.release(part);
    return g.out;
  }

  // conv(), the geometry: the layer on its kernel, validated and tiled by that kernel's *_plan_tiles.  false: failed (rc is set).
  // *loader_norm: the tuning-only CSD_FUSED_NORM form - GroupNorm affine + activation applied by the loader / consumer kernel's loader
  // wave (no gn_apply16 pass).  (The switch also reaches a layer packed for ConvKernel::FUSED, as it always has: an experiment, not a
  // product path)
  bool conv_geometry(const PackedConv& pc, const ConvIn& in, ConvPlan& cp, bool* loader_norm) {
    const int stride = in.stride, up = in.up;
    const bool norm = (bool)in.norm, external_nchw = in.external_nchw;
    cp = pc.proto;
    cp.B = B; cp.IH = in.ih; cp.IW = in.iw;
    cp.stride = stride; cp.pad = in.pad; cp.up = up;
    cp.OH = (in.ih << up) / stride; cp.OW = (in.iw << up) / stride;
    *loader_norm = false;
    if ((pc.kernel == ConvKernel::F16_LC || pc.kernel == ConvKernel::FUSED) && norm && stride == 1 && !up && cp.C0 % 32 == 0 &&
        cp.C1 % 32 == 0 && !CSD_TUNE_ENV("CSD_NO_LC") && CSD_TUNE_ENV("CSD_FUSED_NORM")) {
      ConvPlan trial = cp;
      if (conv16_plan_tiles(&trial, pc.ns, 2, true) == CSD_OK && trial.LC && trial.OH % trial.TH == 0) {
        *loader_norm = true;
        cp = trial;
      }
    }
    if (!*loader_norm) switch (pc.kernel) {
      case ConvKernel::FUSED:
        if (external_nchw || stride != 1 || up) { fail("fused-prologue conv on an unsupported layer"); return false; }
        if (convff_plan_tiles(&cp, pc.ns)) { rc = CSD_ERR_INVALID; return false; }
        break;
      case ConvKernel::QUAD: case ConvKernel::QUAD_UP4:
        if (external_nchw || (!norm && cp.C1 != 0) || (stride == 2 && (norm || up))) { fail("quad fp16 conv on an unsupported layer"); return false; }
        cp.C0 = cp.C0 + cp.C1; cp.C1 = 0;
        if (pc.kernel == ConvKernel::QUAD_UP4) {
          if (!up || stride != 1) { fail("phase-decomposed Upsample packed for a layer that is not one"); return false; }
          cp.up = 2;
        }
        if (conv16q_plan_tiles(&cp, pc.ns)) { rc = CSD_ERR_INVALID; return false; }
        break;
      case ConvKernel::PW16:
        if (in.act != CSD_ACT_NONE || in.temb_col != NONE || external_nchw) { fail("pointwise fp16 layer with act/temb/NCHW"); return false; }
        break;
      case ConvKernel::F16_LC: {
        const int kcs = norm ? conv16_kcs(pc.ns, cp.C0 + cp.C1) : 1;    // fp16-source convs stage in bursts
        // (x_squeeze: the head's scattered NCHW store lives in conv_f16_kernel.h / conv_f32.hip; the loader / consumer schedule keeps its code)
        if (conv16_plan_tiles(&cp, pc.ns, kcs, kcs > 1 && !CSD_TUNE_ENV("CSD_NO_LC") && !(external_nchw && n.cfg.x_squeeze))) {
          rc = CSD_ERR_INVALID; return false;
        }
        break;
      }
      case ConvKernel::F32:
        if (conv_plan_tiles(&cp)) { rc = CSD_ERR_INVALID; return false; }
        break;
      case ConvKernel::PW16_TAPS: case ConvKernel::STEM:      // (conv_taps / Builder::stem)
        fail("conv: a layer packed for another builder"); return false;
    }
    // the packed layout depends on KC only (not on NT / tile shape)
    if (cp.KC != pc.proto.KC) { fail("conv plan/pack mismatch"); return false; }
    return true;
  }

  // conv(), the operand form: o.src_form, o.src0 / src1 and, where the kernel itself normalises, o.nscale / nshift
  void conv_operand(const PackedConv& pc, const ConvIn& in, bool loader_norm, Op& o) {
    const bool norm = (bool)in.norm, quad = is_quad(pc.kernel);
    o.src0 = in.src0; o.src1 = in.src1;
    o.nscale = norm ? nscale : NONE; o.nshift = norm ? nshift : NONE;
    // a quad-schedule conv WITHOUT a GroupNorm in front (Downsample / Upsample, the FIR-resampled Conv_0 of NCSN++) in the full split reads
    // its fp32 source directly: the split happens in the kernel's staging burst (no plane write / read)
    if (quad && !norm && pc.ns == 2 && o.cp.C1 == 0 && (o.cp.NT == 3 || o.cp.NT == 4) && !CSD_TUNE_ENV("CSD_NO_Q_RAW")) {
      o.src_form = ConvSrc::SPLIT_STAGING;
      return;
    }
    if (!((pc.kernel == ConvKernel::F16_LC && norm) || quad) || loader_norm) return;      // fp32 sources
    // fp16 kernel: normalise + activate + split ONCE per element into fp16 planes, conv copies them
    // (a quad-schedule conv without a GroupNorm - Upsample, the FIR-resampled Conv_0 of NCSN++ - gets a plain split)
    const int hw = in.ih * in.iw;
    const size_t nh = ((size_t)B * hw * (o.cp.C0 + o.cp.C1) + 1) / 2;      // halves -> floats
    Op ap;
    ap.kind = OP_GN_APPLY16;
    ap.src0 = in.src0; ap.src1 = in.src1; ap.C0 = pc.proto.C0; ap.C1 = pc.proto.C1; ap.hw = hw;
    ap.nscale = o.nscale; ap.nshift = o.nshift; ap.act = norm ? in.act : (int)CSD_ACT_NONE;
    ap.out = alloc_(nh);
    if (pc.ns >= 2) ap.out2 = alloc_(nh);
    // small maps: the GroupNorm's statistics + finalize launches (the pair gn() planned, still the plan's last two ops) and this pass
    // become ONE launch
    if (in.norm.kind == Norm::STREAMED && in.norm.stats_op + 2 == pl.ops.size() && !CSD_TUNE_ENV("CSD_NO_GN_FUSED") &&
        gn_fused16_groups(hw, pc.proto.C0, pc.proto.C1, pl.ops[in.norm.stats_op].gp.G) > 0) {
      ap.kind = OP_GN_FUSED16;
      ap.gp = pl.ops[in.norm.stats_op].gp;
      ap.pk_w = pl.ops[in.norm.stats_op + 1].pk_w; ap.pk_b = pl.ops[in.norm.stats_op + 1].pk_b;      // gamma, beta
      ap.nscale = NONE; ap.nshift = NONE;
      pl.ops.pop_back();
      pl.ops.pop_back();
      pl.launches -= 2;
    }
    ap.cls = CSD_PROF_GN_APPLY;
    ap.bytes = (double)B * hw * (o.cp.C0 + o.cp.C1) * (4 + 2 * (pc.ns >= 2 ? 2 : 1));
    ap.fp8_lo = pc.ns == 3;
    emit(ap);
    o.src0 = ap.out; o.src1 = ap.out2;
    o.cp.C0 = o.cp.C0 + o.cp.C1; o.cp.C1 = 0;
    o.nscale = NONE; o.nshift = NONE;
    o.src_form = ConvSrc::PLANES16;
  }

  // conv(), the epilogue's tile statistics: where every tile lies inside one sample the epilogue also leaves (sum, sumsq) per
  // (tile, cout) for the next GroupNorm (the quad kernel: per (tile, M half, cout); the fp32 kernel: per (tile, wave, cout))
  void conv_tile_stats(const PackedConv& pc, Op& o) {
    const int oh_tiled = o.cp.up == 2 ? o.cp.IH : o.cp.OH;         // (the phase form tiles the SOURCE image, four workgroups per tile)
    // (ConvKernel::FUSED: the fused-prologue kernels tile every sample on its own - ragged tiles, where they run at all, mask their statistics)
    // (phase-decomposed Upsample: fp32 partials per (tile, M half, phase) - in fp64 they cost the kernel more than the streaming pass
    // over its output that they replace - and only where its tile shape does not depend on the batch: conv16q_plan_tiles)
    if (pc.kernel == ConvKernel::PW16 || o.out_external || o.cp.taps != 9 || !(pc.kernel == ConvKernel::FUSED || oh_tiled % o.cp.TH == 0) ||
        CSD_TUNE_ENV("CSD_NO_FUSED_STATS") || (o.cp.up == 2 && !(conv16q_up4_stats_ok(o.cp) && !CSD_TUNE_ENV("CSD_NO_UP4_STATS"))))
      return;
    const int per_tile = is_quad(pc.kernel) ? 2 : (pc.kernel == ConvKernel::F32 ? 4 : 1);
    const int tpi = cdiv(oh_tiled, o.cp.TH) * o.cp.tiles_x * per_tile * (o.cp.up == 2 ? 4 : 1);
    o.stats = alloc_((size_t)B * tpi * o.cp.Cout * 2 * 2);      // doubles; never released (small)
    tile_stats[o.out] = TileStats{o.stats, tpi};
  }

  // convolution; returns output offset (allocated here unless external or in.out_to names one)
  size_t conv(const std::string& key, const ConvIn& in) {
    const PackedConv& pc = n.pconvs[n.pconv_by_name.at(key)];
    if (pc.kernel == ConvKernel::PW16_TAPS) return conv_taps(pc, in);
    const int ih = in.ih, iw = in.iw;
    Op o;
    o.kind = OP_CONV;
    o.ns = pc.ns; o.kernel = pc.kernel;
    bool loader_norm = false;
    if (!conv_geometry(pc, in, o.cp, &loader_norm)) return NONE;
    conv_operand(pc, in, loader_norm, o);
    o.pk_w = pc.w_off; o.pk_b = pc.b_off;
    o.res = in.residual;
    o.temb_base = dense_all;
    o.out_scale = in.out_scale;
    o.act = in.act;
    o.temb_col = in.temb_col;
    o.temb_stride = n.dense_total;
    o.out_external = in.external_nchw ? 1 : 0;
    const size_t out_elems = (size_t)B * o.cp.OH * o.cp.OW * o.cp.Cout;
    o.out = in.external_nchw ? NONE : (in.out_to != NONE ? in.out_to : alloc_(out_elems));
    conv_tile_stats(pc, o);
    o.cls = o.cp.taps == 1 ? CSD_PROF_CONV1X1 : ((in.stride == 1 && !in.up) ? CSD_PROF_CONV3X3 : CSD_PROF_CONV3X3_RESAMPLE);
    emit(o);
    if (o.src_form == ConvSrc::PLANES16) { ar.release(o.src0); ar.release(o.src1); }      // (plan-time lifetimes: the planes die right after this conv)
    const int cin = in.real_cin > 0 ? in.real_cin : (o.cp.C0 + o.cp.C1);
    count(2.0 * out_elems * cin * o.cp.taps, ((double)B * ih * iw * cin + (double)out_elems) * 4);
    // the profiler's per-launch bytes are what THIS kernel has to move (fp16 planes in, fp32 out, residual in);
    // the plan totals above stay the SURVEY 8(d) algorithmic figures
    pl.ops.back().abytes = pl.ops.back().bytes;
    pl.ops.back().bytes = (double)B * ih * iw * (o.cp.C0 + o.cp.C1) * (o.src_form != ConvSrc::F32 ? 2.0 * pc.ns : 4.0) +
                          (double)out_elems * 4 * (in.residual != NONE ? 2 : 1);
    return o.out;
  }

  // the fused first layer (stem.hip): x, y (+ sigma z) in the caller's NCHW -> nf channels NHWC + tile partials for the next GroupNorm
  size_t stem(const PackedConv& pc, const Module& m, int S) {
    const csd_unet_config& c = n.cfg;
    Op o;
    o.kind = OP_STEM;
    o.pk_w = pc.w_off; o.pk_b = pc.b_off;
    o.Cout = m.cout; o.ns = pc.ns; o.kernel = pc.kernel;
    const size_t out_elems = (size_t)B * S * S * m.cout;
    o.out = alloc_(out_elems);
    const int tpi = stem_tiles_per_image(S);
    o.stats = alloc_((size_t)B * tpi * m.cout * 2 * 2);      // doubles; never released (small)
    tile_stats[o.out] = TileStats{o.stats, tpi};
    // y_scale: room for the perturbed low-resolution y + sigma z of a sampling step (never released: a few KB per sample)
    if (c.y_scale) o.out2 = alloc_((size_t)B * c.y_channels * (S / c.y_scale) * (S / c.y_scale));
    o.cls = CSD_PROF_CONV3X3;
    emit(o);
    const int cin = c.x_channels + c.y_channels;
    count(2.0 * out_elems * cin * 9, ((double)B * S * S * cin + (double)out_elems) * 4);
    return o.out;
  }

  size_t res_block(const Module& m, size_t x0, size_t x1, int c0, int c1, int hw_side, size_t out_to = NONE) {
    const std::string k = std::to_string(m.idx);
    const int hw = hw_side * hw_side;
    // the shortcut contraction first; with CSD_SIDE_STREAM=1 on the side stream (it only depends on the block's input; Conv_1 joins it).
    // Opt-in: -0.35 ms per PC step in a same-box A/B, but the per-launch durations of the overlapped 3x3 launches (what the bench's
    // roofline object and the rocprofv3 summaries report) then include the time they share the CUs with it
    static const bool side_on = CSD_TUNE_ENV("CSD_SIDE_STREAM") != nullptr && atoi(CSD_TUNE_ENV("CSD_SIDE_STREAM")) != 0;
    size_t shortcut = x0, sc_buf = NONE;
    if (m.cin != m.cout) {
      const size_t op0 = pl.ops.size();
      sc_buf = conv(k + (n.cfg.arch == 1 ? ".Conv_2" : ".NIN_0"), {.src0 = x0, .src1 = x1, .ih = hw_side, .iw = hw_side});
      shortcut = sc_buf;
      if (side_on)
        for (size_t i = op0; i < pl.ops.size(); ++i) pl.ops[i].side = 1;
    } else if (x1 != NONE) {
      set_error("res block %d: identity shortcut on a concatenated input is not supported", m.idx);
      rc = CSD_ERR_INVALID;
    }
    const Norm n0 = gn(x0, x1, c0, c1, hw, mname(m.idx, "GroupNorm_0.weight"), mname(m.idx, "GroupNorm_0.bias"));
    const size_t tcol = n.cfg.conditional ? (size_t)n.dense_col.at(m.idx) : NONE;
    const size_t h1 = conv(k + ".Conv_0", {.src0 = x0, .src1 = x1, .ih = hw_side, .iw = hw_side, .pad = 1, .norm = n0, .act = n.cfg.act, .temb_col = tcol});
    const Norm n1 = gn(h1, NONE, m.cout, 0, hw, mname(m.idx, "GroupNorm_1.weight"), mname(m.idx, "GroupNorm_1.bias"));
    const size_t out = conv(k + ".Conv_1", {.src0 = h1, .ih = hw_side, .iw = hw_side, .pad = 1, .norm = n1, .act = n.cfg.act, .residual = shortcut,
                                            .out_scale = skip_scale(), .out_to = out_to});
    if (side_on && sc_buf != NONE && rc == CSD_OK && out != NONE) pl.ops.back().side = 2;
    ar.release(h1);
    ar.release(sc_buf);
    return out;
  }

  float skip_scale() const { return (n.cfg.arch == 1 && n.cfg.skip_rescale) ? 0.70710678118654752440f : 1.f; }

  // ---- NCSN++ pieces (models/layerspp.py, models/up_or_down_sampling.py) ----
  // FIR resampling of an fp32 NHWC tensor: upsample_2d / downsample_2d with the config's 4-tap kernel
  size_t fir(size_t src, int side, int C, bool up) {
    Op o;
    o.kind = OP_FIR;
    o.src0 = src; o.H = o.W = side; o.C0 = C; o.up = up;
    const int os = up ? side * 2 : side / 2;
    o.out = alloc_((size_t)B * os * os * C);
    o.cls = CSD_PROF_OTHER;
    emit(o);
    return o.out;
  }

  // 'residual' input pyramid (ncsnpp.py:300-307): (Downsample(src) + h) * skip scale in ONE launch (fir_pyramid.hip); src NHWC with
  // `pix` floats per pixel.  (The next GroupNorm takes its statistics from a streaming pass: this kernel leaves no tile partials.)
  size_t pyr_conv(const Module& m, size_t src, int pix, int side, size_t h) {
    const csd_unet_config& c = n.cfg;
    Op o;
    o.kind = OP_PYRCONV;
    o.src0 = src; o.res = h;
    o.pk_w = n.pyr_fold_off.at(m.idx); o.pk_b = n.copy_off.at(mname(m.idx, pyr_sub(c, true)));
    o.H = o.W = side; o.C0 = m.cin; o.Cout = m.cout; o.pix = pix; o.fir = c.progressive_input == 2;
    o.out_scale = c.skip_rescale ? 0.70710678118654752440f : 1.f;
    const size_t out_elems = (size_t)B * (side / 2) * (side / 2) * m.cout;
    o.out = alloc_(out_elems);
    o.cls = CSD_PROF_CONV3X3_RESAMPLE;
    emit(o);
    // algorithmic flops: FIR + VALID stride-2 3x3 (fir) or the stride-2 3x3 (fir = False), as the reference computes them
    count(2.0 * out_elems * m.cin * 9 + (o.fir ? 2.0 * B * (side + 1) * (side + 1) * m.cin * 16 : 0.0),
          ((double)B * side * side * m.cin + 2.0 * out_elems) * 4);
    return o.out;
  }

  // act(GroupNorm(x)) materialised in fp32 (the up/down blocks resample it before Conv_0)
  size_t gn_apply32(size_t src, int C, int hw, int act) {
    Op o;
    o.kind = OP_GN_APPLY32;
    o.src0 = src; o.nscale = nscale; o.nshift = nshift; o.C0 = C; o.hw = hw; o.act = act;
    o.out = alloc_((size_t)B * hw * C);
    o.cls = CSD_PROF_GN_APPLY;
    o.bytes = (double)B * hw * C * 8;
    emit(o);
    return o.out;
  }

  // ResnetBlockBigGANpp with up / down (layerspp.py:242-274): GN0+act -> FIR(h), FIR(x) -> Conv_0 (+temb) -> GN1+act
  // -> Conv_1 + Conv_2(x') ; (x + h)/sqrt(2)
  size_t res_block_updown(const Module& m, size_t x, int side) {
    const std::string k = std::to_string(m.idx);
    const int hw = side * side, os = m.up ? side * 2 : side / 2;
    gn(x, NONE, m.cin, 0, hw, mname(m.idx, "GroupNorm_0.weight"), mname(m.idx, "GroupNorm_0.bias"));
    size_t hr, xr;
    if (m.cin % 4 == 0) {      // FIR(act(GroupNorm(x))) and FIR(x) in one pass over x (elementwise.hip: fir_resample2)
      Op o;
      o.kind = OP_FIR2;
      o.src0 = x; o.nscale = nscale; o.nshift = nshift; o.H = o.W = side; o.C0 = m.cin; o.up = m.up != 0; o.act = n.cfg.act;
      o.out = alloc_((size_t)B * os * os * m.cin);       // FIR(h)
      o.out2 = alloc_((size_t)B * os * os * m.cin);      // FIR(x)
      o.cls = CSD_PROF_OTHER;
      o.bytes = (double)B * (hw + 2.0 * os * os) * m.cin * 4;
      emit(o);
      hr = o.out; xr = o.out2;
    } else {
      const size_t ha = gn_apply32(x, m.cin, hw, n.cfg.act);
      hr = fir(ha, side, m.cin, m.up != 0);
      ar.release(ha);
      xr = fir(x, side, m.cin, m.up != 0);
    }
    const size_t tcol = (size_t)n.dense_col.at(m.idx);
    const size_t h1 = conv(k + ".Conv_0", {.src0 = hr, .ih = os, .iw = os, .pad = 1, .temb_col = tcol});
    ar.release(hr);
    const Norm n1 = gn(h1, NONE, m.cout, 0, os * os, mname(m.idx, "GroupNorm_1.weight"), mname(m.idx, "GroupNorm_1.bias"));
    const size_t sc = conv(k + ".Conv_2", {.src0 = xr, .ih = os, .iw = os});
    ar.release(xr);
    const size_t out = conv(k + ".Conv_1", {.src0 = h1, .ih = os, .iw = os, .pad = 1, .norm = n1, .act = n.cfg.act, .residual = sc,
                                            .out_scale = skip_scale()});
    ar.release(h1);
    ar.release(sc);
    return out;
  }

  size_t attn_block(const Module& m, size_t x, int hw_side, size_t out_to = NONE) {
    const std::string k = std::to_string(m.idx);
    const int C = m.cin, L = hw_side * hw_side;
    const Norm n0 = gn(x, NONE, C, 0, L, mname(m.idx, "GroupNorm_0.weight"), mname(m.idx, "GroupNorm_0.bias"));
    const size_t qkv = conv(k + ".qkv", {.src0 = x, .ih = hw_side, .iw = hw_side, .norm = n0});
    Op a;
    a.kind = OP_ATTN;
    a.src0 = qkv; a.hw = L; a.C0 = C;
    a.out = alloc_((size_t)B * L * C);
    a.cls = CSD_PROF_ATTENTION;
    emit(a);
    count(4.0 * B * (double)L * L * C, 0);
    const size_t o = conv(k + ".NIN_3", {.src0 = a.out, .ih = hw_side, .iw = hw_side, .residual = x, .out_scale = skip_scale(), .out_to = out_to});
    ar.release(qkv);
    ar.release(a.out);
    return o;
  }

  // time embedding (models/ddpm.py:153-160, models/ncsnpp.py:270-290): the sinusoidal embedding or the Fourier features of the label, the two
  // Linear layers and every block's Dense_0(act(temb)) in one launch.  l1: the second Linear (in front of it: the first, then the Fourier entry)
  void time_embedding(const Module& l1) {
    const csd_unet_config& c = n.cfg;
    const int nf = c.nf;
    const Module& l0 = n.mods[l1.idx - 1];
    const bool fourier = l0.idx > 0 && n.mods[l0.idx - 1].role == R_EMB_FOURIER;
    Op e;
    e.kind = fourier ? OP_FOURIER : OP_TEMB;
    if (fourier) e.pk_w = n.copy_off.at(mname(l0.idx - 1, "W"));
    e.C0 = nf;
    e.out = alloc_((size_t)B * l0.cin);
    emit(e);
    auto linear = [&](size_t src, size_t pk_w, size_t pk_b, int cin, int cout, int out_act) {
      Op a;
      a.kind = OP_LINEAR;
      a.src0 = src; a.out = alloc_((size_t)B * cout);
      a.pk_w = pk_w; a.pk_b = pk_b;
      a.C0 = cin; a.Cout = cout; a.act = CSD_ACT_NONE; a.out_act = out_act;
      emit(a);
      return a.out;
    };
    const size_t t0 = linear(e.out, n.copy_off.at(mname(l0.idx, "weight")), n.copy_off.at(mname(l0.idx, "bias")), l0.cin, 4 * nf, c.act);
    const size_t t1 = linear(t0, n.copy_off.at(mname(l1.idx, "weight")), n.copy_off.at(mname(l1.idx, "bias")), 4 * nf, 4 * nf, c.act);
    dense_all = linear(t1, n.dense_all_off, n.dense_all_bias_off, 4 * nf, n.dense_total, CSD_ACT_NONE);   // every block's Dense_0(act(temb)) in one launch
    pl.flops += 2.0 * B * ((double)l0.cin * 4 * nf + 16.0 * nf * nf + 4.0 * nf * n.dense_total);
    // (only the DDPM family's plans have ever counted the embedding's bytes; the totals are pinned, see tests/golden/plan_digests.json)
    if (c.arch == 0) pl.bytes += 4.0 * B * (nf + 4 * nf + 4 * nf + 4 * nf + (4.0 * nf + 1) * 0 + 2.0 * n.dense_total);
  }

  // Downsample / Upsample of the DDPM family without a conv: 2x2 average pool / nearest x2
  size_t resample_plain(OpKind kind, size_t src, int side, int C, int out_side) {
    Op p;
    p.kind = kind;
    p.src0 = src; p.H = p.W = side; p.C0 = C;
    p.out = alloc_((size_t)B * out_side * out_side * C);
    emit(p);
    return p.out;
  }

  // the shared GroupNorm scratch of a walk at batch nb over the levels l0 .. n_levels - 1: worst-case partials, scale + shift
  void gn_scratch(int nb, int l0, int cmax) {
    GNPlan g;
    size_t worst = 0;
    for (int l = l0; l < n.cfg.n_levels; ++l) {
      const int side = n.cfg.image_size >> l;
      gn_plan(&g, nb, side * side, cmax, 0, 32);
      worst = std::max(worst, gn_partial_bytes(g));
    }
    gn_partial = alloc_(worst / sizeof(float) + 64);
    nscale = alloc_((size_t)nb * cmax);
    nshift = alloc_((size_t)nb * cmax);
  }

  // ---- the walk (models/ddpm.py:149-213, models/ncsnpp.py:238-388): one module of Net::mods on this Builder's batch ----
  // (out_to: the module writes there instead of into a tensor of its own - a batch chunk's slice of the region's output)
  void step(const Module& m, size_t out_to = NONE) {
    const csd_unet_config& c = n.cfg;
    const bool pp = c.arch == 1;
    const int S = c.image_size, channels = c.x_channels + c.y_channels;
    const std::string k = std::to_string(m.idx);
    size_t o = NONE, sk = NONE;
    switch (m.role) {
      case R_EMB_FOURIER: case R_EMB_LINEAR0:
        return;                                  // (planned with the MLP's last module)
      case R_EMB_LINEAR1:
        time_embedding(m);
        return;
      case R_STEM: {
        const PackedConv& pc = n.pconvs[n.pconv_by_name.at(k)];
        o = pc.kernel == ConvKernel::STEM ? stem(pc, m, S) : conv(k, {.src0 = w.as_out, .ih = S, .iw = S, .pad = 1, .real_cin = channels});
        if (!pp) { ar.release(w.as_out); w.as_out = NONE; }      // (NCSN++ keeps it for the input pyramid: released behind the down path)
        break;
      }
      case R_MID_RES_IN:                         // the down path is done: the input pyramid and the assembled input die here
        if (pp && c.progressive_input == 1 && w.pyr_in != w.as_out) ar.release(w.pyr_in);
        ar.release(w.as_out);
        [[fallthrough]];
      case R_DOWN_BLOCK: case R_MID_RES_OUT: case R_UP_BLOCK:
        if (m.skip) { sk = w.hs.back(); w.hs.pop_back(); }
        o = res_block(m, w.h, sk, m.cin - m.skip, m.skip, m.side, out_to);
        break;
      case R_ATTN: case R_MID_ATTN:
        o = attn_block(m, w.h, m.side, out_to);
        break;
      case R_DOWNSAMPLE:
        o = m.kind == M_RES ? res_block_updown(m, w.h, m.side)
          : c.resamp_with_conv ? conv(k + ".Conv_0", {.src0 = w.h, .ih = m.side, .iw = m.side, .stride = 2})
                               : resample_plain(OP_AVGPOOL, w.h, m.side, m.cin, m.out_side);
        break;
      case R_UPSAMPLE:
        o = m.kind == M_RES ? res_block_updown(m, w.h, m.side)
          : c.resamp_with_conv ? conv(k + ".Conv_0", {.src0 = w.h, .ih = m.side, .iw = m.side, .pad = 1, .up = 1})
                               : resample_plain(OP_UPNEAR, w.h, m.side, m.cin, m.out_side);
        break;
      case R_COMBINE: {                          // pyramid_downsample (FIR, no conv), then Combine 'sum' (layerspp.py:53-57): Conv_0(input_pyramid) + h
        const size_t pn = fir(w.pyr_in, w.pyr_side, n.in_cpad, false);
        if (w.pyr_in != w.as_out) ar.release(w.pyr_in);
        w.pyr_in = pn;
        w.pyr_side /= 2;
        o = conv(k + ".Conv_0", {.src0 = w.pyr_in, .ih = m.side, .iw = m.side, .residual = w.h, .real_cin = channels});
        break;
      }
      case R_PYR_DOWN:
        // 'residual': input_pyramid = Downsample(input_pyramid); h = (input_pyramid + h) * skip scale; input_pyramid = h.  From level 1
        // on the source is the previous level's combined h, a live skip-stack entry: the up path releases it, never this one
        o = pyr_conv(m, w.pyr_in, w.pyr_pix, m.side, w.h);
        w.pyr_in = o; w.pyr_pix = m.cout;
        break;
      case R_PYR_GN: case R_HEAD_GN:
        if (w.pyr != NONE) {
          w.pyr_up = fir(w.pyr, m.side / 2, channels, true);      // pyramid_upsample
          ar.release(w.pyr);
        }
        w.out_norm = gn(w.h, NONE, m.cin, 0, m.side * m.side, mname(m.idx, "weight"), mname(m.idx, "bias"));
        return;
      case R_PYR_CONV: case R_HEAD_CONV:         // (level 0: straight to the caller's NCHW output, pyr = NONE)
        w.pyr = conv(k, {.src0 = w.h, .ih = m.side, .iw = m.side, .pad = 1, .norm = w.out_norm, .act = c.act, .residual = w.pyr_up,
                         .external_nchw = m.level == 0});
        ar.release(w.pyr_up);
        w.pyr_up = NONE;
        return;
    }
    if (!w.h_on_stack) ar.release(w.h);
    ar.release(sk);
    w.h = o;
    w.h_on_stack = m.push;
    if (m.push) w.hs.push_back(w.h);
  }
};

// after the walk: a GroupNorm whose statistics + finalize pair survived (its consumer applies scale / shift itself: the attention
// blocks' q/k/v contraction, the last layer) becomes ONE launch when the map is small enough for the one-sweep kernel
static void fold_small_gn_pairs(Plan& pl) {
  if (CSD_TUNE_ENV("CSD_NO_GN_FUSED")) return;
  std::vector<Op> out;
  out.reserve(pl.ops.size());
  for (size_t i = 0; i < pl.ops.size(); ++i) {
    const Op& a = pl.ops[i];
    if (a.kind == OP_GN_STATS && i + 1 < pl.ops.size() && pl.ops[i + 1].kind == OP_GN_FINAL &&
        gn_fused16_groups(a.gp.HW, a.gp.C0, a.gp.C1, a.gp.G) > 0) {
      const Op& f = pl.ops[i + 1];
      Op o;
      o.kind = OP_GN_STATFIN;
      o.src0 = a.src0; o.src1 = a.src1; o.gp = a.gp;
      o.pk_w = f.pk_w; o.pk_b = f.pk_b;
      o.nscale = f.nscale; o.nshift = f.nshift;
      o.cls = CSD_PROF_GN_STATS; o.bytes = a.bytes;
      o.nb = a.nb; o.stream = a.stream; o.chunk = a.chunk;
      out.push_back(o);
      pl.launches -= 1;
      ++i;
    } else {
      out.push_back(a);
    }
  }
  pl.ops.swap(out);
}

// profiling classes: when the plan runs its big 3x3 stride-1 layers on the fused-prologue kernel (conv_xk / conv_ff: ConvKernel::FUSED),
// class CSD_PROF_CONV3X3 is THAT kernel's launches - the bench's roofline object prices the dominant kernel, SURVEY 8(d) - and the
// other 3x3 stride-1 launches (the first layer, the quad kernel on the small maps) report as CSD_PROF_CONV3X3_OTHER
static void split_conv3x3_classes(Plan& pl) {
  auto is_ff = [](const Op& o) { return o.kind == OP_CONV && o.kernel == ConvKernel::FUSED; };
  if (std::none_of(pl.ops.begin(), pl.ops.end(), is_ff)) return;
  for (Op& o : pl.ops)
    if (o.cls == CSD_PROF_CONV3X3 && !is_ff(o)) o.cls = CSD_PROF_CONV3X3_OTHER;
}

// the ops of a chunk region are enqueued round robin over the chunks (op j of every chunk, then op j + 1): when the host is the slower
// side, every chunk stream still advances - chunk after chunk, the last stream would start when the first is nearly done
static void interleave_chunks(Plan& pl) {
  std::vector<Op> out;
  out.reserve(pl.ops.size());
  for (size_t i = 0; i < pl.ops.size();) {
    if (pl.ops[i].kind != OP_FORK) { out.push_back(pl.ops[i++]); continue; }
    out.push_back(pl.ops[i++]);
    std::vector<std::vector<Op>> per;
    while (i < pl.ops.size() && pl.ops[i].kind != OP_JOIN) {
      const int k = pl.ops[i].chunk - 1;
      if (k < 0) break;
      if ((int)per.size() <= k) per.resize(k + 1);
      per[k].push_back(pl.ops[i++]);
    }
    size_t longest = 0;
    for (auto& v : per) longest = std::max(longest, v.size());
    for (size_t j = 0; j < longest; ++j)
      for (auto& v : per)
        if (j < v.size()) out.push_back(v[j]);
  }
  pl.ops.swap(out);
}

static int build_plan(Net& n, int B, Plan** out) {
  auto it = n.plans.find(B);
  if (it != n.plans.end()) { *out = it->second.get(); return CSD_OK; }
  CSD_REQUIRE(B >= 1, "unet: batch must be >= 1");
  std::unique_ptr<Plan> plp(new Plan());
  Plan& pl = *plp;
  pl.B = B;
  Builder bd(n, pl, B);
  const csd_unet_config& c = n.cfg;
  const bool pp = c.arch == 1;
  const int S = c.image_size, last = c.n_levels - 1;
  int cmax = c.nf;
  for (auto& m : n.mods) cmax = std::max(cmax, std::max(m.cin, m.cout));
  bd.gn_scratch(B, 0, cmax);

  // ---- input assembly: a launch of its own unless the fused first layer reads x, y itself (the NCSN++ input pyramid reads the tensor) ----
  const Module& stem_m = *std::find_if(n.mods.begin(), n.mods.end(), [](const Module& m) { return m.role == R_STEM; });
  const bool fused_stem = n.pconvs[n.pconv_by_name.at(std::to_string(stem_m.idx))].kernel == ConvKernel::STEM;
  const bool pyramid_in = pp && c.progressive_input != 0;
  if (!fused_stem || pyramid_in) {
    Op as;
    as.kind = OP_ASSEMBLE;
    as.out = bd.w.as_out = bd.alloc_((size_t)B * S * S * n.in_cpad);
    bd.emit(as);
  }
  if (pyramid_in) bd.w.pyr_in = bd.w.as_out;
  bd.w.pyr_side = S; bd.w.pyr_pix = n.in_cpad;

  // Batch chunks: below CHUNK_SIDE^2 a launch is bound by its own dependent chain (weights -> LDS, K steps of global loads, epilogue), not by
  // throughput - at 5^2 / 10^2 a kernel takes the same ~20 us for 8 samples as for 64 (profiles/r06_*: timeline by batch).  The levels
  // l0 .. last therefore run as K independent sub-batches on K streams between the Downsample conv that enters level l0 and the Upsample
  // conv that leaves it: each chunk walks the same modules - the range [i_lo, i_hi] of Net::mods, the first module of level l0 to the last
  // one of that level on the up path - with its own temporaries (a private block of the workspace) and reads / writes its slice of the
  // two full-batch tensors at the region's boundary.  A sample's bits do not depend on the batch it runs in (tests: B = 64 == B = 1), so
  // the chunked plan returns the bits of the unchunked one.  DDPM family only: NCSN++ has not been measured with chunks.
  int l0 = c.n_levels, K = 1;
  {
    const char* e_side = CSD_TUNE_ENV("CSD_CHUNK_SIDE");
    const char* e_k = CSD_TUNE_ENV("CSD_CHUNKS");
    const int chunk_side = e_side ? atoi(e_side) : 20;
    for (int l = 1; l <= last; ++l)
      if ((S >> l) <= chunk_side) { l0 = l; break; }
    K = e_k ? atoi(e_k) : (B >= 64 ? 2 : 1);      // measured (NOTEBOOK round 6): B = 64: 2 chunks -0.24 ms per PC step, 3 chunks +0.25; B = 16 .. 48: 2 chunks +0.05 .. +0.23 ms
    K = std::max(1, std::min(K, std::min(B, (int)Net::MAX_CHUNKS)));
    if (l0 > last || pp) K = 1;
  }
  size_t i_lo = n.mods.size(), i_hi = n.mods.size();
  for (const Module& m : n.mods) {
    if (K > 1 && m.level == l0 && m.role == R_DOWN_BLOCK && i_lo == n.mods.size()) i_lo = m.idx;
    if (K > 1 && m.level == l0 && m.last_up) i_hi = m.idx;
  }
  for (size_t i = 0; i < n.mods.size(); ++i) {
    if (i != i_lo) { bd.step(n.mods[i]); continue; }
    const int side0 = S >> l0, Bc = cdiv(B, K);
    const size_t in_full = bd.w.hs.back();              // [B, side0, side0, ch]: the Downsample output that enters level l0
    const size_t in_ps = (size_t)side0 * side0 * n.mods[i_lo].cin, out_ps = (size_t)side0 * side0 * n.mods[i_hi].cout;
    const size_t out_full = bd.alloc_((size_t)B * out_ps);
    // samples b0 .. b0 + nb - 1 planned as a batch of their own by a Builder of their own: its arena starts at `base`, it knows no
    // tile statistics, has its own GroupNorm scratch, reads its rows of dense_all and starts from its slice of the region's input as
    // the one entry of its skip stack.  The main Builder is only read.  *peak: what the chunk needed, in floats from `base`
    auto plan_chunk = [&](Plan& sink, int b0, int nb, size_t base, size_t* peak) {
      Builder cb(n, sink, nb, Arena(base));
      cb.dense_all = bd.dense_all == NONE ? NONE : bd.dense_all + (size_t)b0 * n.dense_total;
      cb.gn_scratch(nb, l0, cmax);
      cb.w.hs.assign(1, in_full + (size_t)b0 * in_ps);
      cb.w.h = cb.w.hs.back();
      for (size_t j = i_lo; j <= i_hi; ++j) cb.step(n.mods[j], j == i_hi ? out_full + (size_t)b0 * out_ps : NONE);
      *peak = cb.ar.peak();
      return cb.rc;
    };
    // a chunk's private block: the largest peak over the region's chunk sizes - Bc and, for a ragged batch, the last chunk's (a peak is
    // not monotone in the batch: which convs leave never-released tile statistics depends on their tiling, that is on nb * OH) - each
    // from a dry run into a throwaway Plan, at a base no offset of the main arena reaches (Arena::release ignores what lies below it)
    size_t chunk_floats = 0;
    for (const int nb : {Bc, B % Bc}) {
      if (nb == 0) continue;
      Plan dry;
      size_t peak = 0;
      const int rc = plan_chunk(dry, 0, nb, (size_t)1 << 40, &peak);
      if (rc) return rc;
      chunk_floats = std::max(chunk_floats, (peak + 63) / 64 * 64);
    }
    const size_t block = bd.alloc_((size_t)K * chunk_floats);
    Op fork, join;
    fork.kind = OP_FORK; join.kind = OP_JOIN;
    fork.n_chunks = join.n_chunks = K;
    bd.emit(fork, 0);
    for (int k = 0; k < K; ++k) {
      const int b0 = k * Bc, nb = std::min(Bc, B - b0);
      if (nb <= 0) break;
      const size_t i0 = pl.ops.size();
      size_t peak = 0;
      const int rc = plan_chunk(pl, b0, nb, block + (size_t)k * chunk_floats, &peak);
      if (rc) return rc;
      CSD_REQUIRE(peak <= chunk_floats, "unet: a chunk outgrew its block");
      for (size_t j = i0; j < pl.ops.size(); ++j) { pl.ops[j].nb = nb; pl.ops[j].stream = k; pl.ops[j].chunk = k + 1; }
    }
    bd.emit(join, 0);
    // back in the full batch: the block and the region's input (consumed by every chunk's last up block) die, the walk goes on behind i_hi
    bd.ar.release(block);
    bd.ar.release(in_full);
    bd.w.hs.pop_back();
    bd.w.h = out_full; bd.w.h_on_stack = false;
    i = i_hi;
  }
  bd.ar.release(bd.w.h);
  if (bd.rc) return bd.rc;
  CSD_REQUIRE(bd.w.hs.empty(), "unet: the skip stack is not empty behind the last module");
  // parameters are read once per forward (+ param_bytes per NFE)
  double pbytes = 0;
  for (auto& p : n.params) pbytes += 4.0 * p.numel;
  pl.bytes += pbytes;
  fold_small_gn_pairs(pl);
  split_conv3x3_classes(pl);
  if (!CSD_TUNE_ENV("CSD_CHUNK_SEQ")) interleave_chunks(pl);
  pl.ws_floats = bd.ar.peak();
  if (c.y_scale) {      // the head writes a workspace tensor; run_plan's last launches fill the caller's `out` from it (unet_run.h)
    pl.ys_out = pl.ws_floats;
    pl.ws_floats += ((size_t)B * c.out_channels * S * S + 63) / 64 * 64;
    pl.launches += 2;
  }
  *out = plp.get();
  n.plans[B] = std::move(plp);
  return CSD_OK;
}

}  // namespace csd
