// unet_plan.h - the inference plan of a network for one batch size: a flat list of kernel launches with every workspace offset fixed
// (Builder: one method per module kind; build_plan: one walk over Net::mods).  Included by unet.hip.
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
  float pending_scale = 1.f;          // out_scale of the NEXT conv() (NCSN++ skip_rescale: (x + h)/sqrt(2))
  size_t next_out = NONE;             // the NEXT conv() writes here instead of allocating (a batch chunk's slice of the region's output tensor)
  int rc = CSD_OK;
  // tensors whose producing conv left per-tile GroupNorm partials behind: workspace offset -> (partials, tiles per sample)
  struct TileStats { size_t off; int tpi; };
  std::map<size_t, TileStats> tile_stats;

  Builder(Net& n_, Plan& p_, int B_) : n(n_), pl(p_), B(B_) {}

  // every workspace allocation goes through here: a new tensor at an offset invalidates what was known about the old one
  size_t alloc_(size_t nfloats) {
    const size_t off = ar.alloc(nfloats);
    tile_stats.erase(off);
    return off;
  }

  void count(double flops, double bytes) {
    pl.flops += flops; pl.bytes += bytes; pl.launches += 1;
    pl.ops.back().flops = flops; pl.ops.back().bytes = bytes;
  }

  // GroupNorm statistics of (src0|src1) -> nscale/nshift
  void gn(size_t src0, size_t src1, int c0, int c1, int hw, const std::string& gname, const std::string& bname) {
    const int G = n.cfg.arch == 1 ? ncsnpp_groups(c0 + c1) : 32;
    if (src1 != NONE && (tile_stats.count(src0) != 0) != (tile_stats.count(src1) != 0)) {
      // a concatenated input of which ONE half carries epilogue partials (the skip tensor next to an Upsample output): the streaming pass
      // reads only the other half and leaves per-channel partials in the same layout (it used to re-read both: 1.26 GB at 160^2 x 192)
      const bool first = tile_stats.count(src0) == 0;
      const size_t src = first ? src0 : src1;
      const int cs = first ? c0 : c1;
      Op s;
      s.kind = OP_GN_STATS;
      if (gn_plan(&s.gp, B, hw, cs, 0, 1)) { rc = CSD_ERR_INVALID; return; }
      s.src0 = src; s.per_channel = true;
      s.stats = alloc_((size_t)B * s.gp.nchunk * cs * 2 * 2);      // doubles; never released (small)
      s.cls = CSD_PROF_GN_STATS; s.bytes = (double)B * hw * cs * 4;
      pl.ops.push_back(s);
      pl.launches += 1;
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
      pl.ops.push_back(f);
      pl.launches += 1;
      pl.bytes += 2.0 * B * hw * (c0 + c1) * 4;   // SURVEY 8(d) algorithmic bytes are those of the unfused op
      return;
    }
    Op s;
    s.kind = OP_GN_STATS;
    if (gn_plan(&s.gp, B, hw, c0, c1, G)) { rc = CSD_ERR_INVALID; return; }
    s.src0 = src0; s.src1 = src1; s.stats = gn_partial;
    s.cls = CSD_PROF_GN_STATS; s.bytes = (double)B * hw * (c0 + c1) * 4;
    pl.ops.push_back(s);
    Op f;
    f.kind = OP_GN_FINAL;
    f.gp = s.gp;
    f.stats = gn_partial; f.pk_w = n.copy_off.at(gname); f.pk_b = n.copy_off.at(bname);
    f.nscale = nscale; f.nshift = nshift;
    f.cls = CSD_PROF_GN_FINAL;
    pl.ops.push_back(f);
    pl.launches += 2;
    pl.bytes += 2.0 * B * hw * (c0 + c1) * 4;   // GroupNorm reads + writes its tensor
  }

  // the arguments of conv() beside the layer's key
  struct ConvIn {
    size_t src0 = NONE, src1 = NONE;      // sources (src1: the second of a virtual concat)
    int ih = 0, iw = 0;                   // extent of the source map
    int stride = 1, pad = 0, up = 0;
    bool norm = false;                    // reads act(GroupNorm(sources)): scale / shift are the ones gn() has just planned
    int act = CSD_ACT_NONE;
    size_t residual = NONE;               // added by the epilogue
    size_t temb_col = NONE;               // first column of the block's Dense_0 rows inside dense_all
    bool external_nchw = false;           // writes the caller's NCHW output
    int real_cin = -1;                    // input channels the flop count takes (a zero-padded input)
  };

  int fail(const char* what) { set_error("%s", what); rc = CSD_ERR_INVALID; return rc; }

  // tap-partial form (conv_pw16.hip): pointwise contraction of act(GN(x)) to 9 * cout partial channels, then the 9-tap gather
  size_t conv_taps(const PackedConv& pc, const ConvIn& in) {
    const int ih = in.ih, iw = in.iw;
    if (!in.norm || in.src1 != NONE || in.stride != 1 || in.up || in.pad != 1 || in.temb_col != NONE) {
      fail("tap-partial conv on an unsupported layer"); return NONE;
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
    pl.ops.push_back(o);
    const size_t out_elems = (size_t)B * ih * iw * pc.tap_cout;
    count(2.0 * out_elems * o.cp.C0 * 9, ((double)B * ih * iw * o.cp.C0 + (double)out_elems) * 4);
    pl.ops.back().bytes = (double)B * ih * iw * (o.cp.C0 + o.cp.Cout) * 4.0;
    Op g;
    g.kind = OP_TAPSUM;
    g.src0 = part; g.pk_b = pc.b_off; g.res = in.residual;
    g.H = ih; g.W = iw; g.Cout = pc.tap_cout;
    g.out_scale = pending_scale;
    pending_scale = 1.f;
    g.out_external = in.external_nchw ? 1 : 0;
    g.out = in.external_nchw ? NONE : alloc_(out_elems);
    g.cls = CSD_PROF_OTHER;
    g.bytes = (double)B * ih * iw * (o.cp.Cout + pc.tap_cout) * 4.0;
    pl.ops.push_back(g);
    pl.launches += 1;
    ar.release(part);
    return g.out;
  }

  // convolution; returns output offset (allocated here unless external)
  size_t conv(const std::string& key, const ConvIn& in) {
    const PackedConv& pc = n.pconvs[n.pconv_by_name.at(key)];
    if (pc.kernel == ConvKernel::PW16_TAPS) return conv_taps(pc, in);
    const int ih = in.ih, iw = in.iw, stride = in.stride, up = in.up;
    const bool norm = in.norm, external_nchw = in.external_nchw, quad = is_quad(pc.kernel);
    Op o;
    o.kind = OP_CONV;
    o.cp = pc.proto;
    o.cp.B = B; o.cp.IH = ih; o.cp.IW = iw;
    o.cp.stride = stride; o.cp.pad = in.pad; o.cp.up = up;
    o.cp.OH = (ih << up) / stride; o.cp.OW = (iw << up) / stride;
    o.ns = pc.ns; o.kernel = pc.kernel;
    // tuning only (CSD_FUSED_NORM): GroupNorm affine + activation applied by the loader / consumer kernel's loader wave (no gn_apply16
    // pass).  (The switch also reaches a layer packed for ConvKernel::FUSED, as it always has: an experiment, not a product path)
    bool fused = false;
    if ((pc.kernel == ConvKernel::F16_LC || pc.kernel == ConvKernel::FUSED) && norm && stride == 1 && !up && o.cp.C0 % 32 == 0 &&
        o.cp.C1 % 32 == 0 && !CSD_TUNE_ENV("CSD_NO_LC") && CSD_TUNE_ENV("CSD_FUSED_NORM")) {
      ConvPlan trial = o.cp;
      if (conv16_plan_tiles(&trial, pc.ns, 2, true) == CSD_OK && trial.LC && trial.OH % trial.TH == 0) {
        fused = true;
        o.cp = trial;
      }
    }
    if (!fused) switch (pc.kernel) {
      case ConvKernel::FUSED:
        if (external_nchw || stride != 1 || up) { fail("fused-prologue conv on an unsupported layer"); return NONE; }
        if (convff_plan_tiles(&o.cp, pc.ns)) { rc = CSD_ERR_INVALID; return NONE; }
        break;
      case ConvKernel::QUAD: case ConvKernel::QUAD_UP4:
        if (external_nchw || (!norm && o.cp.C1 != 0) || (stride == 2 && (norm || up))) { fail("quad fp16 conv on an unsupported layer"); return NONE; }
        o.cp.C0 = o.cp.C0 + o.cp.C1; o.cp.C1 = 0;
        if (pc.kernel == ConvKernel::QUAD_UP4) {
          if (!up || stride != 1) { fail("phase-decomposed Upsample packed for a layer that is not one"); return NONE; }
          o.cp.up = 2;
        }
        if (conv16q_plan_tiles(&o.cp, pc.ns)) { rc = CSD_ERR_INVALID; return NONE; }
        break;
      case ConvKernel::PW16:
        if (in.act != CSD_ACT_NONE || in.temb_col != NONE || external_nchw) { fail("pointwise fp16 layer with act/temb/NCHW"); return NONE; }
        break;
      case ConvKernel::F16_LC: {
        const int kcs = norm ? conv16_kcs(pc.ns, o.cp.C0 + o.cp.C1) : 1;    // fp16-source convs stage in bursts
        // (x_squeeze: the head's scattered NCHW store lives in conv_f16_kernel.h / conv_f32.hip; the loader / consumer schedule keeps its code)
        if (conv16_plan_tiles(&o.cp, pc.ns, kcs, kcs > 1 && !CSD_TUNE_ENV("CSD_NO_LC") && !(external_nchw && n.cfg.x_squeeze))) {
          rc = CSD_ERR_INVALID; return NONE;
        }
        break;
      }
      case ConvKernel::F32:
        if (conv_plan_tiles(&o.cp)) { rc = CSD_ERR_INVALID; return NONE; }
        break;
      case ConvKernel::PW16_TAPS: case ConvKernel::STEM:      // (conv_taps above / Builder::stem)
        fail("conv: a layer packed for another builder"); return NONE;
    }
    // the packed layout depends on KC only (not on NT / tile shape)
    if (o.cp.KC != pc.proto.KC) { fail("conv plan/pack mismatch"); return NONE; }
    o.src0 = in.src0; o.src1 = in.src1; o.pk_w = pc.w_off; o.pk_b = pc.b_off;
    o.res = in.residual;
    o.nscale = norm ? nscale : NONE;
    o.nshift = norm ? nshift : NONE;
    size_t hi16 = NONE, lo16 = NONE;
    // a quad-schedule conv WITHOUT a GroupNorm in front (Downsample / Upsample, the FIR-resampled Conv_0 of NCSN++) in the full split reads
    // its fp32 source directly: the split happens in the kernel's staging burst (no plane write / read)
    const bool q_raw = quad && !norm && pc.ns == 2 && o.cp.C1 == 0 && (o.cp.NT == 3 || o.cp.NT == 4) && !CSD_TUNE_ENV("CSD_NO_Q_RAW");
    if (q_raw) {
      o.src_form = ConvSrc::SPLIT_STAGING;
    } else if (((pc.kernel == ConvKernel::F16_LC && norm) || quad) && !fused) {
      // fp16 kernel: normalise + activate + split ONCE per element into fp16 planes, conv copies them
      // (a quad-schedule conv without a GroupNorm - Upsample, the FIR-resampled Conv_0 of NCSN++ - gets a plain split)
      const size_t nh = ((size_t)B * ih * iw * (o.cp.C0 + o.cp.C1) + 1) / 2;      // halves -> floats
      Op ap;
      ap.kind = OP_GN_APPLY16;
      ap.src0 = in.src0; ap.src1 = in.src1; ap.C0 = pc.proto.C0; ap.C1 = pc.proto.C1; ap.hw = ih * iw;
      ap.nscale = norm ? nscale : NONE; ap.nshift = norm ? nshift : NONE; ap.act = norm ? in.act : (int)CSD_ACT_NONE;
      hi16 = alloc_(nh);
      if (pc.ns >= 2) lo16 = alloc_(nh);
      ap.out = hi16; ap.out2 = lo16;
      // small maps: the GroupNorm's statistics + finalize launches (the two ops gn() has just pushed) and this pass become ONE launch
      const size_t nops = pl.ops.size();
      if (norm && nops >= 2 && pl.ops[nops - 2].kind == OP_GN_STATS && pl.ops[nops - 1].kind == OP_GN_FINAL &&
          pl.ops[nops - 2].src0 == in.src0 && pl.ops[nops - 2].src1 == in.src1 && !CSD_TUNE_ENV("CSD_NO_GN_FUSED") &&
          gn_fused16_groups(ih * iw, pc.proto.C0, pc.proto.C1, pl.ops[nops - 2].gp.G) > 0) {
        ap.kind = OP_GN_FUSED16;
        ap.gp = pl.ops[nops - 2].gp;
        ap.pk_w = pl.ops[nops - 1].pk_w; ap.pk_b = pl.ops[nops - 1].pk_b;      // gamma, beta
        ap.nscale = NONE; ap.nshift = NONE;
        pl.ops.pop_back();
        pl.ops.pop_back();
        pl.launches -= 2;
      }
      ap.cls = CSD_PROF_GN_APPLY;
      ap.bytes = (double)B * ih * iw * (o.cp.C0 + o.cp.C1) * (4 + 2 * (pc.ns >= 2 ? 2 : 1));
      ap.fp8_lo = pc.ns == 3;
      pl.ops.push_back(ap);
      pl.launches += 1;
      o.src0 = hi16; o.src1 = lo16;
      o.cp.C0 = o.cp.C0 + o.cp.C1; o.cp.C1 = 0;
      o.nscale = NONE; o.nshift = NONE;
      o.src_form = ConvSrc::PLANES16;
    }
    o.temb_base = dense_all;
    o.out_scale = pending_scale;
    pending_scale = 1.f;
    o.act = in.act;
    o.temb_col = in.temb_col;
    o.temb_stride = n.dense_total;
    o.out_external = external_nchw ? 1 : 0;
    const size_t out_elems = (size_t)B * o.cp.OH * o.cp.OW * o.cp.Cout;
    o.out = external_nchw ? NONE : (next_out != NONE ? next_out : alloc_(out_elems));
    next_out = NONE;
    const int oh_tiled = o.cp.up == 2 ? o.cp.IH : o.cp.OH;         // (the phase form tiles the SOURCE image, four workgroups per tile)
    // (ConvKernel::FUSED: the fused-prologue kernels tile every sample on its own - ragged tiles, where they run at all, mask their statistics)
    if (pc.kernel != ConvKernel::PW16 && !external_nchw && o.cp.taps == 9 && (pc.kernel == ConvKernel::FUSED || oh_tiled % o.cp.TH == 0) &&
        !CSD_TUNE_ENV("CSD_NO_FUSED_STATS") && (o.cp.up != 2 || (conv16q_up4_stats_ok(o.cp) && !CSD_TUNE_ENV("CSD_NO_UP4_STATS")))) {
      // (phase-decomposed Upsample: fp32 partials per (tile, M half, phase) - in fp64 they cost the kernel more than the streaming pass
      // over its output that they replace - and only where its tile shape does not depend on the batch: conv16q_plan_tiles)
      // every tile lies inside one sample: the epilogue also leaves (sum, sumsq) per (tile, cout) for the next
      // GroupNorm (the quad kernel: per (tile, M half, cout); the fp32 kernel: per (tile, wave, cout))
      const int per_tile = quad ? 2 : (pc.kernel == ConvKernel::F32 ? 4 : 1);
      const int tpi = cdiv(oh_tiled, o.cp.TH) * o.cp.tiles_x * per_tile * (o.cp.up == 2 ? 4 : 1);
      o.stats = alloc_((size_t)B * tpi * o.cp.Cout * 2 * 2);      // doubles; never released (small)
      tile_stats[o.out] = TileStats{o.stats, tpi};
    }
    o.cls = o.cp.taps == 1 ? CSD_PROF_CONV1X1 : ((stride == 1 && !up) ? CSD_PROF_CONV3X3 : CSD_PROF_CONV3X3_RESAMPLE);
    pl.ops.push_back(o);
    ar.release(hi16);      // (plan-time lifetimes: the planes die right after this conv)
    ar.release(lo16);
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
    pl.ops.push_back(o);
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
    gn(x0, x1, c0, c1, hw, mname(m.idx, "GroupNorm_0.weight"), mname(m.idx, "GroupNorm_0.bias"));
    const size_t tcol = n.cfg.conditional ? (size_t)n.dense_col.at(m.idx) : NONE;
    const size_t h1 = conv(k + ".Conv_0", {.src0 = x0, .src1 = x1, .ih = hw_side, .iw = hw_side, .pad = 1, .norm = true, .act = n.cfg.act, .temb_col = tcol});
    gn(h1, NONE, m.cout, 0, hw, mname(m.idx, "GroupNorm_1.weight"), mname(m.idx, "GroupNorm_1.bias"));
    pending_scale = skip_scale();
    next_out = out_to;
    const size_t out = conv(k + ".Conv_1", {.src0 = h1, .ih = hw_side, .iw = hw_side, .pad = 1, .norm = true, .act = n.cfg.act, .residual = shortcut});
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
    pl.ops.push_back(o);
    pl.launches += 1;
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
    pl.ops.push_back(o);
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
    pl.ops.push_back(o);
    pl.launches += 1;
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
      pl.ops.push_back(o);
      pl.launches += 1;
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
    gn(h1, NONE, m.cout, 0, os * os, mname(m.idx, "GroupNorm_1.weight"), mname(m.idx, "GroupNorm_1.bias"));
    const size_t sc = conv(k + ".Conv_2", {.src0 = xr, .ih = os, .iw = os});
    ar.release(xr);
    pending_scale = skip_scale();
    const size_t out = conv(k + ".Conv_1", {.src0 = h1, .ih = os, .iw = os, .pad = 1, .norm = true, .act = n.cfg.act, .residual = sc});
    ar.release(h1);
    ar.release(sc);
    return out;
  }

  size_t attn_block(const Module& m, size_t x, int hw_side, size_t out_to = NONE) {
    const std::string k = std::to_string(m.idx);
    const int C = m.cin, L = hw_side * hw_side;
    gn(x, NONE, C, 0, L, mname(m.idx, "GroupNorm_0.weight"), mname(m.idx, "GroupNorm_0.bias"));
    const size_t qkv = conv(k + ".qkv", {.src0 = x, .ih = hw_side, .iw = hw_side, .norm = true});
    Op a;
    a.kind = OP_ATTN;
    a.src0 = qkv; a.hw = L; a.C0 = C;
    a.out = alloc_((size_t)B * L * C);
    a.cls = CSD_PROF_ATTENTION;
    pl.ops.push_back(a);
    count(4.0 * B * (double)L * L * C, 0);
    pending_scale = skip_scale();
    next_out = out_to;
    const size_t o = conv(k + ".NIN_3", {.src0 = a.out, .ih = hw_side, .iw = hw_side, .residual = x});
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
    pl.ops.push_back(e);
    Op a;
    a.kind = OP_LINEAR;
    a.src0 = e.out; a.out = alloc_((size_t)B * 4 * nf);
    a.pk_w = n.copy_off.at(mname(l0.idx, "weight")); a.pk_b = n.copy_off.at(mname(l0.idx, "bias"));
    a.C0 = l0.cin; a.Cout = 4 * nf; a.act = CSD_ACT_NONE; a.out_act = c.act;
    pl.ops.push_back(a);
    Op b2;
    b2.kind = OP_LINEAR;
    b2.src0 = a.out; b2.out = alloc_((size_t)B * 4 * nf);
    b2.pk_w = n.copy_off.at(mname(l1.idx, "weight")); b2.pk_b = n.copy_off.at(mname(l1.idx, "bias"));
    b2.C0 = 4 * nf; b2.Cout = 4 * nf; b2.act = CSD_ACT_NONE; b2.out_act = c.act;
    pl.ops.push_back(b2);
    Op d;
    d.kind = OP_LINEAR;   // every block's Dense_0(act(temb)) in one launch
    d.src0 = b2.out; d.out = alloc_((size_t)B * n.dense_total);
    d.pk_w = n.dense_all_off; d.pk_b = n.dense_all_bias_off;
    d.C0 = 4 * nf; d.Cout = n.dense_total; d.act = CSD_ACT_NONE;
    pl.ops.push_back(d);
    dense_all = d.out;
    pl.launches += 4;
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
    pl.ops.push_back(p);
    pl.launches += 1;
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
  const int S = c.image_size, last = c.n_levels - 1, channels = c.x_channels + c.y_channels;
  const int pin = pp ? c.progressive_input : 0;
  int cmax = c.nf;
  for (auto& m : n.mods) cmax = std::max(cmax, std::max(m.cin, m.cout));
  bd.gn_scratch(B, 0, cmax);

  // ---- input assembly: a launch of its own unless the fused first layer reads x, y itself (the NCSN++ input pyramid reads the tensor) ----
  const Module& stem_m = *std::find_if(n.mods.begin(), n.mods.end(), [](const Module& m) { return m.role == R_STEM; });
  const PackedConv& stem_pc = n.pconvs[n.pconv_by_name.at(std::to_string(stem_m.idx))];
  size_t as_out = NONE;
  const bool fused_stem = stem_pc.kernel == ConvKernel::STEM;
  if (!fused_stem || pin != 0) {
    Op as;
    as.kind = OP_ASSEMBLE;
    as.out = as_out = bd.alloc_((size_t)B * S * S * n.in_cpad);
    pl.ops.push_back(as);
    pl.launches += 1;
  }

  // ---- the walk (models/ddpm.py:149-213, models/ncsnpp.py:238-388): one module of Net::mods at a time on the Builder's CURRENT batch ----
  std::vector<size_t> hs;                        // skip stack
  size_t h = NONE;                               // the current tensor
  bool h_on_stack = true;                        // ... is hs.back(): its consumer must not release it
  size_t pyr_in = pin != 0 ? as_out : NONE;      // NCSN++ input pyramid (level 0: the in_cpad-channel padded NHWC input)
  int pyr_side = S, pyr_pix = n.in_cpad;
  size_t pyr = NONE, pyr_up = NONE;              // NCSN++ output pyramid [B, side, side, channels] of the level below / its FIR upsampling
  // (out_to: the module writes there instead of into a tensor of its own - a batch chunk's slice of the region's output)
  auto step = [&](const Module& m, size_t out_to) {
    const std::string k = std::to_string(m.idx);
    size_t o = NONE, sk = NONE;
    switch (m.role) {
      case R_EMB_FOURIER: case R_EMB_LINEAR0:
        return;                                  // (planned with the MLP's last module)
      case R_EMB_LINEAR1:
        bd.time_embedding(m);
        return;
      case R_STEM:
        o = fused_stem ? bd.stem(stem_pc, m, S) : bd.conv(k, {.src0 = as_out, .ih = S, .iw = S, .pad = 1, .real_cin = channels});
        if (!pp) { bd.ar.release(as_out); as_out = NONE; }      // (NCSN++ keeps it for the input pyramid: released behind the down path)
        break;
      case R_MID_RES_IN:                         // the down path is done: the input pyramid and the assembled input die here
        if (pin == 1 && pyr_in != as_out) bd.ar.release(pyr_in);
        bd.ar.release(as_out);
        [[fallthrough]];
      case R_DOWN_BLOCK: case R_MID_RES_OUT: case R_UP_BLOCK:
        if (m.skip) { sk = hs.back(); hs.pop_back(); }
        o = bd.res_block(m, h, sk, m.cin - m.skip, m.skip, m.side, out_to);
        break;
      case R_ATTN: case R_MID_ATTN:
        o = bd.attn_block(m, h, m.side, out_to);
        break;
      case R_DOWNSAMPLE:
        o = m.kind == M_RES ? bd.res_block_updown(m, h, m.side)
          : c.resamp_with_conv ? bd.conv(k + ".Conv_0", {.src0 = h, .ih = m.side, .iw = m.side, .stride = 2})
                               : bd.resample_plain(OP_AVGPOOL, h, m.side, m.cin, m.out_side);
        break;
      case R_UPSAMPLE:
        o = m.kind == M_RES ? bd.res_block_updown(m, h, m.side)
          : c.resamp_with_conv ? bd.conv(k + ".Conv_0", {.src0 = h, .ih = m.side, .iw = m.side, .pad = 1, .up = 1})
                               : bd.resample_plain(OP_UPNEAR, h, m.side, m.cin, m.out_side);
        break;
      case R_COMBINE: {                          // pyramid_downsample (FIR, no conv), then Combine 'sum' (layerspp.py:53-57): Conv_0(input_pyramid) + h
        const size_t pn = bd.fir(pyr_in, pyr_side, n.in_cpad, false);
        if (pyr_in != as_out) bd.ar.release(pyr_in);
        pyr_in = pn;
        pyr_side /= 2;
        o = bd.conv(k + ".Conv_0", {.src0 = pyr_in, .ih = m.side, .iw = m.side, .residual = h, .real_cin = channels});
        break;
      }
      case R_PYR_DOWN:
        // 'residual': input_pyramid = Downsample(input_pyramid); h = (input_pyramid + h) * skip scale; input_pyramid = h.  From level 1
        // on the source is the previous level's combined h, a live skip-stack entry: the up path releases it, never this one
        o = bd.pyr_conv(m, pyr_in, pyr_pix, m.side, h);
        pyr_in = o; pyr_pix = m.cout;
        break;
      case R_PYR_GN: case R_HEAD_GN:
        if (pyr != NONE) {
          pyr_up = bd.fir(pyr, m.side / 2, channels, true);      // pyramid_upsample
          bd.ar.release(pyr);
        }
        bd.gn(h, NONE, m.cin, 0, m.side * m.side, mname(m.idx, "weight"), mname(m.idx, "bias"));
        return;
      case R_PYR_CONV: case R_HEAD_CONV:         // (level 0: straight to the caller's NCHW output, pyr = NONE)
        pyr = bd.conv(k, {.src0 = h, .ih = m.side, .iw = m.side, .pad = 1, .norm = true, .act = c.act, .residual = pyr_up,
                          .external_nchw = m.level == 0});
        bd.ar.release(pyr_up);
        pyr_up = NONE;
        return;
    }
    if (!h_on_stack) bd.ar.release(h);
    bd.ar.release(sk);
    h = o;
    h_on_stack = m.push;
    if (m.push) hs.push_back(h);
  };

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
    if (i != i_lo) { step(n.mods[i], NONE); continue; }
    const int side0 = S >> l0, Bc = cdiv(B, K);
    const size_t in_full = hs.back();                   // [B, side0, side0, ch]: the Downsample output that enters level l0
    const size_t in_ps = (size_t)side0 * side0 * n.mods[i_lo].cin, out_ps = (size_t)side0 * side0 * n.mods[i_hi].cout;
    const size_t dense_full = bd.dense_all, gp_full = bd.gn_partial, ns_full = bd.nscale, nh_full = bd.nshift;
    std::vector<size_t> hs_main;
    hs_main.swap(hs);
    auto tile_stats_main = bd.tile_stats;
    Arena ar_main = bd.ar;
    // one chunk's walk in the Builder's current arena
    auto chunk_walk = [&](int b0, int nb, size_t out_slice) {
      bd.B = nb;
      bd.tile_stats.clear();
      hs.assign(1, in_full + (size_t)b0 * in_ps);
      h = hs.back(); h_on_stack = true;
      bd.dense_all = dense_full == NONE ? NONE : dense_full + (size_t)b0 * n.dense_total;
      bd.gn_scratch(nb, l0, cmax);                      // the chunk's own GroupNorm scratch
      for (size_t j = i_lo; j <= i_hi; ++j) step(n.mods[j], j == i_hi ? out_slice : NONE);
      return bd.rc;
    };
    // dry run of one full-size chunk: the size of a chunk's private block
    size_t chunk_floats = 0;
    {
      const size_t nops = pl.ops.size();
      const int64_t launches = pl.launches;
      const double flops = pl.flops, bytes = pl.bytes;
      bd.ar = Arena(0);
      const int rc = chunk_walk(0, Bc, 0);
      chunk_floats = (bd.ar.peak() + 63) / 64 * 64;
      pl.ops.resize(nops);
      pl.launches = launches; pl.flops = flops; pl.bytes = bytes;
      bd.next_out = NONE;
      if (rc) return rc;
    }
    bd.ar = ar_main;
    const size_t out_full = bd.alloc_((size_t)B * out_ps);
    const size_t block = bd.alloc_((size_t)K * chunk_floats);
    ar_main = bd.ar;
    {
      Op f;
      f.kind = OP_FORK;
      f.n_chunks = K;
      pl.ops.push_back(f);
    }
    for (int k = 0; k < K; ++k) {
      const int b0 = k * Bc, nb = std::min(Bc, B - b0);
      if (nb <= 0) break;
      const size_t i0 = pl.ops.size();
      bd.ar = Arena(block + (size_t)k * chunk_floats);
      const int rc = chunk_walk(b0, nb, out_full + (size_t)b0 * out_ps);
      if (rc) return rc;
      CSD_REQUIRE(bd.ar.peak() <= chunk_floats, "unet: a chunk outgrew its block");
      for (size_t j = i0; j < pl.ops.size(); ++j) { pl.ops[j].nb = nb; pl.ops[j].stream = k; pl.ops[j].chunk = k + 1; }
    }
    {
      Op j;
      j.kind = OP_JOIN;
      j.n_chunks = K;
      pl.ops.push_back(j);
    }
    // back in the full batch
    bd.ar = ar_main;
    bd.B = B;
    bd.tile_stats = tile_stats_main;
    bd.tile_stats.erase(out_full);
    bd.dense_all = dense_full; bd.gn_partial = gp_full; bd.nscale = ns_full; bd.nshift = nh_full;
    hs.swap(hs_main);
    bd.ar.release(block);
    bd.ar.release(hs.back());      // the region's input: consumed by every chunk's last up block
    hs.pop_back();
    h = out_full; h_on_stack = false;
    i = i_hi;
  }
  bd.ar.release(h);
  if (bd.rc) return bd.rc;
  CSD_REQUIRE(hs.empty(), "unet: the skip stack is not empty behind the last module");
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
