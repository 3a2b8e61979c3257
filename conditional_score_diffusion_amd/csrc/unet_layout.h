// unet_layout.h - the packed-weight buffer of a network: which kernel every layer runs on and where its weights live (build_packed_layout),
// and the packing itself (pack_all).  Included by unet.hip.
#pragma once

namespace csd {

// ---- packed layout ------------------------------------------------------------------------------
static int proto_conv(ConvPlan* p, int c0, int c1, int cout, int taps) {
  memset(p, 0, sizeof(*p));
  p->B = 1; p->IH = p->IW = p->OH = p->OW = 32;   // placeholder geometry: only channel fields matter
  p->C0 = c0; p->C1 = c1; p->Cout = cout; p->taps = taps;
  p->stride = 1; p->pad = taps == 9 ? 1 : 0; p->up = 0;
  return conv_plan_tiles(p);
}

static int build_packed_layout(Net& n) {
  size_t off = 0;
  auto take = [&](size_t nfl) { size_t o = off; off += (nfl + 63) / 64 * 64; return o; };
  auto add_copy = [&](const std::string& pname) {
    const int pi = n.P(pname);
    Net::Copy cpy{pi, take((size_t)n.params[pi].numel)};
    n.copies.push_back(cpy);
    n.copy_off[pname] = cpy.off;
  };
  const int net_ns = precision_ns(n.cfg.precision);
  // the 6 -> nf stem: with the input padded to 16 channels (zeros) it runs on the fp16 matrix cores like every other 3x3 (one K step
  // per tap) instead of the fp32 ones (36 MFMAs of 64 cycles per 32 pixels: 380 us per evaluation at 160^2, B = 64, MFMA-bound)
  if (n.cfg.arch == 0 && net_ns && !CSD_TUNE_ENV("CSD_STEM_F32")) n.in_cpad = 16;
  // more than 8 assembled channels (both families: 9 .. CSD_MAX_IO_CHANNELS): the next multiple of 16 in every precision - the fp32
  // kernel's and the fp16 kernels' K chunk alike.  Everything that reads the assembled tensor or packs the first layer's weights takes
  // its width from in_cpad: OP_ASSEMBLE and its buffer (unet_plan.h), the first layer's proto / pack below (zero weights for the padding
  // channels), stem.hip's own padding (stem_cpad: the same wide_cpad)
  if (n.cfg.x_channels + n.cfg.y_channels > 8) n.in_cpad = wide_cpad(n.cfg.x_channels + n.cfg.y_channels);
  // quad schedule: measured faster than the loader/consumer one in the split (3-MFMA) mode only
  const bool use_q = net_ns == 2 && !CSD_TUNE_ENV("CSD_NO_Q");
  int cur_res = n.cfg.image_size;    // resolution of the layer being laid out
  // opt-in experiment (measured slower: one loader wave cannot convert a patch as fast as three waves consume it)
  const bool fused_norm = CSD_TUNE_ENV("CSD_FUSED_NORM") != nullptr;
  // what build_packed_layout knows about a convolution when it picks the kernel
  struct ConvSpec {
    int c0 = 0, c1 = 0, cout = 0, taps = 9;        // reads (c0 | c1) channels
    std::vector<PackedConv::Src> srcs;
    bool normed = false;         // a GroupNorm in front (or, in an NCSN++ up / down block, its FIR-resampled activation): quad-eligible
    bool resample = false;       // reads a resampled map: Downsample / Upsample, Conv_0 of an NCSN++ up / down block
    bool upsample = false;       // the nearest-x2 Upsample conv
    bool last = false;           // the network's last layer / an output-pyramid conv: a handful of couts
  };
  auto add_conv = [&](const std::string& key, const ConvSpec& sp) -> int {
    const int c0 = sp.c0, c1 = sp.c1, cout = sp.cout, taps = sp.taps;
    const std::vector<PackedConv::Src>& srcs = sp.srcs;
    const bool normed = sp.normed, resample = sp.resample, upsample = sp.upsample, last = sp.last;
    PackedConv pc;
    int rc;
    if (last && net_ns && taps == 9 && c1 == 0 && srcs.size() == 1 && srcs[0].layout == 0 && srcs[0].cout_off == 0 &&
        (srcs[0].cin_src <= 0 || srcs[0].cin_src == c0) && n.cfg.act == CSD_ACT_SWISH && pw16_taps_supported(c0, cout, net_ns)) {
      // the network's last layer (nf -> 3 channels): one pointwise contraction to 27 tap-partial channels + a gather (conv_pw16.hip).
      // SiLU networks only: it is the one activation pw16_kernel's prologue applies; any other head takes the ordinary 3x3 path below
      if ((rc = proto_conv(&pc.proto, c0, 0, pw16_taps_cout(cout), 1))) return rc;
      pc.ns = net_ns;
      pc.kernel = ConvKernel::PW16_TAPS;
      pc.tap_cout = cout;
      pc.w_off = take(pw16_packed_bytes(pc.proto, pc.ns) / sizeof(float) + 1);
      pc.b_off = take((size_t)pc.proto.CoutPad + 96);
      pc.srcs = srcs;
      n.pconv_by_name[key] = (int)n.pconvs.size();
      n.pconvs.push_back(pc);
      return CSD_OK;
    }
    rc = proto_conv(&pc.proto, c0, c1, cout, taps);
    if (rc) return rc;
    // the 5 x 5 level on the quad schedule: 32-cout groups (conv_f16_q.hip: q_ntq)
    static const int nt1_res = CSD_TUNE_ENV("CSD_Q_NT1_RES") ? atoi(CSD_TUNE_ENV("CSD_Q_NT1_RES")) : 5;      // tuning aid (0 disables)
    if (net_ns == 2 && normed && !resample && cur_res <= nt1_res) pc.proto.qnt = 1;
    ConvPlan one = pc.proto;       // a GroupNorm-ed conv reads ONE fp16 tensor of c0 + c1 channels
    one.C0 = c0 + c1; one.C1 = 0;
    // high-resolution GroupNorm-ed convs run the loader/consumer schedule with the norm fused into its loader
    // (standard fragment layout); the quad schedule serves the lower levels, whose tiles straddle samples
    // (fp16 mode: the loader/consumer schedule wins on the GroupNorm-ed convs, the quad schedule on the resampling ones,
    // which would otherwise convert fp32 -> fp16 inside the old kernel's staging loop)
    const bool q_here = use_q || (net_ns == 1 && resample && !CSD_TUNE_ENV("CSD_NO_Q"));
    // fused-prologue schedule: GroupNorm-ed stride-1 convs whose 16 x 16 tiles lie inside one sample (reads the fp32 residual
    // stream itself: the gn_apply16 pass and its fp16 planes disappear)
    ConvPlan ffp = pc.proto;
    ffp.IH = ffp.IW = ffp.OH = ffp.OW = cur_res;
    // (NCSN++ up / down blocks: Conv_0 reads FIR(act(GroupNorm(x))) - an fp32 tensor that is already normalised and activated, so the same
    // kernel takes it with its NORM = false prologue (plain split; the values stay far inside e4m3): no split pass, no fp16 planes)
    const bool fir_act_input = resample && !upsample && normed && n.cfg.arch == 1;
    const int ff_ns = n.cfg.precision == CSD_PREC_F16F8 ? 3 : net_ns;      // 3: fp16 hi*hi + fp8 corrections (conv_ff.hip)
    if (net_ns && normed && (!resample || fir_act_input) && n.cfg.act == CSD_ACT_SWISH && convff_supported(ffp, ff_ns)) {
      pc.ns = ff_ns;
      pc.kernel = ConvKernel::FUSED;
      pc.proto.KC = 16;
      pc.w_off = take(convff_packed_bytes(pc.proto, pc.ns) / sizeof(float) + 1);
    } else if (q_here && normed && !(fused_norm && cur_res >= 64) && conv16q_supported(one, net_ns)) {
      // 3: fp16 hi*hi + fp8 corrections - for GroupNorm-ed operands only: e4m3 saturates at 448, which activated, normalised values never
      // reach, while the raw residual stream that the resampling convs read does at the large-sigma end of a sampling run (measured: the
      // 1000-step trajectory error went from 6e-7 to 1e-4 with them included)
      pc.ns = (n.cfg.precision == CSD_PREC_F16F8 && net_ns == 2 && !resample && conv16q_supported(one, 3)) ? 3 : net_ns;
      pc.proto.KC = 16;
      const bool up4 = upsample && srcs.size() == 1 && conv16q_up4_supported(one, pc.ns);
      pc.kernel = up4 ? ConvKernel::QUAD_UP4 : ConvKernel::QUAD;
      pc.w_off = take((up4 ? conv16q_up4_packed_bytes(one, pc.ns) : conv16q_packed_bytes(one, pc.ns)) / sizeof(float) + 1);
    } else if (net_ns && conv16_supported(pc.proto)) {
      pc.ns = net_ns;
      pc.kernel = ConvKernel::F16_LC;
      if ((rc = conv16_plan_tiles(&pc.proto, pc.ns))) return rc;
      pc.w_off = take(conv16_packed_bytes(pc.proto, pc.ns) / sizeof(float) + 1);
    } else if (net_ns && pw16_supported(pc.proto, net_ns)) {
      bool aligned = true;
      for (const auto& sr : srcs) aligned = aligned && (sr.cout_off % 16 == 0);
      if (aligned) {
        pc.ns = net_ns;
        pc.kernel = ConvKernel::PW16;
        pc.w_off = take(pw16_packed_bytes(pc.proto, pc.ns) / sizeof(float) + 1);
      } else {      // (a source at an unaligned cout_off: the fp32 kernel)
        pc.w_off = take(conv_packed_floats(pc.proto));
      }
    } else {
      pc.w_off = take(conv_packed_floats(pc.proto));
    }
    pc.b_off = take((size_t)pc.proto.CoutPad + 96);
    pc.srcs = srcs;
    n.pconv_by_name[key] = (int)n.pconvs.size();
    n.pconvs.push_back(pc);
    return CSD_OK;
  };
  const csd_unet_config& c = n.cfg;
  const bool pp = c.arch == 1;
  // the first layer of both families in the fp16 modes: input assembly + 3x3 conv + the next GroupNorm's partials as one launch (stem.hip)
  auto stem_layout = [&](Module& m) -> bool {
    if (!(net_ns && m.cin == c.x_channels + c.y_channels && stem_planned(c.x_channels, c.y_channels, m.cout, c.image_size, net_ns)))
      return false;
    // (x_squeeze on the <= 8 channel kernel: its SQ variant covers ONE squeezed image channel, x_channels = 4 - the 4 + 1 .. 4 + 4
    // networks - in the split-operand modes; 8 + 0 and the plain fp16 mode keep the assemble pass + generic convolution)
    if (c.x_squeeze && c.x_channels + c.y_channels <= 8 && (c.x_channels != 4 || net_ns < 2)) return false;
    // (y_scale: the YS variant of the <= 8 channel kernel holds up to 4 x channels and the four taps of up to 4 y channels; other
    // splits keep the assemble pass)
    if (c.y_scale && (c.y_channels > 4 || c.x_channels > 4)) return false;
    // (NCSN++ above 8 channels keeps the assemble pass + generic convolution: with an input pyramid the assembled tensor is written
    // anyway, and on the network stem_wide_kernel measured no faster - 14.37 against 14.36 / 14.44 ms per evaluation at 9 + 3 -> 128
    // channels, 80^2, B = 64, DESIGN.md 4d.  A wide NCSN++ WITHOUT an input pyramid, where the fused layer would also save the assemble
    // launch, has not been measured and keeps the same plan until it is; the tuning switch CSD_PP_WIDE_STEM is the other side of
    // that measurement)
    if (pp && c.x_channels + c.y_channels > 8 && !CSD_TUNE_ENV("CSD_PP_WIDE_STEM")) return false;
    PackedConv pc;
    if (proto_conv(&pc.proto, n.in_cpad, 0, m.cout, 9)) return false;
    pc.ns = net_ns;
    pc.kernel = ConvKernel::STEM;
    pc.w_off = take(stem_packed_bytes(m.cin, m.cout, net_ns) / sizeof(float) + 1);
    pc.b_off = take((size_t)pc.proto.CoutPad + 96);
    pc.srcs = {{n.P(mname(m.idx, "weight")), n.P(mname(m.idx, "bias")), 0, m.cout, 0, m.cin}};
    n.pconv_by_name[std::to_string(m.idx)] = (int)n.pconvs.size();
    n.pconvs.push_back(pc);
    return true;
  };
  // ResnetBlockDDPM / ResnetBlockBigGANpp reading (c0 | c1) channels
  auto res_layout = [&](Module& m, int c0, int c1) -> int {
    const std::string k = std::to_string(m.idx);
    const bool plain = !m.up && !m.down;
    add_copy(mname(m.idx, "GroupNorm_0.weight"));
    add_copy(mname(m.idx, "GroupNorm_0.bias"));
    // Conv_0 reads the GroupNorm-ed input directly only in plain blocks; up/down blocks feed it the FIR-resampled
    // activation (an fp32 tensor without a norm)
    int r = add_conv(k + ".Conv_0", {.c0 = c0, .c1 = c1, .cout = m.cout,
                                     .srcs = {{n.P(mname(m.idx, "Conv_0.weight")), n.P(mname(m.idx, "Conv_0.bias")), 0, m.cout, 0}},
                                     .normed = true,      // (up/down blocks: quad-eligible, a plain split of the resampled tensor)
                                     .resample = !plain});
    if (r) return r;
    add_copy(mname(m.idx, "GroupNorm_1.weight"));
    add_copy(mname(m.idx, "GroupNorm_1.bias"));
    r = add_conv(k + ".Conv_1", {.c0 = m.cout, .cout = m.cout,
                                 .srcs = {{n.P(mname(m.idx, "Conv_1.weight")), n.P(mname(m.idx, "Conv_1.bias")), 0, m.cout, 0}},
                                 .normed = true});
    if (r) return r;
    if (m.cin != m.cout || !plain) {      // shortcut: NIN_0 (W [in, out]) / NCSN++ Conv_2 (1x1, OIHW)
      r = pp ? add_conv(k + ".Conv_2", {.c0 = c0, .c1 = c1, .cout = m.cout, .taps = 1,
                                        .srcs = {{n.P(mname(m.idx, "Conv_2.weight")), n.P(mname(m.idx, "Conv_2.bias")), 0, m.cout, 0}}})
             : add_conv(k + ".NIN_0", {.c0 = c0, .c1 = c1, .cout = m.cout, .taps = 1,
                                       .srcs = {{n.P(mname(m.idx, "NIN_0.W")), n.P(mname(m.idx, "NIN_0.b")), 1, m.cout, 0}}});
      if (r) return r;
    }
    if (c.conditional) {
      n.dense_col[m.idx] = n.dense_total;
      n.dense_total += m.cout;
    }
    return CSD_OK;
  };
  auto attn_layout = [&](Module& m) -> int {
    const std::string k = std::to_string(m.idx);
    const int C = m.cin;
    add_copy(mname(m.idx, "GroupNorm_0.weight"));
    add_copy(mname(m.idx, "GroupNorm_0.bias"));
    int r = add_conv(k + ".qkv", {.c0 = C, .cout = 3 * C, .taps = 1,
                                  .srcs = {{n.P(mname(m.idx, "NIN_0.W")), n.P(mname(m.idx, "NIN_0.b")), 1, C, 0},
                                           {n.P(mname(m.idx, "NIN_1.W")), n.P(mname(m.idx, "NIN_1.b")), 1, C, C},
                                           {n.P(mname(m.idx, "NIN_2.W")), n.P(mname(m.idx, "NIN_2.b")), 1, C, 2 * C}}});
    if (r) return r;
    return add_conv(k + ".NIN_3", {.c0 = C, .cout = C, .taps = 1,
                                   .srcs = {{n.P(mname(m.idx, "NIN_3.W")), n.P(mname(m.idx, "NIN_3.b")), 1, C, 0}}});
  };
  auto resample_layout = [&](Module& m) -> int {
    if (!c.resamp_with_conv) return CSD_OK;
    // quad-eligible: plain fp16 split of the source tensor + quad schedule (x2 addressing / stride 2: the fp16 kernels also cover the
    // stride-2 Downsample)
    return add_conv(std::to_string(m.idx) + ".Conv_0",
                    {.c0 = m.cin, .cout = m.cin, .srcs = {{n.P(mname(m.idx, "Conv_0.weight")), n.P(mname(m.idx, "Conv_0.bias")), 0, m.cin, 0}},
                     .normed = true, .resample = true, .upsample = m.kind == M_UP});
  };
  for (Module& m : n.mods) {
    cur_res = (m.up || m.down) ? m.out_side : m.side;      // (a BigGAN up / down block convolves the resampled map)
    const std::string k = std::to_string(m.idx);
    int rc = CSD_OK;
    switch (m.role) {
      case R_EMB_FOURIER:
        add_copy(mname(m.idx, "W"));
        break;
      case R_EMB_LINEAR0: case R_EMB_LINEAR1: case R_PYR_GN: case R_HEAD_GN:
        add_copy(mname(m.idx, "weight"));
        add_copy(mname(m.idx, "bias"));
        break;
      case R_STEM:      // Cin padded to in_cpad (zero weights for the padding channels)
        if (!stem_layout(m))
          rc = add_conv(k, {.c0 = n.in_cpad, .cout = m.cout, .srcs = {{n.P(mname(m.idx, "weight")), n.P(mname(m.idx, "bias")), 0, m.cout, 0, m.cin}}});
        break;
      case R_DOWN_BLOCK: case R_MID_RES_IN: case R_MID_RES_OUT: case R_UP_BLOCK:
        rc = res_layout(m, m.cin - m.skip, m.skip);
        break;
      case R_ATTN: case R_MID_ATTN:
        rc = attn_layout(m);
        break;
      case R_DOWNSAMPLE: case R_UPSAMPLE:
        rc = m.kind == M_RES ? res_layout(m, m.cin, 0) : resample_layout(m);
        break;
      case R_COMBINE:      // 1x1 conv of the (in_cpad-channel padded) input pyramid
        rc = add_conv(k + ".Conv_0", {.c0 = n.in_cpad, .cout = m.cout, .taps = 1,
                                      .srcs = {{n.P(mname(m.idx, "Conv_0.weight")), n.P(mname(m.idx, "Conv_0.bias")), 0, m.cout, 0, m.cin}}});
        break;
      case R_PYR_DOWN:     // the FIR-folded 6x6 stride-2 weight (pack_all folds it) + the raw bias
        n.pyr_fold_off[m.idx] = take((size_t)36 * m.cin * m.cout);
        add_copy(mname(m.idx, pyr_sub(c, true)));
        break;
      case R_PYR_CONV: case R_HEAD_CONV:
        // the network's last layer and the output pyramid's convs: a handful of couts each.  (The DDPM family's head is laid out as a conv
        // without a norm in front and leaves cin_src to its default: where the tap-partial form does not apply, that selects its kernel)
        rc = add_conv(k, {.c0 = m.cin, .cout = m.cout, .srcs = {{n.P(mname(m.idx, "weight")), n.P(mname(m.idx, "bias")), 0, m.cout, 0, pp ? m.cin : 0}},
                          .normed = pp, .last = true});
        break;
    }
    if (rc) return rc;
  }
  if (c.conditional) {
    n.dense_all_off = take((size_t)n.dense_total * 4 * c.nf);
    n.dense_all_bias_off = take((size_t)n.dense_total);
  }
  n.packed_floats = off;
  return CSD_OK;
}

// ---- weight packing -------------------------------------------------------------------------------
__global__ void copy_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}
__global__ void fill_f32_kernel(float* __restrict__ dst, float v, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = v;
}

static int dev_copy(const float* src, float* dst, size_t nfl, hipStream_t s) {
  if (!nfl) return CSD_OK;
  const int grid = (int)std::min<size_t>(cdiv64(nfl, 256), 1024);
  hipLaunchKernelGGL(copy_f32_kernel, dim3(grid), dim3(256), 0, s, src, dst, nfl);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}
static int dev_fill(float* dst, float v, size_t nfl, hipStream_t s) {
  if (!nfl) return CSD_OK;
  const int grid = (int)std::min<size_t>(cdiv64(nfl, 256), 1024);
  hipLaunchKernelGGL(fill_f32_kernel, dim3(grid), dim3(256), 0, s, dst, v, nfl);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}

// every raw fp32 copy of a pack (GroupNorm affine, Linear / Dense weights, conv biases: ~480 of them at the SR3-160 shape) in ONE launch:
// a table of (source, destination offset, count) in device memory, one workgroup row per entry.  As separate launches they were 900
// kernel dispatches per pack - a third of the launches of a four-forward profile of NCSN++-256.
struct CopyDesc { const float* src; float* dst; unsigned long long n; };
__global__ void copy_table_kernel(const CopyDesc* __restrict__ tab) {
  const CopyDesc d = tab[blockIdx.y];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += (size_t)gridDim.x * blockDim.x) d.dst[i] = d.src[i];
}
// the host copy of the table belongs to the handle: the upload is stream-ordered and may still be in flight when pack returns, so the
// next pack waits for the event behind the previous upload before it rewrites the vector (no stream synchronisation in a pack)
static int run_copy_table(Net& n, hipStream_t s);

static int pack_all(Net& n, float* pk, hipStream_t s) {
  for (auto& p : n.params)
    CSD_REQUIRE(p.ptr != nullptr, "pack: parameter '%s' was never registered (csd_unet_set_param)", p.name.c_str());
  int rc;
  if (n.copy_ev) CSD_CHECK_HIP(hipEventSynchronize(n.copy_ev));      // (the previous pack's table upload has left the host vector)
  n.copy_host.clear();
  struct { Net& n; void add(const float* src, float* dst, size_t nfl) { if (nfl) n.copy_host.push_back(CopyDesc{src, dst, (unsigned long long)nfl}); } } batch{n};
  for (auto& cp : n.copies) batch.add(n.params[cp.param].ptr, pk + cp.off, (size_t)n.params[cp.param].numel);
  for (auto& pc : n.pconvs) {
    if ((rc = dev_fill(pk + pc.b_off, 0.f, (size_t)pc.proto.CoutPad, s))) return rc;
    for (auto& src : pc.srcs) {   // sources are listed with ascending cout_off, first one clears the tensor
      const int cin_src = src.cin_src > 0 ? src.cin_src : pc.proto.C0 + pc.proto.C1;
      ConvPlan one = pc.proto;
      one.C0 = pc.proto.C0 + pc.proto.C1; one.C1 = 0;
      const float* w = n.params[src.param_w].ptr;
      float* dst = pk + pc.w_off;
      switch (pc.kernel) {
        case ConvKernel::STEM: rc = stem_pack_weight(w, cin_src, pc.proto.Cout, pc.ns, dst, s); break;
        case ConvKernel::FUSED: rc = convff_pack_weight(pc.proto, pc.ns, w, src.layout, cin_src, src.cout_src, src.cout_off, dst, s); break;
        case ConvKernel::QUAD_UP4: rc = conv16q_pack_weight_up4(one, pc.ns, w, dst, s); break;
        case ConvKernel::QUAD: rc = conv16q_pack_weight(one, pc.ns, w, src.layout, cin_src, src.cout_src, src.cout_off, dst, s); break;
        case ConvKernel::PW16_TAPS: rc = pw16_pack_weight_taps(pc.proto, pc.ns, w, pc.tap_cout, dst, s); break;
        case ConvKernel::PW16: rc = pw16_pack_weight(pc.proto, pc.ns, w, src.layout, cin_src, src.cout_src, src.cout_off, dst, s); break;
        case ConvKernel::F16_LC: rc = conv16_pack_weight(pc.proto, pc.ns, w, src.layout, cin_src, src.cout_src, src.cout_off, dst, s); break;
        case ConvKernel::F32: rc = conv_pack_weight(pc.proto, w, src.layout, cin_src, src.cout_src, src.cout_off, dst, s); break;
      }
      if (rc) return rc;
      batch.add(n.params[src.param_b].ptr, pk + pc.b_off + src.cout_off, (size_t)src.cout_src);      // (behind the fill above: same stream)
    }
  }
  for (auto& m : n.mods) {
    if (m.kind != M_PYR) continue;
    rc = fir_pyr_fold_launch(n.params[n.P(mname(m.idx, pyr_sub(n.cfg, false)))].ptr, m.cin, m.cout,
                             n.cfg.progressive_input == 2 ? n.cfg.fir_kernel : nullptr, pk + n.pyr_fold_off.at(m.idx), nullptr, s);
    if (rc) return rc;
  }
  if (n.cfg.conditional) {
    const int K = 4 * n.cfg.nf;
    for (auto& m : n.mods) {
      if (m.kind != M_RES) continue;
      const int col = n.dense_col.at(m.idx);
      batch.add(n.params[n.P(mname(m.idx, "Dense_0.weight"))].ptr, pk + n.dense_all_off + (size_t)col * K, (size_t)m.cout * K);
      batch.add(n.params[n.P(mname(m.idx, "Dense_0.bias"))].ptr, pk + n.dense_all_bias_off + col, (size_t)m.cout);
    }
  }
  if ((rc = run_copy_table(n, s))) return rc;
  n.packed_once = true;
  return CSD_OK;
}

static int run_copy_table(Net& n, hipStream_t s) {
  if (n.copy_host.empty()) return CSD_OK;
  if (n.copy_tab_cap < n.copy_host.size()) {
    if (n.copy_tab) (void)hipFree(n.copy_tab);
    n.copy_tab = nullptr;
    CSD_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&n.copy_tab), n.copy_host.size() * sizeof(CopyDesc)));
    n.copy_tab_cap = n.copy_host.size();
  }
  if (!n.copy_ev) CSD_CHECK_HIP(hipEventCreateWithFlags(&n.copy_ev, hipEventDisableTiming));
  CSD_CHECK_HIP(hipMemcpyAsync(n.copy_tab, n.copy_host.data(), n.copy_host.size() * sizeof(CopyDesc), hipMemcpyHostToDevice, s));
  CSD_CHECK_HIP(hipEventRecord(n.copy_ev, s));
  size_t longest = 0;
  for (auto& d : n.copy_host) longest = std::max<size_t>(longest, d.n);
  const unsigned gx = (unsigned)std::min<size_t>(cdiv64(longest, 256), 64);
  hipLaunchKernelGGL(copy_table_kernel, dim3(gx, (unsigned)n.copy_host.size()), dim3(256), 0, s, n.copy_tab);
  CSD_LAUNCH_CHECK();
  return CSD_OK;
}
}  // namespace csd
