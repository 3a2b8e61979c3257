// plan_digest.h - csd_unet_debug_digest: 64-bit FNV-1a digests of everything the host side derives from a configuration (a debug export
// like csd_debug_timing: not part of include/csd.h).  tests/test_host_logic.py pins them to tests/golden/plan_digests.json, so a change
// that is meant to leave every packed offset, launch and workspace address alone can prove it without a GPU.  Hashed field by field
// (never raw struct bytes: padding, and Op::cp / Op::gp are only filled for the kinds that use them).
//
// The pinned values date from an Op of lettered slots (offsets a .. e, ints i0 .. i4) and a PackedConv of one flag per kernel.  The hash
// still takes its values in THAT order; legacy_slots / legacy_flags below are the only place that knows it - and the record of what the
// letters used to mean.  The training digest likewise dates from a TStep of ten positional saved-tensor slots: legacy_saved.
#pragma once

namespace csd {

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void raw(const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) { h ^= static_cast<const unsigned char*>(p)[i]; h *= 1099511628211ull; }
  }
  void i(int64_t v) { raw(&v, sizeof(v)); }
  void z(size_t v) { i(v == NONE ? -1 : (int64_t)v); }
  void f(double v) { raw(&v, sizeof(v)); }
  void s(const std::string& v) { i((int64_t)v.size()); raw(v.data(), v.size()); }
  void cp(const ConvPlan& p) {
    for (int v : {p.B, p.IH, p.IW, p.OH, p.OW, p.C0, p.C1, p.Cout, p.taps, p.stride, p.pad, p.up, p.KC, p.NT, p.MT, p.KCS, p.LC, p.TH, p.TW, p.PH,
                  p.PW, p.tiles_x, p.tiles_y, p.n_groups, p.CoutPad, p.qnt}) i(v);
    z(p.lds_bytes);
  }
};

// ---- the pinned order ---------------------------------------------------------------------------------
// PackedConv: ns, then the flags pw, q, ff, tap_cout, stem, up4
struct LegacyFlags { int pw = 0, q = 0, ff = 0, stem = 0, up4 = 0; };
static LegacyFlags legacy_flags(ConvKernel k) {
  LegacyFlags f;
  switch (k) {
    case ConvKernel::F32: case ConvKernel::F16_LC: break;      // (told apart by ns == 0)
    case ConvKernel::PW16: case ConvKernel::PW16_TAPS: f.pw = 1; break;      // (PW16_TAPS: tap_cout != 0)
    case ConvKernel::QUAD: f.q = 1; break;
    case ConvKernel::QUAD_UP4: f.q = 1; f.up4 = 1; break;
    case ConvKernel::FUSED: f.ff = 1; break;
    case ConvKernel::STEM: f.stem = 1; break;
  }
  return f;
}

// Op: the offsets a, b, c, d, e, out, stats, pk0, pk1 and the ints i0 .. i4 of every kind (an unused slot: NONE / 0)
struct LegacySlots {
  size_t a = NONE, b = NONE, c = NONE, d = NONE, e = NONE, out = NONE, stats = NONE, pk0 = NONE, pk1 = NONE;
  int i0 = 0, i1 = 0, i2 = 0, i3 = 0, i4 = 0;
};
static void legacy_stem(const Op& o, LegacySlots& l) {
  l.i0 = o.Cout; l.i4 = o.ns; l.stats = o.stats; l.c = o.out2;
}
static void legacy_embedding(const Op& o, LegacySlots& l) { l.i0 = o.C0; }      // OP_TEMB, OP_FOURIER (pk0 = W)
static void legacy_fir(const Op& o, LegacySlots& l) {      // OP_FIR, OP_FIR2 (d / e: the GroupNorm it applies, c: FIR(x))
  l.a = o.src0; l.d = o.nscale; l.e = o.nshift; l.c = o.out2; l.i0 = o.H; l.i1 = o.C0; l.i2 = o.up;
}
static void legacy_gn_apply32(const Op& o, LegacySlots& l) { l.a = o.src0; l.d = o.nscale; l.e = o.nshift; l.i0 = o.C0; l.i1 = o.hw; }
static void legacy_linear(const Op& o, LegacySlots& l) { l.a = o.src0; l.i0 = o.C0; l.i1 = o.Cout; l.i2 = o.out_act; }
static void legacy_gn_stats(const Op& o, LegacySlots& l) { l.a = o.src0; l.b = o.src1; l.out = o.stats; l.i0 = o.per_channel; }
static void legacy_gn_final(const Op& o, LegacySlots& l) { l.a = o.stats; l.out = o.nscale; l.b = o.nshift; }      // (nshift in b ...)
static void legacy_gn_final_tiles(const Op& o, LegacySlots& l) {                                                     // (... but in c here ...)
  l.a = o.stats; l.i0 = o.tiles0; l.i1 = o.C0; l.b = o.stats1; l.i2 = o.tiles1; l.i3 = o.C1; l.i4 = o.hw; l.out = o.nscale; l.c = o.nshift;
}
static void legacy_gn_statfin(const Op& o, LegacySlots& l) { l.a = o.src0; l.b = o.src1; l.out = o.nscale; l.c = o.nshift; }      // (... and here)
static void legacy_gn_planes16(const Op& o, LegacySlots& l) {      // OP_GN_APPLY16, OP_GN_FUSED16: out / c = the hi / lo plane
  l.a = o.src0; l.b = o.src1; l.i0 = o.C0; l.i1 = o.C1; l.i2 = o.hw; l.d = o.nscale; l.e = o.nshift; l.c = o.out2; l.i3 = o.fp8_lo;
}
static void legacy_conv(const Op& o, LegacySlots& l) {
  l.a = o.src0; l.b = o.src1; l.c = o.res; l.d = o.nscale; l.e = o.nshift; l.stats = o.stats;
  const LegacyFlags f = legacy_flags(o.kernel);
  l.i2 = f.ff ? 3 : (f.pw ? 1 : (f.q ? 2 : 0));      // "kernel id"
  l.i3 = o.src_form == ConvSrc::SPLIT_STAGING ? 2 : (o.src_form == ConvSrc::PLANES16 ? 1 : 0);
  l.i4 = o.ns;
}
static void legacy_attn(const Op& o, LegacySlots& l) { l.a = o.src0; l.i0 = o.hw; l.i1 = o.C0; }
static void legacy_resample_plain(const Op& o, LegacySlots& l) { l.a = o.src0; l.i0 = o.H; l.i1 = o.C0; }      // OP_AVGPOOL, OP_UPNEAR
static void legacy_pyrconv(const Op& o, LegacySlots& l) {
  l.a = o.src0; l.c = o.res; l.i0 = o.H; l.i1 = o.C0; l.i2 = o.Cout; l.i3 = o.pix; l.i4 = o.fir;
}
static void legacy_tapsum(const Op& o, LegacySlots& l) { l.a = o.src0; l.c = o.res; l.i0 = o.H; l.i1 = o.W; l.i2 = o.Cout; }
static LegacySlots legacy_slots(const Op& o) {
  LegacySlots l;
  l.out = o.out;      // (the kinds that write partial sums or scale / shift have no `out`: theirs went into this slot)
  l.pk0 = o.pk_w; l.pk1 = o.pk_b;
  switch (o.kind) {
    case OP_ASSEMBLE: case OP_TO_NCHW: break;
    case OP_STEM: legacy_stem(o, l); break;
    case OP_TEMB: case OP_FOURIER: legacy_embedding(o, l); break;
    case OP_FIR: case OP_FIR2: legacy_fir(o, l); break;
    case OP_GN_APPLY32: legacy_gn_apply32(o, l); break;
    case OP_LINEAR: legacy_linear(o, l); break;
    case OP_GN_STATS: legacy_gn_stats(o, l); break;
    case OP_GN_FINAL: legacy_gn_final(o, l); break;
    case OP_GN_FINAL_TILES: legacy_gn_final_tiles(o, l); break;
    case OP_GN_STATFIN: legacy_gn_statfin(o, l); break;
    case OP_GN_APPLY16: case OP_GN_FUSED16: legacy_gn_planes16(o, l); break;
    case OP_CONV: legacy_conv(o, l); break;
    case OP_ATTN: legacy_attn(o, l); break;
    case OP_AVGPOOL: case OP_UPNEAR: legacy_resample_plain(o, l); break;
    case OP_PYRCONV: legacy_pyrconv(o, l); break;
    case OP_TAPSUM: legacy_tapsum(o, l); break;
    case OP_FORK: case OP_JOIN: l.i0 = o.n_chunks; break;
  }
  return l;
}

static uint64_t digest_params(const Net& n) {
  Fnv h;
  for (const Param& p : n.params) { h.s(p.name); h.i(p.ndim); for (int j = 0; j < 4; ++j) h.i(p.shape[j]); }      // (4: arch 0 / 1 have no 5-D parameter)
  return h.h;
}

static uint64_t digest_layout(const Net& n) {
  Fnv h;
  for (const auto& kv : n.pconv_by_name) {
    const PackedConv& pc = n.pconvs[kv.second];
    h.s(kv.first); h.i(kv.second); h.z(pc.w_off); h.z(pc.b_off);
    const LegacyFlags f = legacy_flags(pc.kernel);
    for (int v : {pc.ns, f.pw, f.q, f.ff, pc.tap_cout, f.stem, f.up4, pc.proto.C0, pc.proto.C1, pc.proto.Cout,
                  pc.proto.taps, pc.proto.KC, pc.proto.NT, pc.proto.CoutPad, pc.proto.qnt}) h.i(v);
    for (const auto& sr : pc.srcs) for (int v : {sr.param_w, sr.param_b, sr.layout, sr.cout_src, sr.cout_off, sr.cin_src}) h.i(v);
  }
  for (const auto& cpy : n.copies) { h.i(cpy.param); h.z(cpy.off); }
  for (const auto& kv : n.copy_off) { h.s(kv.first); h.z(kv.second); }
  for (const auto& kv : n.pyr_fold_off) { h.i(kv.first); h.z(kv.second); }
  for (const auto& kv : n.dense_col) { h.i(kv.first); h.i(kv.second); }
  h.i(n.dense_total); h.z(n.dense_all_off); h.z(n.dense_all_bias_off); h.z(n.packed_floats); h.i(n.in_cpad);
  return h.h;
}

static uint64_t digest_plan(const Plan& pl) {
  Fnv h;
  for (const Op& o : pl.ops) {
    h.i(o.kind);
    const LegacySlots l = legacy_slots(o);
    for (size_t v : {l.a, l.b, l.c, l.d, l.e, l.out, l.stats, o.temb_base, l.pk0, l.pk1, o.temb_col}) h.z(v);
    for (int v : {l.i0, l.i1, l.i2, l.i3, l.i4, o.act, o.out_external, o.side, o.nb, o.stream, o.chunk, o.temb_stride, o.cls}) h.i(v);
    for (double v : {(double)o.out_scale, o.flops, o.bytes, o.abytes}) h.f(v);
    if (o.kind == OP_CONV) h.cp(o.cp);
    if (o.kind == OP_GN_FINAL_TILES) h.i(o.gp.G);
    if (o.kind == OP_GN_STATS || o.kind == OP_GN_FINAL || o.kind == OP_GN_STATFIN || o.kind == OP_GN_FUSED16)
      for (int v : {o.gp.B, o.gp.HW, o.gp.C0, o.gp.C1, o.gp.G, o.gp.nchunk}) h.i(v);
  }
  h.z(pl.ws_floats); h.i(pl.launches); h.f(pl.flops); h.f(pl.bytes);
  return h.h;
}

// TStep: its saved tensors were ten positional slots sv[0 .. 9]; the pinned hash takes all ten in this order (an unused slot: null)
static std::array<const float*, 10> legacy_saved(const TStep& sp) {
  switch (sp.kind) {
    case TS_RES: return {sp.op0, sp.rs0, sp.ms0, sp.c0, sp.a1, sp.rs1, sp.ms1, sp.mask, sp.xr};
    case TS_ATTN: return {sp.op0, sp.rs0, sp.ms0, sp.qkv, sp.attn};
    case TS_HEAD: case TS_PYR: return {sp.op0, sp.rs0, sp.ms0};
    case TS_COMBINE: return {sp.pyr};
    default: return {};
  }
}

// the training graph's dry run (the one csd_unet_train_workspace_bytes sizes the workspace with); 0: no planned training graph
static uint64_t digest_train(csd_unet* net, int B, float dropout_p) {
  if (train_check(net)) return 0;
  TrainState st;
  float* const base = reinterpret_cast<float*>(uintptr_t(256));
  TG g(net->net, st, B, nullptr, true, nullptr, nullptr, base);
  g.p_drop = dropout_p;
  g.want_dx = true;
  if (g.forward(nullptr, nullptr, nullptr, nullptr) || g.backward(nullptr)) return 0;
  Fnv h;
  auto off = [&](const float* p) { h.i(p ? (int64_t)(p - base) : -1); };
  for (const TStep& sp : st.steps) {
    for (int64_t v : {(int64_t)sp.kind, (int64_t)sp.mod, (int64_t)sp.in0, (int64_t)sp.in1, (int64_t)sp.out, (int64_t)sp.drop_id, (int64_t)sp.flag}) h.i(v);
    for (const float* p : legacy_saved(sp)) off(p);
  }
  for (const TT& t : st.t) { off(t.p); h.i(t.H); h.i(t.C); }
  h.z(st.fwd_top); h.z(g.peak);
  return h.h;
}

}  // namespace csd

// out: (a) parameter table, (b) packed layout, (c) inference plan for B, (d) training dry run for B (0 where there is none)
extern "C" int csd_unet_debug_digest(csd_unet* net, int B, float dropout_p, uint64_t out[4]) {
  CSD_REQUIRE(net && out, "debug_digest: null argument");
  CSD_REQUIRE(net->net.cfg.arch != 2, "debug_digest: the 3-D networks (arch 2) have no digest");
  CSD_REQUIRE(!net->net.cfg.x_squeeze, "debug_digest: a handle with x_squeeze has no digest (its plan is the unsqueezed network's)");
  CSD_REQUIRE(!net->net.cfg.y_scale, "debug_digest: a handle with y_scale has no digest (its plan is the paired network's)");
  Plan* pl = nullptr;
  const int rc = build_plan(net->net, B, &pl);
  if (rc) return rc;
  out[0] = digest_params(net->net);
  out[1] = digest_layout(net->net);
  out[2] = digest_plan(*pl);
  out[3] = digest_train(net, B, dropout_p);
  return CSD_OK;
}
