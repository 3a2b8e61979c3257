// plan_digest.h - csd_unet_debug_digest: 64-bit FNV-1a digests of everything the host side derives from a configuration (a debug export
// like csd_debug_timing: not part of include/csd.h).  tests/test_host_logic.py pins them to tests/golden/plan_digests.json, so a change
// that is meant to leave every packed offset, launch and workspace address alone can prove it without a GPU.  Hashed field by field
// (never raw struct bytes: padding, and Op::cp / Op::gp are only filled for the kinds that use them).
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
    for (int v : {pc.ns, (int)pc.pw, (int)pc.q, (int)pc.ff, pc.tap_cout, (int)pc.stem, (int)pc.up4, pc.proto.C0, pc.proto.C1, pc.proto.Cout,
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
    for (size_t v : {o.a, o.b, o.c, o.d, o.e, o.out, o.stats, o.temb_base, o.pk0, o.pk1, o.temb_col}) h.z(v);
    for (int v : {o.i0, o.i1, o.i2, o.i3, o.i4, o.act, o.out_external, o.side, o.nb, o.stream, o.chunk, o.temb_stride, o.cls}) h.i(v);
    for (double v : {(double)o.fscale, o.flops, o.bytes, o.abytes}) h.f(v);
    if (o.kind == OP_CONV) h.cp(o.cp);
    if (o.kind == OP_GN_FINAL_TILES) h.i(o.gp.G);
    if (o.kind == OP_GN_STATS || o.kind == OP_GN_FINAL || o.kind == OP_GN_STATFIN || o.kind == OP_GN_FUSED16)
      for (int v : {o.gp.B, o.gp.HW, o.gp.C0, o.gp.C1, o.gp.G, o.gp.nchunk}) h.i(v);
  }
  h.z(pl.ws_floats); h.i(pl.launches); h.f(pl.flops); h.f(pl.bytes);
  return h.h;
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
    for (const float* p : sp.sv) off(p);
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
