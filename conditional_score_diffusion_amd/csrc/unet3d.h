// unet3d.h - the 3-D DDPM family (csd_unet_config.arch == 2; reference models/ddpm3D.py:38-196) behind the csd_unet handle: topology and
// parameter table, packed layout + pack, the plan of one batch size and its executor.  Part of unet.hip's translation unit.
//
// The network is the DDPM U-Net on 3x3x3 convolutions without attention: 2x2x2 average-pool downsampling, nearest x2 upsampling, a
// 3x3x3 convolution (Conv_2) as the shortcut of every residual block whose channel count changes.  The plan is the layer list of
// DDPM3D.forward with every buffer at a fixed offset of the caller's workspace; it launches the kernels the per-operator path launches
// (conv3d.hip through conv3d_launch - same Conv3dArgs, brick and NT as csd_conv3d_block -, gn_stats_launch / gn_finalize_launch as
// csd_groupnorm_scale_shift, csd_avgpool3d_2_ndhwc, csd_nearest_up2_3d_ndhwc, timestep_embedding_launch, linear_launch) with the weights
// packed ONCE by csd_unet_pack, so an evaluation is bitwise the operator path's.  Two things differ in form, not in value: the input
// boundary (cat, 2v - 1, NCDHW -> NDHWC) is fused into the stem convolution (conv3d_stem_kernel, the direct kernel's fmaf chain), and all
// Dense_0 projections of an evaluation are one linear launch over concatenated weights (each output element's arithmetic is unchanged).
// One stream, no atomics, a fixed order: repeatable and independent of the batch position.
#pragma once

namespace csd {

static inline bool is3d(const Net& n) { return n.cfg.arch == 2; }
// elements of one channel of one sample: what the PC loop's sizes are multiples of
static inline size_t sample_elems(const csd_unet_config& c) {
  return c.arch == 2 ? (size_t)c.vol[0] * c.vol[1] * c.vol[2] : (size_t)c.image_size * c.image_size;
}

// ---- module list + parameter table: DDPM3D.__init__ (models/ddpm3D.py:56-105) ----------------------------------------------------------
static int build_modules3d(Net& n) {
  const csd_unet_config& c = n.cfg;
  CSD_REQUIRE(c.n_levels >= 1 && c.n_levels <= CSD_MAX_LEVELS, "unet 3-D: bad n_levels %d", c.n_levels);
  CSD_REQUIRE(!c.resamp_with_conv, "unet 3-D: resamp_with_conv is not provided - the reference fails there too (its Upsample builds a 2-D "
                                   "convolution, its Downsample pads 2 of the 3 dimensions)");
  CSD_REQUIRE(c.conditional, "unet 3-D: conditional = 0 is not provided - the reference's module list only exists under `if conditional`");
  CSD_REQUIRE(c.nf >= 32 && c.nf % 32 == 0, "unet 3-D: nf = %d is not divisible into the 32 GroupNorm groups", c.nf);
  CSD_REQUIRE(c.precision == CSD_PREC_F32 || c.precision == CSD_PREC_F16X3,
              "unet 3-D: precision must be fp32 (CSD_PREC_F32) or fp16x3 (CSD_PREC_F16X3); fp16 and fp16f8 are not provided in 3-D");
  CSD_REQUIRE(c.act >= CSD_ACT_SWISH && c.act <= CSD_ACT_ELU, "unet 3-D: bad activation id %d", c.act);
  CSD_REQUIRE(c.num_res_blocks >= 1, "unet 3-D: bad num_res_blocks %d", c.num_res_blocks);
  CSD_REQUIRE(c.x_channels >= 1 && c.y_channels >= 0 && c.x_channels + c.y_channels <= 8, "unet 3-D: x + y channels must be in 1 .. 8");
  CSD_REQUIRE(c.out_channels >= 1 && c.out_channels <= 32, "unet 3-D: out_channels %d not in 1 .. 32", c.out_channels);
  for (int l = 0; l < c.n_levels; ++l) CSD_REQUIRE(c.ch_mult[l] >= 1, "unet 3-D: bad ch_mult[%d] = %d", l, c.ch_mult[l]);
  for (int a = 0; a < 3; ++a) CSD_REQUIRE(c.vol[a] >= 1, "unet 3-D: volume %d x %d x %d has an extent below 1", c.vol[0], c.vol[1], c.vol[2]);
  for (int l = 0; l + 1 < c.n_levels; ++l)
    for (int a = 0; a < 3; ++a)
      CSD_REQUIRE((c.vol[a] >> l) >= 2 && (c.vol[a] >> l) % 2 == 0,
                  "unet 3-D: volume %d x %d x %d has an odd extent (or one below 2) at level %d, which the 2x2x2 average pool cannot halve",
                  c.vol[0], c.vol[1], c.vol[2], l);
  const int nf = c.nf, channels = c.x_channels + c.y_channels, last = c.n_levels - 1;
  auto add = [&](ModKind k, Role role, int level, int cin, int cout) -> Module& {
    Module m;
    m.kind = k; m.idx = (int)n.mods.size(); m.role = role; m.level = level; m.cin = cin; m.cout = cout;
    n.mods.push_back(m);
    return n.mods.back();
  };
  add(M_LINEAR, R_EMB_LINEAR0, 0, nf, 4 * nf);
  add(M_LINEAR, R_EMB_LINEAR1, 0, 4 * nf, 4 * nf);
  add(M_CONV3, R_STEM, 0, channels, nf).push = true;
  std::vector<int> hs_c{nf};
  int in_ch = nf, widest = nf;
  for (int l = 0; l <= last; ++l) {
    for (int b = 0; b < c.num_res_blocks; ++b) {
      add(M_RES, R_DOWN_BLOCK, l, in_ch, nf * c.ch_mult[l]).push = true;
      in_ch = nf * c.ch_mult[l];
      hs_c.push_back(in_ch);
    }
    if (l != last) {
      add(M_DOWN, R_DOWNSAMPLE, l, in_ch, in_ch).push = true;
      hs_c.push_back(in_ch);
    }
  }
  add(M_RES, R_MID_RES_IN, last, in_ch, in_ch);
  add(M_RES, R_MID_RES_OUT, last, in_ch, in_ch);
  for (int l = last; l >= 0; --l) {
    for (int b = 0; b < c.num_res_blocks + 1; ++b) {
      const int skip = hs_c.back(), out_ch = nf * c.ch_mult[l];
      hs_c.pop_back();
      CSD_REQUIRE(in_ch + skip != out_ch,
                  "unet 3-D: with this ch_mult the up block at level %d concatenates %d + %d channels, as many as it puts out: it has no Conv_2 "
                  "and the concatenation itself would be the residual, which the planned network does not materialise (no reference config "
                  "has such a ch_mult)", l, in_ch, skip);
      add(M_RES, R_UP_BLOCK, l, in_ch + skip, out_ch).skip = skip;
      widest = std::max(widest, in_ch + skip);
      in_ch = out_ch;
    }
    if (l != 0) add(M_UP, R_UPSAMPLE, l, in_ch, in_ch);
  }
  add(M_GN, R_HEAD_GN, 0, in_ch, in_ch);
  add(M_CONV3, R_HEAD_CONV, 0, in_ch, c.out_channels);
  const size_t vox = sample_elems(c);
  CSD_REQUIRE(vox * (size_t)widest * sizeof(float) < ((size_t)1 << 31) && vox < ((size_t)1 << 28),
              "unet 3-D: one sample (%d x %d x %d voxels, up to %d channels) exceeds the convolution kernel's 2 GiB per-sample addressing",
              c.vol[0], c.vol[1], c.vol[2], widest);

  const int temb = 4 * nf;
  for (auto& m : n.mods) {
    switch (m.kind) {
      case M_LINEAR:
        n.add_param(mname(m.idx, "weight"), {m.cout, m.cin});
        n.add_param(mname(m.idx, "bias"), {m.cout});
        break;
      case M_CONV3:
        n.add_param(mname(m.idx, "weight"), {m.cout, m.cin, 3, 3, 3});
        n.add_param(mname(m.idx, "bias"), {m.cout});
        break;
      case M_GN:
        n.add_param(mname(m.idx, "weight"), {m.cin});
        n.add_param(mname(m.idx, "bias"), {m.cin});
        break;
      case M_RES:                                      // ResnetBlockDDPM(dim = 3, conv_shortcut = True), models/layers.py:634-656
        n.add_param(mname(m.idx, "GroupNorm_0.weight"), {m.cin});
        n.add_param(mname(m.idx, "GroupNorm_0.bias"), {m.cin});
        n.add_param(mname(m.idx, "Conv_0.weight"), {m.cout, m.cin, 3, 3, 3});
        n.add_param(mname(m.idx, "Conv_0.bias"), {m.cout});
        n.add_param(mname(m.idx, "Dense_0.weight"), {m.cout, temb});
        n.add_param(mname(m.idx, "Dense_0.bias"), {m.cout});
        n.add_param(mname(m.idx, "GroupNorm_1.weight"), {m.cout});
        n.add_param(mname(m.idx, "GroupNorm_1.bias"), {m.cout});
        n.add_param(mname(m.idx, "Conv_1.weight"), {m.cout, m.cout, 3, 3, 3});
        n.add_param(mname(m.idx, "Conv_1.bias"), {m.cout});
        if (m.cin != m.cout) {
          n.add_param(mname(m.idx, "Conv_2.weight"), {m.cout, m.cin, 3, 3, 3});
          n.add_param(mname(m.idx, "Conv_2.bias"), {m.cout});
        }
        break;
      default:                                         // Downsample / Upsample without a convolution hold no parameter
        break;
    }
  }
  return CSD_OK;
}

// ---- packed layout: [conv weights in csd_conv3d_block's pack, one per layer | Dense_0 weights concatenated | their biases] -----------------
static int build_packed_layout3d(Net& n) {
  const csd_unet_config& c = n.cfg;
  size_t off = 0;                                      // floats; every entry starts on a 256-byte boundary
  auto add_slot = [&](const std::string& key, int c0, int cin, int cout, bool stem) {
    Conv3Slot s;
    s.param_w = n.P("all_modules." + key + ".weight");
    s.param_b = n.P("all_modules." + key + ".bias");
    s.cin = cin; s.c0 = c0; s.cout = cout;
    s.direct = stem || conv3d_is_direct(c.precision, c0);
    s.off = off;
    off += align_up(cdiv64((int64_t)conv3d_wpack_size(cin, cout, s.direct), 4), 64);
    n.slot3_by_name[key] = (int)n.slots3.size();
    n.slots3.push_back(s);
  };
  n.dense_total = 0;
  for (auto& m : n.mods) {
    const std::string id = std::to_string(m.idx);
    if (m.kind == M_CONV3) add_slot(id, m.cin, m.cin, m.cout, m.role == R_STEM);
    if (m.kind != M_RES) continue;
    const int c0 = m.cin - m.skip;
    add_slot(id + ".Conv_0", c0, m.cin, m.cout, false);
    add_slot(id + ".Conv_1", m.cout, m.cout, m.cout, false);
    if (m.cin != m.cout) add_slot(id + ".Conv_2", c0, m.cin, m.cout, false);
    n.dense_col[m.idx] = n.dense_total;
    n.dense_total += m.cout;
  }
  for (auto& s : n.slots3) CSD_REQUIRE(s.param_w >= 0 && s.param_b >= 0, "unet 3-D: internal error, a convolution has no parameter");
  n.dense_all_off = off;
  off += align_up((size_t)n.dense_total * 4 * c.nf, 64);
  n.dense_all_bias_off = off;
  off += align_up((size_t)n.dense_total, 64);
  n.packed_floats = off;
  return CSD_OK;
}

static int pack_all3d(Net& n, float* packed, hipStream_t s) {
  for (auto& p : n.params)
    if (!p.ptr) { set_error("pack: parameter '%s' was never set", p.name.c_str()); return CSD_ERR_STATE; }
  int rc;
  for (auto& sl : n.slots3)
    if ((rc = conv3d_pack_launch(n.params[sl.param_w].ptr, packed + sl.off, sl.cin, sl.cout, sl.direct, s))) return rc;
  const size_t K = (size_t)4 * n.cfg.nf;
  for (auto& m : n.mods) {
    if (m.kind != M_RES) continue;
    const size_t col = (size_t)n.dense_col[m.idx];
    const Param& w = n.params[n.P(mname(m.idx, "Dense_0.weight"))];
    const Param& b = n.params[n.P(mname(m.idx, "Dense_0.bias"))];
    CSD_CHECK_HIP(hipMemcpyAsync(packed + n.dense_all_off + col * K, w.ptr, (size_t)m.cout * K * sizeof(float), hipMemcpyDeviceToDevice, s));
    CSD_CHECK_HIP(hipMemcpyAsync(packed + n.dense_all_bias_off + col, b.ptr, (size_t)m.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  n.packed_once = true;
  return CSD_OK;
}

// ---- the plan of one batch size: DDPM3D.forward (models/ddpm3D.py:107-171) ---------------------------------------------------------------
namespace {
struct T3 {                // an activation [B, D >> lvl, H >> lvl, W >> lvl, C] in the workspace
  size_t off = NONE;
  int C = 0, lvl = 0;
};

struct Builder3 {
  Net& n;
  Plan3& pl;
  Arena ar;
  int B;
  Builder3(Net& n_, Plan3& pl_, int B_) : n(n_), pl(pl_), B(B_) {}
  int ext(int a, int lvl) const { return n.cfg.vol[a] >> lvl; }
  size_t vox(int lvl) const { return (size_t)ext(0, lvl) * ext(1, lvl) * ext(2, lvl); }
  T3 alloc(int C, int lvl) {
    T3 t;
    t.C = C; t.lvl = lvl;
    t.off = ar.alloc((size_t)B * vox(lvl) * C);
    return t;
  }
  void push(Op3& o, int launches = 1) {
    pl.launches += launches;
    pl.flops += o.flops;
    pl.bytes += o.bytes;
    pl.ops.push_back(o);
  }
  void dims(Op3& o, int lvl) const { o.D = ext(0, lvl); o.H = ext(1, lvl); o.W = ext(2, lvl); }

  // GroupNorm statistics of x0 (| x1) -> scale / shift [B, C0 + C1]; the fp64 partials live only between the op's two launches
  int gn(const T3& x0, const T3* x1, int pw, int pb, size_t* ns, size_t* nh) {
    const int C1 = x1 ? x1->C : 0;
    GNPlan g;
    int rc = gn_plan(&g, B, (int)vox(x0.lvl), x0.C, C1, 32);
    if (rc) return rc;
    Op3 o;
    o.kind = O3_GN; o.a = x0.off; o.b = x1 ? x1->off : NONE; o.C0 = x0.C; o.C1 = C1; o.pw = pw; o.pb = pb;
    dims(o, x0.lvl);
    o.partial = ar.alloc(cdiv64((int64_t)gn_partial_bytes(g), 4));
    o.ns = *ns = ar.alloc((size_t)B * (x0.C + C1));
    o.nh = *nh = ar.alloc((size_t)B * (x0.C + C1));
    ar.release(o.partial);
    o.cls = CSD_PROF_GN_STATS;
    o.bytes = (double)B * vox(x0.lvl) * (x0.C + C1) * 4;
    push(o, 2);
    return CSD_OK;
  }

  // csd_conv3d_block on x0 (| x1); ns == NONE: no prologue.  external: the destination is the caller's output
  T3 conv(const std::string& key, const T3& x0, const T3* x1, size_t ns, size_t nh, size_t temb_col, size_t res, bool external = false) {
    const Conv3Slot& sl = n.slots3[n.slot3_by_name.at(key)];
    Op3 o;
    o.kind = O3_CONV; o.slot = n.slot3_by_name.at(key);
    o.a = x0.off; o.b = x1 ? x1->off : NONE; o.C0 = x0.C; o.C1 = x1 ? x1->C : 0; o.Cout = sl.cout;
    o.ns = ns; o.nh = nh; o.temb_col = temb_col; o.res = res; o.act = n.cfg.act;
    dims(o, x0.lvl);
    T3 y;
    y.C = sl.cout; y.lvl = x0.lvl;
    if (external) o.out_external = true;
    else y = alloc(sl.cout, x0.lvl);
    o.out = y.off;
    const double nv = (double)B * vox(x0.lvl);
    o.cls = sl.direct ? CSD_PROF_CONV3X3_OTHER : CSD_PROF_CONV3X3;
    o.flops = 2.0 * 27 * sl.cin * sl.cout * nv;
    o.bytes = (nv * (sl.cin + sl.cout * (res != NONE ? 2 : 1)) + 27.0 * sl.cin * sl.cout) * 4;
    push(o);
    return y;
  }

  // ResnetBlockDDPM.forward (models/layers.py:658-675) on x = x0 (| x1)
  int res_block(const Module& m, const T3& x0, const T3* x1, T3* out) {
    const std::string id = std::to_string(m.idx);
    size_t ns, nh;
    int rc = gn(x0, x1, n.P(mname(m.idx, "GroupNorm_0.weight")), n.P(mname(m.idx, "GroupNorm_0.bias")), &ns, &nh);
    if (rc) return rc;
    T3 h = conv(id + ".Conv_0", x0, x1, ns, nh, (size_t)n.dense_col.at(m.idx), NONE);
    ar.release(ns); ar.release(nh);
    if ((rc = gn(h, nullptr, n.P(mname(m.idx, "GroupNorm_1.weight")), n.P(mname(m.idx, "GroupNorm_1.bias")), &ns, &nh))) return rc;
    T3 sc = x0;
    const bool has_sc = m.cin != m.cout;
    if (has_sc) sc = conv(id + ".Conv_2", x0, x1, NONE, NONE, NONE, NONE);
    else CSD_REQUIRE(!x1, "unet 3-D: internal error, a concatenated residual");
    *out = conv(id + ".Conv_1", h, nullptr, ns, nh, NONE, sc.off);
    ar.release(ns); ar.release(nh); ar.release(h.off);
    if (has_sc) ar.release(sc.off);
    return CSD_OK;
  }
};
}  // namespace

static int build_plan3d(Net& n, int B, Plan3** out) {
  CSD_REQUIRE(B >= 1 && B <= 65535, "unet 3-D: bad batch size %d", B);
  auto it = n.plans3.find(B);
  if (it != n.plans3.end()) { *out = it->second.get(); return CSD_OK; }
  const csd_unet_config& c = n.cfg;
  std::unique_ptr<Plan3> plan(new Plan3());
  plan->B = B;
  Builder3 b(n, *plan, B);
  const int nf = c.nf, K = 4 * nf;
  int rc;

  // time embedding: sinusoidal -> Linear -> act -> Linear, then every Dense_0(act(temb)) of the evaluation in one launch
  const size_t e0 = b.ar.alloc((size_t)B * nf), e1 = b.ar.alloc((size_t)B * K), e2 = b.ar.alloc((size_t)B * K);
  const size_t dense = b.ar.alloc((size_t)B * n.dense_total);
  {
    Op3 o;
    o.kind = O3_TEMB; o.out = e0; o.N = nf;
    b.push(o);
    Op3 l0;
    l0.kind = O3_LINEAR; l0.a = e0; l0.out = e1; l0.K = nf; l0.N = K; l0.act = CSD_ACT_NONE;
    l0.pw = n.P(mname(0, "weight")); l0.pb = n.P(mname(0, "bias"));
    l0.flops = 2.0 * B * nf * K; l0.bytes = ((double)nf * K + (double)B * (nf + K)) * 4;
    b.push(l0);
    Op3 l1;
    l1.kind = O3_LINEAR; l1.a = e1; l1.out = e2; l1.K = K; l1.N = K; l1.act = c.act;
    l1.pw = n.P(mname(1, "weight")); l1.pb = n.P(mname(1, "bias"));
    l1.flops = 2.0 * B * K * K; l1.bytes = ((double)K * K + 2.0 * B * K) * 4;
    b.push(l1);
    Op3 ld;
    ld.kind = O3_LINEAR; ld.a = e2; ld.out = dense; ld.K = K; ld.N = n.dense_total; ld.act = c.act;
    ld.pk_w = n.dense_all_off; ld.pk_b = n.dense_all_bias_off;
    ld.flops = 2.0 * B * K * n.dense_total; ld.bytes = ((double)K * n.dense_total + (double)B * (K + n.dense_total)) * 4;
    b.push(ld);
  }
  b.ar.release(e0); b.ar.release(e1); b.ar.release(e2);
  plan->dense_off = dense;

  std::vector<T3> hs;
  T3 h;
  for (auto& m : n.mods) {
    switch (m.role) {
      case R_EMB_LINEAR0:
      case R_EMB_LINEAR1:
        break;
      case R_STEM: {
        Op3 o;
        o.kind = O3_STEM; o.slot = n.slot3_by_name.at(std::to_string(m.idx));
        o.C0 = c.x_channels; o.C1 = c.y_channels; o.Cout = m.cout;
        b.dims(o, 0);
        h = b.alloc(m.cout, 0);
        o.out = h.off;
        const double nv = (double)B * b.vox(0);
        o.cls = CSD_PROF_CONV3X3_OTHER;
        o.flops = 2.0 * 27 * m.cin * m.cout * nv;
        o.bytes = (nv * (m.cin + m.cout) + 27.0 * m.cin * m.cout) * 4;
        b.push(o);
        hs.push_back(h);
        break;
      }
      case R_DOWN_BLOCK: {
        T3 y;
        if ((rc = b.res_block(m, hs.back(), nullptr, &y))) return rc;
        hs.push_back(y);
        break;
      }
      case R_DOWNSAMPLE: {
        const T3& x = hs.back();
        Op3 o;
        o.kind = O3_POOL; o.a = x.off; o.C0 = x.C;
        b.dims(o, x.lvl);
        T3 y = b.alloc(x.C, x.lvl + 1);
        o.out = y.off;
        o.bytes = (double)B * (b.vox(x.lvl) + b.vox(y.lvl)) * x.C * 4;
        b.push(o);
        hs.push_back(y);
        break;
      }
      case R_MID_RES_IN:                               // reads the top of the skip stack, which stays there for the up path
        if ((rc = b.res_block(m, hs.back(), nullptr, &h))) return rc;
        break;
      case R_MID_RES_OUT: {
        T3 y;
        if ((rc = b.res_block(m, h, nullptr, &y))) return rc;
        b.ar.release(h.off);
        h = y;
        break;
      }
      case R_UP_BLOCK: {
        const T3 skip = hs.back();
        hs.pop_back();
        T3 y;
        if ((rc = b.res_block(m, h, &skip, &y))) return rc;
        b.ar.release(h.off); b.ar.release(skip.off);      // the skip tensor lived until its up block had read it
        h = y;
        break;
      }
      case R_UPSAMPLE: {
        Op3 o;
        o.kind = O3_UP; o.a = h.off; o.C0 = h.C;
        b.dims(o, h.lvl);
        T3 y = b.alloc(h.C, h.lvl - 1);
        o.out = y.off;
        o.bytes = (double)B * (b.vox(h.lvl) + b.vox(y.lvl)) * h.C * 4;
        b.push(o);
        b.ar.release(h.off);
        h = y;
        break;
      }
      case R_HEAD_GN:
        break;                                         // (fused into the head convolution's staging, below)
      case R_HEAD_CONV: {
        CSD_REQUIRE(hs.empty() && h.lvl == 0, "unet 3-D: internal error, the skip stack is not empty at the head");
        size_t ns, nh;
        const int gi = m.idx - 1;
        if ((rc = b.gn(h, nullptr, n.P(mname(gi, "weight")), n.P(mname(gi, "bias")), &ns, &nh))) return rc;
        // one output channel: NDHWC is NCDHW already and the head writes the caller's output; else a de-interleave pass behind it
        const bool direct_out = c.out_channels == 1;
        T3 y = b.conv(std::to_string(m.idx), h, nullptr, ns, nh, NONE, NONE, direct_out);
        b.ar.release(ns); b.ar.release(nh); b.ar.release(h.off);
        if (!direct_out) {
          Op3 o;
          o.kind = O3_TO_NCDHW; o.a = y.off; o.C0 = c.out_channels; o.out_external = true;
          b.dims(o, 0);
          o.bytes = 2.0 * B * b.vox(0) * c.out_channels * 4;
          b.push(o);
          b.ar.release(y.off);
        }
        break;
      }
      default:
        CSD_REQUIRE(false, "unet 3-D: internal error, module %d has no place in the plan", m.idx);
    }
  }
  b.ar.release(dense);
  plan->ws_floats = b.ar.peak();
  *out = plan.get();
  n.plans3[B] = std::move(plan);
  return CSD_OK;
}

static int run_plan3d(Net& n, const Plan3& pl, const float* pk, float* ws, const float* x, const float* y, const float* labels, float* out,
                      const float* y_noise, float y_sigma, hipStream_t s) {
  const csd_unet_config& c = n.cfg;
  const int B = pl.B;
  auto W = [&](size_t off) -> float* { return off == NONE ? nullptr : ws + off; };
  auto P = [&](int idx) -> const float* { return idx < 0 ? nullptr : n.params[idx].ptr; };
  int rc;
  for (const Op3& o : pl.ops) {
    switch (o.kind) {
      case O3_TEMB: {
        ProfScope prof(o.cls, o.flops, o.bytes, s);
        if ((rc = timestep_embedding_launch(labels, W(o.out), B, o.N, s))) return rc;
        break;
      }
      case O3_LINEAR: {
        ProfScope prof(o.cls, o.flops, o.bytes, s);
        const float* w = o.pk_w != NONE ? pk + o.pk_w : P(o.pw);
        const float* bias = o.pk_b != NONE ? pk + o.pk_b : P(o.pb);
        if ((rc = linear_launch(W(o.a), w, bias, W(o.out), B, o.K, o.N, o.act, s))) return rc;
        break;
      }
      case O3_STEM: {
        const Conv3Slot& sl = n.slots3[o.slot];
        ProfScope prof(o.cls, o.flops, o.bytes, s);
        if ((rc = conv3d_stem_launch(x, y, y_noise, y_sigma, pk + sl.off, P(sl.param_b), W(o.out), B, o.C0, o.C1, o.Cout, o.D, o.H, o.W,
                                     c.centered, s))) return rc;
        break;
      }
      case O3_GN: {
        GNPlan g;
        if ((rc = gn_plan(&g, B, o.D * o.H * o.W, o.C0, o.C1, 32))) return rc;
        double* partial = reinterpret_cast<double*>(W(o.partial));
        {
          ProfScope prof(CSD_PROF_GN_STATS, 0, o.bytes, s);
          if ((rc = gn_stats_launch(g, W(o.a), W(o.b), partial, s))) return rc;
        }
        ProfScope prof(CSD_PROF_GN_FINAL, 0, (double)gn_partial_bytes(g), s);
        if ((rc = gn_finalize_launch(g, partial, P(o.pw), P(o.pb), 1e-6f, W(o.ns), W(o.nh), s))) return rc;
        break;
      }
      case O3_CONV: {
        const Conv3Slot& sl = n.slots3[o.slot];
        Conv3dCall k;
        k.x0 = W(o.a); k.x1 = W(o.b); k.wpack = pk + sl.off; k.bias = P(sl.param_b); k.nscale = W(o.ns); k.nshift = W(o.nh);
        k.temb = o.temb_col == NONE ? nullptr : ws + pl.dense_off + o.temb_col;
        k.temb_stride = o.temb_col == NONE ? 0 : n.dense_total;
        k.res = W(o.res); k.out = o.out_external ? out : W(o.out);
        k.act = o.act; k.out_scale = 1.0f;
        k.B = B; k.C0 = o.C0; k.C1 = o.C1; k.Cout = o.Cout; k.D = o.D; k.H = o.H; k.W = o.W; k.precision = c.precision;
        ProfScope prof(o.cls, o.flops, o.bytes, s);
        if ((rc = conv3d_launch(k, s))) return rc;
        break;
      }
      case O3_POOL: {
        ProfScope prof(o.cls, 0, o.bytes, s);
        if ((rc = csd_avgpool3d_2_ndhwc(W(o.a), W(o.out), B, o.D, o.H, o.W, o.C0, s))) return rc;
        break;
      }
      case O3_UP: {
        ProfScope prof(o.cls, 0, o.bytes, s);
        if ((rc = csd_nearest_up2_3d_ndhwc(W(o.a), W(o.out), B, o.D, o.H, o.W, o.C0, s))) return rc;
        break;
      }
      case O3_TO_NCDHW: {
        ProfScope prof(o.cls, 0, o.bytes, s);
        if ((rc = nhwc_to_nchw_launch(W(o.a), out, B, o.C0, o.D * o.H * o.W, o.C0, s))) return rc;
        break;
      }
    }
  }
  return CSD_OK;
}

}  // namespace csd
