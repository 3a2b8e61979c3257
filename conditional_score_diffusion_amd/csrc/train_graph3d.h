// train_graph3d.h - the training step of the 3-D DDPM family (arch 2; reference models/ddpm3D.py:107-171 with model.train()) as one planned
// graph behind the entry points of train_graph.h.  Included from unet.hip behind train_graph.h: it shares TrainState, the (handle,
// workspace) record map, the call-index contract, the GradMarks machinery and the bump allocator with its dry-run sizing (TG3 derives from
// TG for exactly those; the 2-D forward / backward are untouched).
//
// What it replaces: torch autograd over models/ddpm3d.py's _GradOps3D (grad_ops_3d).  The forward runs the same layer sequence on the same
// kernels - channels-last [B, D, H, W, C], GroupNorm + activation as its own saved operand (the weight gradient needs it), Dense_0's row and
// the shortcut in the convolutions' epilogues, dropout in the GroupNorm's apply pass with the operator path's Philox stream ids
// (call << 16) + k - and keeps only what a gradient reads.  The backward walks the recorded steps in reverse and writes (or, accumulating,
// adds to) every parameter gradient at the caller's pointer.  Against the autograd graph: no per-layer host node, no flipped / transposed
// weight copy (conv3d_pack_launch's flip_t mode packs the data gradient's weight from the forward layer's), the weight gradient's reduce
// stage adds to the slot itself (conv3d_wgrad_beta), Conv_0's bias gradient and Dense_0's gradient share one voxel reduction, Conv_1's and
// Conv_2's bias gradients another, and the stem's data gradient, the NDHWC -> NCDHW change, the x slice and the 2v - 1 map's factor are one
// kernel (conv3d_stem_dx_launch).  An up block's input h | skip is never concatenated: its GroupNorm (gn3_two) and Conv_2 read the two
// sources, and the GroupNorm's backward writes the gradient per source (GnBwdSplit), adding to what another consumer of the tensor left
// there - a tensor with two consumers gets no add pass either (grad_dst).
// One stream, a fixed order, no atomics: bitwise repeatable, and a sample's results do not depend on its place in the batch (every kernel
// here works per sample; the weight gradient's split count is a function of the volume and the channel counts only).
#pragma once

namespace csd {

// NCDHW sources a [B, Ca, vox] | b [B, Cb, vox] (b optional) -> NDHWC [B, vox, Ca + Cb]; v -> 2v - 1 unless `centered`
__global__ void ncdhw_to_ndhwc2_kernel(const float* __restrict__ a, int Ca, const float* __restrict__ b, int Cb, float* __restrict__ out,
                                       size_t vox, size_t total, int centered) {
  const int C = Ca + Cb;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const size_t r = i / C;
    const size_t v = r % vox, bi = r / vox;
    float val = c < Ca ? a[(bi * Ca + c) * vox + v] : b[(bi * Cb + (c - Ca)) * vox + v];
    if (!centered) val = 2.f * val - 1.f;
    out[i] = val;
  }
}

// act(x * scale + shift) of x = x0 [B, vox, C0] | x1 [B, vox, C1] into ONE tensor [B, vox, C0 + C1] (gn_apply_kernel's expression on the
// virtual concatenation of an up block: the GroupNorm's output is the convolution's and the weight gradient's operand, the input is never
// concatenated); scale / shift [B, C0 + C1]
__global__ void gn_apply2_kernel(const float* __restrict__ x0, const float* __restrict__ x1, int C0, int C1, const float* __restrict__ nscale,
                                 const float* __restrict__ nshift, float* __restrict__ y, size_t vox, int act, size_t total4) {
  const int C = C0 + C1, C4 = C >> 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i / C4;
    const int c = (int)(i - pix * C4) * 4;
    const size_t b = pix / vox;
    const float4 v = *reinterpret_cast<const float4*>(c < C0 ? x0 + pix * C0 + c : x1 + pix * C1 + (c - C0));
    const float4 sc = *reinterpret_cast<const float4*>(nscale + b * C + c);
    const float4 sh = *reinterpret_cast<const float4*>(nshift + b * C + c);
    float o[4] = {v.x * sc.x + sh.x, v.y * sc.y + sh.y, v.z * sc.z + sh.z, v.w * sc.w + sh.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      switch (act) {
        case CSD_ACT_SWISH: o[j] = o[j] / (1.0f + expf(-o[j])); break;
        case CSD_ACT_RELU: o[j] = o[j] > 0.f ? o[j] : 0.f; break;
        case CSD_ACT_LRELU: o[j] = o[j] > 0.f ? o[j] : 0.2f * o[j]; break;
        case CSD_ACT_ELU: o[j] = o[j] > 0.f ? o[j] : expm1f(o[j]); break;
        default: break;
      }
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// the 2x2x2 average pool's backward: dx [B, D, H, W, C] (=|+=) dy [B, D/2, H/2, W/2, C] / 8 (acc: dx already holds another consumer's gradient)
__global__ void avgpool3d_2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int D, int H, int W, int C, size_t total, int acc) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t r = i / C;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H); r /= H;
    const int z = (int)(r % D);
    const size_t b = r / D;
    const float v = dy[(((b * (D >> 1) + (z >> 1)) * (H >> 1) + (y >> 1)) * (W >> 1) + (x >> 1)) * C + c] * 0.125f;
    dx[i] = acc ? dx[i] + v : v;
  }
}

#define TG_RUN(expr)                       \
  do {                                     \
    if (!dry) {                            \
      const int _rc = (expr);              \
      if (_rc) return _rc;                 \
    }                                      \
  } while (0)

// (TT::H holds the tensor's LEVEL here: its extents are vol[a] >> level)
struct TG3 : TG {
  using TG::TG;
  int ext(int a, int lvl) const { return n.cfg.vol[a] >> lvl; }
  size_t vox(int lvl) const { return (size_t)ext(0, lvl) * ext(1, lvl) * ext(2, lvl); }
  size_t act3_n(int lvl, int C) const { return (size_t)B * vox(lvl) * C; }
  int new_tensor3(int lvl, int C) {
    TT t;
    t.H = lvl; t.C = C;
    t.p = alloc(act3_n(lvl, C));
    st.t.push_back(t);
    return (int)st.t.size() - 1;
  }
  // where a consumer writes its gradient of tensor tid: the tensor's gradient buffer, made by the first consumer to arrive (*acc = 0: it
  // stores) - every later one adds to it in the kernel that forms its contribution (*acc = 1), never in a pass of its own.  Call it
  // before the step's temporaries: the buffer lives until the tensor's producer has read it
  float* grad_dst(int tid, int* acc) {
    TT& t = st.t[tid];
    *acc = t.g != nullptr;
    if (!t.g) t.g = alloc(act3_n(t.H, t.C));
    return t.g;
  }

  // ---- operator wrappers (scratch is a temporary above `top`) ---------------------------------------------------------------------
  // csd_conv3d_block without prologue on x [B, vox, Cin]: ((conv + bias) + (res + temb row)); the weight is packed into scratch
  // (x1, C1: the second source of a two-source layer, x = x | x1 of Cin = C0 + C1 channels)
  int conv3(const float* x, const float* w, const float* b, float* y, int Cin, int Cout, int lvl, const float* res = nullptr,
            const float* temb = nullptr, const float* x1 = nullptr, int C1 = 0) {
    const size_t m = top;
    void* sc = alloc_bytes(csd_conv3d_block_scratch_bytes(Cin, Cout));
    if (!dry) {
      void* wp = scratch_aligned<void>(sc);
      const bool direct = conv3d_is_direct(prec, Cin - C1);
      int rc = conv3d_pack_launch(w, wp, Cin, Cout, direct, s);
      if (rc) return rc;
      Conv3dCall c;
      c.x0 = x; c.x1 = x1; c.C1 = C1; c.wpack = wp; c.bias = b; c.res = res; c.temb = temb; c.temb_stride = Cout; c.out = y; c.act = CSD_ACT_NONE;
      c.B = B; c.C0 = Cin - C1; c.Cout = Cout; c.D = ext(0, lvl); c.H = ext(1, lvl); c.W = ext(2, lvl); c.precision = prec;
      if ((rc = conv3d_launch(c, s))) return rc;
    }
    top = m;
    return CSD_OK;
  }
  // the data gradient of y = conv3(x, w [Cout, Cin, 27]): dx [B, vox, Cin] = conv3(dy * 2^k, w flipped and transposed) / 2^k with the
  // per-sample power of two of csd_conv3d_dgrad_scale - grad_ops_3d.conv3d_dgrad without the weight copy (flip_t pack)
  int dgrad3(const float* dy, const float* w, float* dx, int Cin, int Cout, int lvl) {
    const size_t m = top;
    float* rowscale = alloc(B);
    float* ns = alloc((size_t)B * Cout);
    float* nh = alloc((size_t)B * Cout);
    void* ssc = alloc_bytes(csd_conv3d_dgrad_scale_scratch_bytes(B));
    void* sc = alloc_bytes(csd_conv3d_block_scratch_bytes(Cout, Cin));
    if (!dry) {
      int rc = csd_conv3d_dgrad_scale(dy, rowscale, ns, nh, B, (int64_t)(vox(lvl) * Cout), Cout, ssc, s);
      if (rc) return rc;
      void* wp = scratch_aligned<void>(sc);
      if ((rc = conv3d_pack_launch(w, wp, Cout, Cin, conv3d_is_direct(prec, Cout), s, true))) return rc;
      Conv3dCall c;
      c.x0 = dy; c.wpack = wp; c.nscale = ns; c.nshift = nh; c.act = CSD_ACT_NONE; c.out = dx;
      c.B = B; c.C0 = Cout; c.Cout = Cin; c.D = ext(0, lvl); c.H = ext(1, lvl); c.W = ext(2, lvl); c.precision = prec;
      if ((rc = conv3d_launch(c, s))) return rc;
      if ((rc = csd_scale_rows(dx, dx, rowscale, 1, B, (int64_t)(vox(lvl) * Cin), s))) return rc;
    }
    top = m;
    return CSD_OK;
  }
  // (ci_off, Cin_dw: `a` is one source of a two-source layer: the input-channel slice ci_off .. ci_off + Cin of dw [Cout, Cin_dw, 27])
  int wgrad3(const float* a, const float* dy, float* dw, int Cin, int Cout, int lvl, int ci_off = 0, int Cin_dw = 0) {
    if (!pg) return CSD_OK;
    const size_t m = top;
    void* sc = alloc_bytes(csd_conv3d_wgrad_scratch_bytes(B, Cin, Cout, ext(0, lvl), ext(1, lvl), ext(2, lvl), prec));
    TG_RUN(conv3d_wgrad_beta(a, dy, dw, B, Cin, Cout, ext(0, lvl), ext(1, lvl), ext(2, lvl), prec, sc, s, gacc, ci_off, Cin_dw));
    top = m;
    return CSD_OK;
  }
  int gn3(const float* x, const float* gamma, const float* beta, float* y, float* rs, float* ms, int C, int lvl, float* mask = nullptr,
          uint64_t drop_id = 0) {
    const size_t m = top;
    float* sc = alloc_bytes(csd_groupnorm_nhwc_scratch_bytes(B, C, (int)vox(lvl)));
    TG_RUN(groupnorm_act_dropout_nhwc(x, gamma, beta, y, rs, ms, mask, p_drop, seed, drop_id, B, C, (int)vox(lvl), 32, 1e-6f, act, sc, s));
    top = m;
    return CSD_OK;
  }
  // t: the GroupNorm's input (one source, or the two of an up block) and where its gradient goes (GnBwdSplit, common.h)
  // act(GroupNorm(x0 | x1)) of an up block's two sources into one tensor: the two-source statistics of csd_groupnorm_scale_shift, then
  // gn_apply2_kernel
  int gn3_two(const float* x0, const float* x1, int C0, int C1, const float* gamma, const float* beta, float* y, float* rs, float* ms, int lvl) {
    const size_t m = top;
    const int C = C0 + C1;
    GNPlan g;
    int rc = gn_plan(&g, B, (int)vox(lvl), C0, C1, 32);
    if (rc) return rc;
    float* sc = alloc((size_t)B * C);
    float* sh = alloc((size_t)B * C);
    double* partial = reinterpret_cast<double*>(alloc_bytes(gn_partial_bytes(g)));
    if (!dry) {
      if ((rc = gn_stats_launch(g, x0, x1, partial, s))) return rc;
      if ((rc = gn_finalize_launch(g, partial, gamma, beta, 1e-6f, sc, sh, s, rs, ms))) return rc;
      const size_t total4 = act3_n(lvl, C) / 4;
      hipLaunchKernelGGL(gn_apply2_kernel, dim3(launch_blocks(total4)), dim3(256), 0, s, x0, x1, C0, C1, sc, sh, y, vox(lvl), act, total4);
      CSD_LAUNCH_CHECK();
    }
    top = m;
    return CSD_OK;
  }
  int gn3_bwd(const GnBwdSplit& t, const float* gamma, const float* beta, const float* rs, const float* ms, const float* dy,
              float* dgamma, float* dbeta, int C, int lvl, const float* add = nullptr) {
    const size_t m = top;
    float* grow = alloc((size_t)B * C);
    float* brow = alloc((size_t)B * C);
    float* sc = alloc_bytes(csd_groupnorm_nhwc_scratch_bytes(B, C, (int)vox(lvl)));
    TG_RUN(groupnorm_act_backward_nhwc_split(t, gamma, beta, rs, ms, dy, add, grow, brow, C, B, C, (int)vox(lvl), 32, act, sc, s));
    if (pg) TG_RUN(sum_rows2(grow, dgamma, brow, dbeta, B, C, s, gacc));
    top = m;
    return CSD_OK;
  }
  // out[b, c] = sum over the voxels of dy [B, vox, C]   (C a multiple of 4: every activation of the network is)
  int sum_vox(const float* dy, float* out, int C, int lvl) {
    const size_t m = top;
    float* sc = alloc_bytes(csd_sum_pixels_scratch_bytes(B, (int)vox(lvl), C));
    TG_RUN(csd_sum_pixels_nhwc(dy, out, B, (int)vox(lvl), C, sc, s));
    top = m;
    return CSD_OK;
  }

  // =====================================================================================================================================
  // forward
  // =====================================================================================================================================
  // ResnetBlockDDPM(dim = 3, conv_shortcut = True).forward (models/layers.py:658-675), _GradOps3D.res
  // in1 >= 0: an up block - x = tensor in | tensor in1 (h | skip) is read from its two sources by the GroupNorm and by Conv_2
  int res3_fwd(const Module& m, int in, int* out_tid, int in1 = -1) {
    const int lvl = st.t[in].H, cin = m.cin, cout = m.cout;
    const float* h = st.t[in].p;
    const float* h1 = in1 >= 0 ? st.t[in1].p : nullptr;
    const int C1 = in1 >= 0 ? st.t[in1].C : 0, C0 = cin - C1;
    CSD_REQUIRE(st.t[in].C == C0 && (in1 < 0 || (st.t[in1].H == lvl && cin != cout)), "train_forward 3-D: module %d reads %d + %d channels, not %d",
                m.idx, st.t[in].C, C1, cin);
    TStep sp;
    sp.kind = TS_RES; sp.mod = m.idx; sp.in0 = in; sp.in1 = in1;
    sp.op0 = alloc(act3_n(lvl, cin));                  // act(GroupNorm_0(x))
    sp.rs0 = alloc((size_t)B * cin); sp.ms0 = alloc((size_t)B * cin);
    sp.c0 = alloc(act3_n(lvl, cout));
    sp.a1 = alloc(act3_n(lvl, cout));
    sp.rs1 = alloc((size_t)B * cout); sp.ms1 = alloc((size_t)B * cout);
    ++drop_count;
    sp.drop_id = (call << 16) + (uint64_t)drop_count;
    if (p_drop > 0.f) sp.mask = alloc(act3_n(lvl, cout));
    sp.out = new_tensor3(lvl, cout);
    float* o = st.t[sp.out].p;
    const size_t mk = top;
    int rc = h1 ? gn3_two(h, h1, C0, C1, W(m.idx, "GroupNorm_0.weight"), W(m.idx, "GroupNorm_0.bias"), sp.op0, sp.rs0, sp.ms0, lvl)
                : gn3(h, W(m.idx, "GroupNorm_0.weight"), W(m.idx, "GroupNorm_0.bias"), sp.op0, sp.rs0, sp.ms0, cin, lvl);
    if (rc) return rc;
    float* d = alloc((size_t)B * cout);                // Dense_0(act(temb)) rides in Conv_0's epilogue
    TG_RUN(csd_linear(st.temb2_act, W(m.idx, "Dense_0.weight"), W(m.idx, "Dense_0.bias"), d, B, 4 * n.cfg.nf, cout, CSD_ACT_NONE, s));
    rc = conv3(sp.op0, W(m.idx, "Conv_0.weight"), W(m.idx, "Conv_0.bias"), sp.c0, cin, cout, lvl, nullptr, d);
    if (rc) return rc;
    rc = gn3(sp.c0, W(m.idx, "GroupNorm_1.weight"), W(m.idx, "GroupNorm_1.bias"), sp.a1, sp.rs1, sp.ms1, cout, lvl, sp.mask, sp.drop_id);
    if (rc) return rc;
    const float* shortcut = h;
    if (cin != cout) {
      float* sc = alloc(act3_n(lvl, cout));
      rc = conv3(h, W(m.idx, "Conv_2.weight"), W(m.idx, "Conv_2.bias"), sc, cin, cout, lvl, nullptr, nullptr, h1, C1);
      if (rc) return rc;
      shortcut = sc;
    }
    rc = conv3(sp.a1, W(m.idx, "Conv_1.weight"), W(m.idx, "Conv_1.bias"), o, cout, cout, lvl, shortcut);      // + shortcut in the epilogue
    if (rc) return rc;
    top = mk;
    st.steps.push_back(sp);
    *out_tid = sp.out;
    return CSD_OK;
  }

  // DDPM3D.forward (models/ddpm3D.py:107-171): the walk of build_plan3d (unet3d.h)
  int forward(const float* x, const float* y, const float* labels, float* out) {
    const csd_unet_config& c = n.cfg;
    const int cx = c.x_channels, cy = c.y_channels, cio = cx + cy, nf = c.nf, co = c.out_channels;
    st.t.clear(); st.steps.clear();
    drop_count = 0;
    st.lin0 = 0; st.emb_dim = nf; st.fourier_mod = -1;
    // network input: cat(x, y), 2v - 1 for data in [0, 1], NCDHW -> NDHWC (the stem's weight gradient reads it)
    st.xin = alloc(act3_n(0, cio));
    if (!dry) {
      const size_t total = act3_n(0, cio);
      hipLaunchKernelGGL(ncdhw_to_ndhwc2_kernel, dim3(launch_blocks(total)), dim3(256), 0, s, x, cx, y, cy, st.xin, vox(0), total, c.centered);
      CSD_LAUNCH_CHECK();
    }
    std::vector<int> hs;
    int h = -1;
    for (const Module& m : n.mods) {
      int rc = CSD_OK;
      switch (m.role) {
        case R_EMB_LINEAR0:
          st.lin0 = m.idx;
          st.emb = alloc((size_t)B * nf);
          TG_RUN(csd_timestep_embedding(labels, st.emb, B, nf, s));
          st.temb1 = alloc((size_t)B * 4 * nf); st.temb2 = alloc((size_t)B * 4 * nf);
          TG_RUN(csd_linear(st.emb, W(m.idx, "weight"), W(m.idx, "bias"), st.temb1, B, nf, 4 * nf, CSD_ACT_NONE, s));
          break;
        case R_EMB_LINEAR1:
          TG_RUN(csd_linear(st.temb1, W(m.idx, "weight"), W(m.idx, "bias"), st.temb2, B, 4 * nf, 4 * nf, act, s));
          st.temb2_act = alloc((size_t)B * 4 * nf);
          TG_RUN(csd_act(st.temb2, nullptr, st.temb2_act, act, (int64_t)B * 4 * nf, s));
          break;
        case R_STEM: {
          h = new_tensor3(0, nf);
          rc = conv3(st.xin, W(m.idx, "weight"), W(m.idx, "bias"), st.t[h].p, cio, nf, 0);
          if (rc) return rc;
          TStep sp;
          sp.kind = TS_STEM; sp.mod = m.idx; sp.out = h;
          st.steps.push_back(sp);
          hs.push_back(h);
          break;
        }
        case R_DOWN_BLOCK: {
          int o;
          rc = res3_fwd(m, hs.back(), &o); if (rc) return rc;
          hs.push_back(o);
          break;
        }
        case R_DOWNSAMPLE: {                           // 2x2x2 average pool
          const int in = hs.back(), lvl = st.t[in].H, C = st.t[in].C;
          const int o = new_tensor3(lvl + 1, C);
          TG_RUN(csd_avgpool3d_2_ndhwc(st.t[in].p, st.t[o].p, B, ext(0, lvl), ext(1, lvl), ext(2, lvl), C, s));
          TStep sp;
          sp.kind = TS_DOWN; sp.mod = m.idx; sp.in0 = in; sp.out = o;
          st.steps.push_back(sp);
          hs.push_back(o);
          break;
        }
        case R_MID_RES_IN:                             // reads the top of the skip stack, which stays there for the up path
          rc = res3_fwd(m, hs.back(), &h);
          break;
        case R_MID_RES_OUT:
          rc = res3_fwd(m, h, &h);
          break;
        case R_UP_BLOCK:
          CSD_REQUIRE(!hs.empty(), "train_forward 3-D: the skip stack is empty at an up block");
          rc = res3_fwd(m, h, &h, hs.back());           // (h | skip: two sources, no concatenated tensor)
          hs.pop_back();
          break;
        case R_UPSAMPLE: {                             // nearest x2
          const int lvl = st.t[h].H, C = st.t[h].C;
          const int o = new_tensor3(lvl - 1, C);
          TG_RUN(csd_nearest_up2_3d_ndhwc(st.t[h].p, st.t[o].p, B, ext(0, lvl), ext(1, lvl), ext(2, lvl), C, s));
          TStep sp;
          sp.kind = TS_UP; sp.mod = m.idx; sp.in0 = h; sp.out = o;
          st.steps.push_back(sp);
          h = o;
          break;
        }
        case R_HEAD_GN: {                              // act(GroupNorm(h)) + the head convolution, NCDHW out
          const Module& mc = n.mods[m.idx + 1];
          const int C = m.cin;
          CSD_REQUIRE(hs.empty() && st.t[h].H == 0, "train_forward 3-D: the skip stack is not empty at the head");
          TStep sp;
          sp.kind = TS_HEAD; sp.mod = m.idx; sp.in0 = h;
          sp.op0 = alloc(act3_n(0, C));
          sp.rs0 = alloc((size_t)B * C); sp.ms0 = alloc((size_t)B * C);
          rc = gn3(st.t[h].p, W(m.idx, "weight"), W(m.idx, "bias"), sp.op0, sp.rs0, sp.ms0, C, 0); if (rc) return rc;
          const size_t mk = top;
          // (one output channel: NDHWC is NCDHW already and the head writes the caller's output)
          float* o = co == 1 ? out : alloc(act3_n(0, co));
          rc = conv3(sp.op0, W(mc.idx, "weight"), W(mc.idx, "bias"), o, C, co, 0); if (rc) return rc;
          if (co != 1) TG_RUN(nhwc_to_nchw_launch(o, out, B, co, (int)vox(0), co, s));
          top = mk;
          st.steps.push_back(sp);
          break;
        }
        case R_HEAD_CONV:
          break;                                       // (with its GroupNorm)
        default:
          CSD_REQUIRE(false, "train_forward 3-D: module %d has no place in the graph", m.idx);
      }
      if (rc) return rc;
    }
    st.fwd_top = top;
    return CSD_OK;
  }

  // =====================================================================================================================================
  // backward
  // =====================================================================================================================================
  int res3_bwd(const TStep& sp, float* dtemb_act) {
    const Module& m = n.mods[sp.mod];
    const TT& tin = st.t[sp.in0];
    const int lvl = tin.H, cin = m.cin, cout = m.cout;
    const float* h = tin.p;
    // where the gradient w.r.t. the block input goes: per source, into the buffer another consumer made or a new one
    GnBwdSplit in;
    in.x0 = h; in.C0 = tin.C;
    in.dx0 = grad_dst(sp.in0, &in.acc0);
    if (sp.in1 >= 0) { in.x1 = st.t[sp.in1].p; in.dx1 = grad_dst(sp.in1, &in.acc1); }
    const size_t mk = top;
    int rc;
    const float* dout = st.t[sp.out].g;
    // Conv_1 (and Conv_2): the bias gradients are the same voxel sums of dout
    rc = wgrad3(sp.a1, dout, DW(m.idx, "Conv_1.weight"), cout, cout, lvl); if (rc) return rc;
    if (pg) {
      float* bc = alloc((size_t)B * cout);
      rc = sum_vox(dout, bc, cout, lvl); if (rc) return rc;
      TG_RUN(sum_rows_beta(bc, DW(m.idx, "Conv_1.bias"), B, cout, gacc, s));
      if (cin != cout) TG_RUN(sum_rows_beta(bc, DW(m.idx, "Conv_2.bias"), B, cout, gacc, s));
    }
    float* d1 = alloc(act3_n(lvl, cout));
    rc = dgrad3(dout, W(m.idx, "Conv_1.weight"), d1, cout, cout, lvl); if (rc) return rc;
    if (sp.mask) TG_RUN(csd_mul(d1, sp.mask, d1, (int64_t)act3_n(lvl, cout), s));
    float* d1b = alloc(act3_n(lvl, cout));
    GnBwdSplit mid;
    mid.x0 = sp.c0; mid.dx0 = d1b; mid.C0 = cout;
    rc = gn3_bwd(mid, W(m.idx, "GroupNorm_1.weight"), W(m.idx, "GroupNorm_1.bias"), sp.rs1, sp.ms1, d1, DW(m.idx, "GroupNorm_1.weight"),
                 DW(m.idx, "GroupNorm_1.bias"), cout, lvl);
    if (rc) return rc;
    // Conv_0's bias and the time-embedding row share the per-(sample, channel) voxel sums of d1b
    if (pg) {
      float* dd = alloc((size_t)B * cout);
      rc = sum_vox(d1b, dd, cout, lvl); if (rc) return rc;
      TG_RUN(sum_rows_beta(dd, DW(m.idx, "Conv_0.bias"), B, cout, gacc, s));
      rc = linear_bwd(st.temb2_act, CSD_ACT_NONE, W(m.idx, "Dense_0.weight"), dd, DW(m.idx, "Dense_0.weight"), DW(m.idx, "Dense_0.bias"), dtemb_act,
                      4 * n.cfg.nf, cout);
      if (rc) return rc;
    }
    rc = wgrad3(sp.op0, d1b, DW(m.idx, "Conv_0.weight"), cin, cout, lvl); if (rc) return rc;
    float* d0 = d1;                                    // (d1 is dead: Conv_0's data gradient takes its place where the widths agree)
    if (cin != cout) d0 = alloc(act3_n(lvl, cin));
    rc = dgrad3(d1b, W(m.idx, "Conv_0.weight"), d0, cin, cout, lvl); if (rc) return rc;
    const float* add = dout;                           // the identity shortcut's gradient; it joins inside the GroupNorm_0 backward
    if (cin != cout) {                                 // Conv_2 read the block input itself: its weight gradient per source
      rc = wgrad3(h, dout, DW(m.idx, "Conv_2.weight"), in.C0, cout, lvl, 0, cin); if (rc) return rc;
      if (in.x1) { rc = wgrad3(in.x1, dout, DW(m.idx, "Conv_2.weight"), cin - in.C0, cout, lvl, in.C0, cin); if (rc) return rc; }
      float* dsc = alloc(act3_n(lvl, cin));
      rc = dgrad3(dout, W(m.idx, "Conv_2.weight"), dsc, cin, cout, lvl); if (rc) return rc;
      add = dsc;
    }
    // ... which writes the block input's gradient where it belongs: h's and the skip tensor's buffers of an up block (no split pass),
    // added to what another consumer left there (no add pass)
    rc = gn3_bwd(in, W(m.idx, "GroupNorm_0.weight"), W(m.idx, "GroupNorm_0.bias"), sp.rs0, sp.ms0, d0, DW(m.idx, "GroupNorm_0.weight"),
                 DW(m.idx, "GroupNorm_0.bias"), cin, lvl, add);
    if (rc) return rc;
    top = mk;
    return CSD_OK;
  }

  int head3_bwd(const TStep& sp, const float* d_out) {
    const Module& mg = n.mods[sp.mod];
    const Module& mc = n.mods[sp.mod + 1];
    const TT& tin = st.t[sp.in0];
    const int C = mg.cin, co = n.cfg.out_channels;
    GnBwdSplit in;
    in.x0 = tin.p; in.C0 = C;
    in.dx0 = grad_dst(sp.in0, &in.acc0);
    const size_t mk = top;
    int rc;
    const float* dP = d_out;                           // NDHWC; one channel: the caller's NCDHW gradient as it is
    if (co != 1) {
      float* t = alloc(act3_n(0, co));
      if (!dry) {
        const size_t total = act3_n(0, co);
        hipLaunchKernelGGL(ncdhw_to_ndhwc2_kernel, dim3(launch_blocks(total)), dim3(256), 0, s, d_out, co, nullptr, 0, t, vox(0), total, 1);
        CSD_LAUNCH_CHECK();
      }
      dP = t;
    }
    rc = wgrad3(sp.op0, dP, DW(mc.idx, "weight"), C, co, 0); if (rc) return rc;
    if (pg) {                                          // bias: the NCDHW gradient -> per-(sample, channel) sums -> batch sum
      float* bc = alloc((size_t)B * co);
      TG_RUN(csd_sum_inner(d_out, bc, (int64_t)B * co, (int64_t)vox(0), s));
      TG_RUN(sum_rows_beta(bc, DW(mc.idx, "bias"), B, co, gacc, s));
    }
    float* dg = alloc(act3_n(0, C));
    rc = dgrad3(dP, W(mc.idx, "weight"), dg, C, co, 0); if (rc) return rc;
    rc = gn3_bwd(in, W(mg.idx, "weight"), W(mg.idx, "bias"), sp.rs0, sp.ms0, dg, DW(mg.idx, "weight"), DW(mg.idx, "bias"), C, 0);
    if (rc) return rc;
    top = mk;
    return CSD_OK;
  }

  int backward(const float* d_out) {
    const csd_unet_config& c = n.cfg;
    const int nf = c.nf;
    top = st.fwd_top;
    int rc;
    float* dtemb_act = nullptr;                        // sum over the blocks of dDense . W: gradient w.r.t. act(temb2)
    if (pg) {
      dtemb_act = alloc((size_t)B * 4 * nf);
      if (!dry) CSD_CHECK_HIP(hipMemsetAsync(dtemb_act, 0, (size_t)B * 4 * nf * sizeof(float), s));
    }
    for (int i = (int)st.steps.size() - 1; i >= 0; --i) {
      const TStep& sp = st.steps[i];
      // step i + 1 and everything behind it is complete (the steps walk the modules in ascending order)
      if (i + 1 < (int)st.steps.size() && st.steps[i + 1].mod >= 0) { rc = marks_reached(st.steps[i + 1].mod); if (rc) return rc; }
      switch (sp.kind) {
        case TS_HEAD: rc = head3_bwd(sp, d_out); if (rc) return rc; break;
        case TS_RES: rc = res3_bwd(sp, dtemb_act); if (rc) return rc; break;
        case TS_UP: {                                  // nearest x2: dx = the 2x2x2 block sums = 8 x the average pool
          const TT& tin = st.t[sp.in0];
          const int lvl = tin.H;
          int acc;
          float* dst = grad_dst(sp.in0, &acc);
          CSD_REQUIRE(!acc, "backward 3-D: internal error, the Upsample's input has a second consumer");
          TG_RUN(csd_avgpool3d_2_ndhwc(st.t[sp.out].g, dst, B, ext(0, lvl - 1), ext(1, lvl - 1), ext(2, lvl - 1), tin.C, s));
          rc = scale_into(dst, dst, 8.f, act3_n(lvl, tin.C)); if (rc) return rc;
          break;
        }
        case TS_DOWN: {                                // 2x2x2 average pool: dx (+)= nearest x2 of dy / 8 (its input is a skip tensor too)
          const TT& tin = st.t[sp.in0];
          const int lvl = tin.H;
          int acc;
          float* dst = grad_dst(sp.in0, &acc);
          if (!dry) {
            const size_t total = act3_n(lvl, tin.C);
            hipLaunchKernelGGL(avgpool3d_2_bwd_kernel, dim3(launch_blocks(total)), dim3(256), 0, s, st.t[sp.out].g, dst, ext(0, lvl), ext(1, lvl),
                               ext(2, lvl), tin.C, total, acc);
            CSD_LAUNCH_CHECK();
          }
          break;
        }
        case TS_STEM: {
          const Module& m = n.mods[sp.mod];
          const TT& to = st.t[sp.out];
          const int cio = c.x_channels + c.y_channels;
          rc = wgrad3(st.xin, to.g, DW(m.idx, "weight"), cio, nf, 0); if (rc) return rc;
          if (pg) {
            const size_t mk = top;
            float* bc = alloc((size_t)B * nf);
            rc = sum_vox(to.g, bc, nf, 0); if (rc) return rc;
            TG_RUN(sum_rows_beta(bc, DW(m.idx, "bias"), B, nf, gacc, s));
            top = mk;
          }
          // the data gradient, NDHWC -> NCDHW, the x channels only and the 2v - 1 map's factor in one kernel
          if (want_dx) TG_RUN(conv3d_stem_dx_launch(to.g, W(m.idx, "weight"), d_x, B, c.x_channels, cio, nf, ext(0, 0), ext(1, 0), ext(2, 0),
                                                    in_scale(), s));
          break;
        }
        default:
          CSD_REQUIRE(false, "backward 3-D: internal error, step kind %d", (int)sp.kind);
      }
    }
    if (pg) {                                          // temb MLP (models/ddpm3D.py:111-115)
      const size_t mk = top;
      float* d2 = alloc((size_t)B * 4 * nf);           // gradient w.r.t. temb2 = act'(temb2) * dtemb_act
      TG_RUN(csd_act(st.temb2, dtemb_act, d2, act, (int64_t)B * 4 * nf, s));
      float* dact1 = alloc((size_t)B * 4 * nf);
      if (!dry) CSD_CHECK_HIP(hipMemsetAsync(dact1, 0, (size_t)B * 4 * nf * sizeof(float), s));
      const int l0 = st.lin0, l1 = st.lin0 + 1;
      rc = linear_bwd(st.temb1, act, W(l1, "weight"), d2, DW(l1, "weight"), DW(l1, "bias"), dact1, 4 * nf, 4 * nf); if (rc) return rc;
      float* d1 = alloc((size_t)B * 4 * nf);
      TG_RUN(csd_act(st.temb1, dact1, d1, act, (int64_t)B * 4 * nf, s));
      rc = linear_bwd(st.emb, CSD_ACT_NONE, W(l0, "weight"), d1, DW(l0, "weight"), DW(l0, "bias"), nullptr, nf, 4 * nf); if (rc) return rc;
      top = mk;
    }
    return marks_reached(-1);
  }
};
#undef TG_RUN

static size_t train3d_workspace_peak(Net& net, int B, float dropout_p) {
  TrainState st;
  TG3 g(net, st, B, nullptr, true, nullptr, nullptr, reinterpret_cast<float*>(uintptr_t(256)));
  g.p_drop = dropout_p;
  g.want_dx = true;
  if (g.forward(nullptr, nullptr, nullptr, nullptr)) return 0;
  if (g.backward(nullptr)) return 0;
  return g.peak;
}

static int train3d_forward(Net& net, TrainState& st, int B, hipStream_t s, const float* const* params, float* ws, float p_drop, uint64_t seed,
                           uint64_t call, const float* x, const float* y, const float* labels, float* out) {
  TG3 g(net, st, B, s, false, params, nullptr, ws);
  g.p_drop = p_drop; g.seed = seed; g.call = call;
  return g.forward(x, y, labels, out);
}

static int train3d_backward(Net& net, TrainState& st, int B, hipStream_t s, const float* const* params, float* const* grads, float* ws,
                            float* d_x, int accumulate, GradMarks* gm, const float* d_out) {
  TG3 g(net, st, B, s, false, params, grads, ws);
  g.pg = grads != nullptr;
  g.gacc = accumulate;
  g.want_dx = d_x != nullptr;
  g.d_x = d_x;
  g.gm = gm;
  return g.backward(d_out);
}

}  // namespace csd
