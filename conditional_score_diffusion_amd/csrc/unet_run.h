// unet_run.h - run_plan: enqueue the launches of a plan.  No allocation, no synchronisation, no decision that the plan has not already
// taken.  Included by unet.hip.
#pragma once

namespace csd {

static int run_plan(Net& n, const Plan& pl, const float* pk, float* ws, const float* x, const float* y,
                    const float* labels, float* out, const float* y_noise, float y_sigma, hipStream_t s) {
  const csd_unet_config& c = n.cfg;
  const int B = pl.B, S = c.image_size;
  auto W = [&](size_t off) -> float* { return off == NONE ? nullptr : ws + off; };
  bool side_pending = false;
  // y_scale: the head's NCHW output goes to the plan's workspace tensor, the caller's `out` is filled behind the last op
  float* const out_caller = out;
  if (c.y_scale) out = W(pl.ys_out);
  for (const Op& o : pl.ops) {
    int rc = CSD_OK;
    // batch-chunk region: the chunk streams start behind everything enqueued so far; the caller's stream resumes behind all of them
    if (o.kind == OP_FORK) {
      if (!n.chunks_ready(o.n_chunks - 1)) { set_error("unet: cannot create the chunk streams"); return CSD_ERR_HIP; }
      CSD_CHECK_HIP(hipEventRecord(n.ev_cfork, s));
      for (int k = 0; k + 1 < o.n_chunks; ++k) CSD_CHECK_HIP(hipStreamWaitEvent(n.cstream[k], n.ev_cfork, 0));
      continue;
    }
    if (o.kind == OP_JOIN) {
      for (int k = 0; k + 1 < o.n_chunks; ++k) {
        CSD_CHECK_HIP(hipEventRecord(n.ev_cjoin[k], n.cstream[k]));
        CSD_CHECK_HIP(hipStreamWaitEvent(s, n.ev_cjoin[k], 0));
      }
      continue;
    }
    const int Bo = o.nb ? o.nb : B;
    // side-stream ops: fork after everything enqueued so far, join before the op that consumes the result
    hipStream_t so = o.stream ? n.cstream[o.stream - 1] : s;
    if (o.side == 1 && n.side_ready()) {
      CSD_CHECK_HIP(hipEventRecord(n.ev_fork, s));
      CSD_CHECK_HIP(hipStreamWaitEvent(n.side, n.ev_fork, 0));
      so = n.side;
    } else if (o.side == 2 && side_pending) {
      CSD_CHECK_HIP(hipStreamWaitEvent(s, n.ev_join, 0));
      side_pending = false;
    }
    ProfScope prof(o.cls, o.flops, o.bytes, so, o.abytes);
    switch (o.kind) {
      case OP_ASSEMBLE:
        rc = assemble_input_launch(x, y, y_noise, y_sigma, W(o.out), Bo, c.x_channels, c.y_channels, S * S,
                                   n.in_cpad, c.centered, so, c.x_squeeze, S, c.y_scale);
        break;
      case OP_STEM:
        rc = stem_launch(x, y, y_noise, y_sigma, pk + o.pk_w, pk + o.pk_b, W(o.out), reinterpret_cast<double*>(W(o.stats)), Bo,
                         c.x_channels, c.y_channels, o.Cout, S, c.centered, o.ns, so, c.x_squeeze, c.y_scale, W(o.out2));
        break;
      case OP_TEMB:
        rc = timestep_embedding_launch(labels, W(o.out), Bo, o.C0, so);
        break;
      case OP_FOURIER:
        rc = fourier_embedding_launch(labels, pk + o.pk_w, W(o.out), Bo, o.C0, so);
        break;
      case OP_FIR:
        rc = fir_resample_nhwc_launch(W(o.src0), W(o.out), Bo, o.H, o.W, o.C0, c.fir_kernel, o.up, so);
        break;
      case OP_FIR2:
        rc = fir_resample2_nhwc_launch(W(o.src0), W(o.nscale), W(o.nshift), W(o.out2), W(o.out), Bo, o.H, o.W, o.C0, c.fir_kernel, o.up, o.act, so);
        break;
      case OP_GN_APPLY32:
        rc = gn_apply_launch(W(o.src0), W(o.nscale), W(o.nshift), W(o.out), Bo, o.hw, o.C0, o.act, so);
        break;
      case OP_LINEAR:
        rc = linear_launch(W(o.src0), pk + o.pk_w, pk + o.pk_b, W(o.out), Bo, o.C0, o.Cout, o.act, so, o.out_act);
        break;
      case OP_GN_STATS:
        rc = gn_stats_launch(o.gp, W(o.src0), W(o.src1), reinterpret_cast<double*>(W(o.stats)), so, o.per_channel);
        break;
      case OP_GN_FINAL:
        rc = gn_finalize_launch(o.gp, reinterpret_cast<const double*>(W(o.stats)), pk + o.pk_w, pk + o.pk_b, 1e-6f, W(o.nscale), W(o.nshift), so);
        break;
      case OP_GN_FINAL_TILES:
        rc = gn_finalize_tiles_launch(reinterpret_cast<const double*>(W(o.stats)), o.tiles0, o.C0,
                                      reinterpret_cast<const double*>(W(o.stats1)), o.tiles1, o.C1, Bo, o.hw, o.gp.G, pk + o.pk_w, pk + o.pk_b, 1e-6f,
                                      W(o.nscale), W(o.nshift), so);
        break;
      case OP_GN_STATFIN:
        rc = gn_fused16_launch(W(o.src0), W(o.src1), o.gp.C0, o.gp.C1, pk + o.pk_w, pk + o.pk_b, 1e-6f, nullptr, nullptr, Bo, o.gp.HW, o.gp.G,
                               CSD_ACT_NONE, so, 0, W(o.nscale), W(o.nshift));
        break;
      case OP_GN_FUSED16:
        rc = gn_fused16_launch(W(o.src0), W(o.src1), o.C0, o.C1, pk + o.pk_w, pk + o.pk_b, 1e-6f, W(o.out), W(o.out2), Bo, o.hw, o.gp.G, o.act, so, o.fp8_lo);
        break;
      case OP_GN_APPLY16:
        rc = gn_apply16_launch(W(o.src0), W(o.src1), o.C0, o.C1, W(o.nscale), W(o.nshift), W(o.out), W(o.out2), Bo, o.hw, o.act, so, o.fp8_lo);
        break;
      case OP_CONV: {
        ConvArgs a;
        a.src0 = W(o.src0); a.src1 = W(o.src1);
        a.wpack = pk + o.pk_w; a.bias = o.pk_b == NONE ? nullptr : pk + o.pk_b;
        a.temb = o.temb_col == NONE ? nullptr : ws + o.temb_base + o.temb_col;
        a.res = W(o.res);
        a.nscale = W(o.nscale);
        a.nshift = W(o.nshift);
        a.out = o.out_external ? out : W(o.out);
        a.temb_stride = o.temb_stride;
        a.out_stride = o.cp.Cout; a.out_coff = 0;
        a.out_nchw = o.out_external;
        a.out_sq = (o.out_external && c.x_squeeze) ? c.x_channels : 0;
        a.act = o.act;
        a.out_scale = o.out_scale;
        a.dbg = nullptr;
        a.stats = reinterpret_cast<double*>(W(o.stats));
        switch (o.kernel) {
          case ConvKernel::FUSED: rc = convff_launch(o.cp, o.ns, a, so); break;
          case ConvKernel::QUAD: case ConvKernel::QUAD_UP4: rc = conv16q_launch(o.cp, o.ns, a, so, o.src_form == ConvSrc::SPLIT_STAGING); break;
          case ConvKernel::PW16: case ConvKernel::PW16_TAPS: rc = pw16_launch(o.cp, o.ns, a, so); break;
          case ConvKernel::F16_LC: rc = conv16_launch(o.cp, o.ns, a, so, o.src_form == ConvSrc::PLANES16); break;
          case ConvKernel::F32: rc = conv_launch(o.cp, a, so); break;
          case ConvKernel::STEM: set_error("unet: the fused stem is OP_STEM, not a convolution launch"); rc = CSD_ERR_STATE; break;
        }
        if (so == n.side && n.side != nullptr && rc == CSD_OK) {
          CSD_CHECK_HIP(hipEventRecord(n.ev_join, n.side));
          side_pending = true;
        }
        break;
      }
      case OP_ATTN:
        // fp16 arithmetic modes: the split-operand kernel on the fp16 matrix cores (fp32-class in the split modes); fp32 mode: the fp32 MFMA one
        rc = (precision_ns(c.precision) && !CSD_TUNE_ENV("CSD_ATTN_F32"))
                 ? attention16_launch(W(o.src0), 3 * o.C0, W(o.out), Bo, o.hw, o.C0, precision_ns(c.precision) >= 2 ? 2 : 1, so)
                 : attention_launch(W(o.src0), 3 * o.C0, W(o.out), Bo, o.hw, o.C0, so);
        break;
      case OP_AVGPOOL:
        rc = avgpool2_launch(W(o.src0), W(o.out), Bo, o.H, o.W, o.C0, so);
        break;
      case OP_UPNEAR:
        rc = nearest_up2_nhwc_launch(W(o.src0), W(o.out), Bo, o.H, o.W, o.C0, so);
        break;
      case OP_PYRCONV:
        rc = fir_pyr_conv_launch(W(o.src0), (int64_t)o.H * o.W * o.pix, o.pix, 1, Bo, o.H, o.C0, pk + o.pk_w, pk + o.pk_b, W(o.res), W(o.out), o.Cout,
                                 o.fir, o.out_scale, so);
        break;
      case OP_TAPSUM:
        rc = tapsum_launch(W(o.src0), pk + o.pk_b, W(o.res), o.out_external ? out : W(o.out), Bo, o.H, o.W, o.Cout, o.out_external, o.out_scale, so,
                           (o.out_external && c.x_squeeze) ? c.x_channels : 0);
        break;
      default:
        set_error("unet: unknown op");
        rc = CSD_ERR_STATE;
    }
    if (rc) return rc;
  }
  if (c.y_scale) {      // out[b] = the x block [Cx, S, S] as the head wrote it, then bilin_down of the other channels [., S / K, S / K]
    const size_t hw = (size_t)S * S, ld_src = (size_t)c.out_channels * hw, ld_dst = out_sample_elems(c);
    ProfScope prof(CSD_PROF_OTHER, 0, 2.0 * B * ld_src * 4, s);
    CSD_CHECK_HIP(hipMemcpy2DAsync(out_caller, ld_dst * 4, out, ld_src * 4, c.x_channels * hw * 4, B, hipMemcpyDeviceToDevice, s));
    if (c.out_channels > c.x_channels) {
      const int rc = bilinear_down_launch(out + c.x_channels * hw, ld_src, out_caller + c.x_channels * hw, ld_dst, B,
                                          c.out_channels - c.x_channels, S, c.y_scale, s);
      if (rc) return rc;
    }
  }
  return CSD_OK;
}

}  // namespace csd
