// pc_loop.h - the fused predictor-corrector sampler: its scratch, the noise-draw schedule, the loop of csd_pc_sample and its step,
// inpainting, colorization and cascade forms.  Host code only; the kernels are sampler.hip's.  Included by unet.hip behind Evaluator.
#pragma once

// ---- fused PC sampler -------------------------------------------------------------------------------
// HW below is the per-sample element count of one channel (sample_elems): image_size^2, or D*H*W for the 3-D family.
// scratch of csd_pc_* : net_out [B*Co*HW] | x_mean [B*Cx*HW] | z [B*Cx*HW] | zy [B*max(Cy,1)*HW] | labels [B] | ystate [B*max(Cy,1)*HW]
// (y_t of the use_path bridge) | the norm partials (double) [B*64*2] | the device flag of the finiteness contract.  A y_scale network
// needs less of net_out, zy and ystate (its y lives at S / K); the regions keep the full-resolution sizes.
struct PCScratch { float *net_out, *x_mean, *z, *zy, *labels, *ystate; double* partial; int* nonfinite; size_t bytes; };
static PCScratch pc_scratch(void* base, const csd_unet_config& cf, int B) {
  PCScratch L;
  const size_t hw = sample_elems(cf), ny = (size_t)B * std::max(cf.y_channels, 1) * hw;
  ScratchCarver c(base);
  L.net_out = c.take<float>((size_t)B * cf.out_channels * hw);
  L.x_mean = c.take<float>((size_t)B * cf.x_channels * hw);
  L.z = c.take<float>((size_t)B * cf.x_channels * hw);
  L.zy = c.take<float>(ny);
  L.labels = c.take<float>((size_t)B);
  L.ystate = c.take<float>(ny);
  L.partial = c.take<double>((size_t)B * 64 * 2);
  L.nonfinite = c.take<int>(1);
  L.bytes = c.bytes();
  return L;
}

extern "C" size_t csd_pc_scratch_bytes(const csd_unet* net, int B) { return net ? pc_scratch(nullptr, net->net.cfg, B).bytes : 0; }

__global__ void fill_labels_kernel(float* dst, float v, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) dst[i] = v;
}

// ---- the noise-draw schedule ------------------------------------------------------------------------------------------------------------
// The draws behind the prior form ONE sequence in the order the loop consumes them: draw j of it is Philox stream 1 + j (stream 0 is
// the caller's prior) and lies on the tape behind the draws before it.  A schedule is the optional draw in front of the loop plus the
// draws of one step in that order; every mode (plain, std_y, use_path, inpainting, colorization) is one list, built by pc_schedule below.
enum { DRAW_ZY0 = 0, DRAW_ZY_PATH = 1, DRAW_ZY = 2, DRAW_Z = 3, DRAW_BLEND = 4, DRAW_COLORIZE = 5 };      // the kinds of csd_pc_noise_draws (include/csd.h)
enum { BLEND_NONE = 0, BLEND_INPAINT = 1, BLEND_COLORIZE = 2 };      // what is re-imposed behind every phase (the `inpaint` argument of csd_pc_noise_draws)
// the re-imposition of a call: its mode and that mode's struct
struct PCBlend { int mode = BLEND_NONE; const csd_pc_inpaint_params* ip = nullptr; const csd_pc_colorize_params* cp = nullptr; };
// what a mode's refusals call its entries (csd_<entry>_sample / _step_begin / _step_end) and its constraint
static const char* const BLEND_ENTRY[] = {"pc_sample", "pc_inpaint", "pc_colorize"};
static const char* const BLEND_NOUN[] = {"", "inpainting", "colorization"};
enum { PHASE_CORRECTOR = 0, PHASE_PREDICTOR = 1, PHASE_NONE = 2 };
struct PCDraw { int kind, phase; size_t elems, offset; };      // offset: floats of the step's draws in front of it
struct PCDrawAt { size_t offset; uint64_t stream; size_t elems; };      // where one draw of one step is: tape offset and Philox stream

struct PCSchedule {
  size_t nx = 0, ny = 0;                             // elements of an x draw / a y draw (ny at S / K for a y_scale handle)
  bool path = false;                                 // use_path: y_t follows the bridge (csd_pc_params.path_coef)
  bool perturb_y = false;                            // std_y given: every evaluation draws its own y_t
  // a phase whose rule is 'none' (csd_pc_params.corrector / .predictor == 2) evaluates nothing and draws no update noise
  bool has[2] = {false, false};
  int order[2] = {PHASE_CORRECTOR, PHASE_PREDICTOR}; // execution order of the step's phases: the predictor first under use_path
  int n_pre = 0; size_t pre_elems = 0;               // the draw in front of the loop: z_y0 of use_path, or none
  PCDraw step[6]; int n_step = 0;                    // the draws of one step (at most [zy] z [z_blend | z_colorize] per phase)
  size_t step_elems = 0;
  void add(int kind, int phase, size_t elems) {
    step[n_step++] = PCDraw{kind, phase, elems, step_elems};
    step_elems += elems;
  }
  // the draw (kind, phase) of step i, step -1 = in front of the loop; stream 0 (the prior's): the schedule has no such draw
  PCDrawAt draw(int i, int kind, int phase) const {
    if (i < 0) return PCDrawAt{0, kind == DRAW_ZY0 && n_pre ? (uint64_t)1 : 0, pre_elems};
    for (int k = 0; k < n_step; ++k)
      if (step[k].kind == kind && step[k].phase == phase)
        return PCDrawAt{pre_elems + (size_t)i * step_elems + step[k].offset, (uint64_t)1 + n_pre + (uint64_t)i * n_step + k,
                        step[k].elems};
    return PCDrawAt{0, 0, 0};
  }
  bool evaluates_first(int phase) const { return phase == (has[order[0]] ? order[0] : order[1]); }      // (of the phases that exist)
  bool is_last(int phase) const { return phase == order[1]; }
};

// The schedule of a call with these rules and modes, and the ONE check of what they exclude (csd_pc_* and csd_pc_noise_draws).  The
// handle's refusals come first: an inpainting or colorization entry refuses the handle before it looks at another argument.
static int pc_schedule(PCSchedule* sc, const csd_unet* net, int B, int predictor, int corrector, bool std_y, bool path, int blend) {
  const csd_unet_config& cf = net->net.cfg;
  CSD_REQUIRE(blend >= BLEND_NONE && blend <= BLEND_COLORIZE, "pc_sample: bad inpaint mode %d (0 none, 1 inpainting, 2 colorization)", blend);
  const bool inpaint = blend == BLEND_INPAINT, colorize = blend == BLEND_COLORIZE;
  const char *entry = BLEND_ENTRY[blend], *noun = BLEND_NOUN[blend];
  if (blend != BLEND_NONE) {
    CSD_REQUIRE(!is3d(net->net), "%s: %s is not provided for the 3-D networks (arch 2) on the device loop", entry, noun);
    CSD_REQUIRE(!cf.x_squeeze, "%s: %s is not provided for a handle with x_squeeze (the 2x super-resolution networks are conditional)",
                entry, noun);
    CSD_REQUIRE(!cf.y_scale, "%s: %s is not provided for a handle with y_scale (the Kx super-resolution networks are conditional)",
                entry, noun);
  }
  CSD_REQUIRE(!(colorize && cf.y_channels != 0), "pc_colorize: colorization runs unconditional networks only (y_channels = %d)", cf.y_channels);
  CSD_REQUIRE(!(colorize && cf.x_channels != 3), "pc_colorize: colorization needs a 3-channel state (x_channels = %d)", cf.x_channels);
  CSD_REQUIRE(predictor >= 0 && predictor <= 2 && corrector >= 0 && corrector <= 2, "pc_sample: bad predictor / corrector id");
  CSD_REQUIRE(predictor != 2 || corrector != 2, "pc_sample: predictor and corrector are both 'none'");
  CSD_REQUIRE(!(std_y && cf.y_channels == 0), "pc_sample: std_y given for an unconditional network");
  CSD_REQUIRE(!inpaint || cf.y_channels == 0, "pc_inpaint: inpainting runs unconditional networks only (y_channels = %d)", cf.y_channels);
  CSD_REQUIRE(blend == BLEND_NONE || (!std_y && !path), "%s: std_y / path_coef belong to the conditional samplers", entry);
  CSD_REQUIRE(!path || (cf.y_channels > 0 && !std_y), "pc_sample: use_path needs a conditioning image and no marginal std_y");
  *sc = PCSchedule();
  // (y_scale = K: y, its noise and the bridge's y_t live at S / K; a sample of net_out is the x block, then the downsampled y block)
  const size_t hw = sample_elems(cf), hwy = cf.y_scale ? hw / ((size_t)cf.y_scale * cf.y_scale) : hw;
  sc->nx = (size_t)B * cf.x_channels * hw; sc->ny = (size_t)B * cf.y_channels * hwy;
  sc->path = path; sc->perturb_y = std_y;
  sc->has[PHASE_CORRECTOR] = corrector != 2; sc->has[PHASE_PREDICTOR] = predictor != 2;
  if (path) {                                        // z_y0 | per step: z_y of the bridge, then the predictor FIRST
    sc->order[0] = PHASE_PREDICTOR; sc->order[1] = PHASE_CORRECTOR;
    sc->n_pre = 1; sc->pre_elems = sc->ny;
    sc->add(DRAW_ZY_PATH, PHASE_NONE, sc->ny);
  }
  for (int phase : sc->order) {
    if (sc->has[phase]) {
      if (std_y) sc->add(DRAW_ZY, phase, sc->ny);
      sc->add(DRAW_Z, phase, sc->nx);                // (a probability-flow predictor still consumes its draw)
    }
    if (inpaint) sc->add(DRAW_BLEND, phase, sc->nx); // behind every phase, a 'none' phase included
    if (colorize) sc->add(DRAW_COLORIZE, phase, sc->nx);      // the same place; a full-size draw whose channel 0 is used
  }
  return CSD_OK;
}

extern "C" int64_t csd_pc_noise_draws(const csd_unet* net, int B, int predictor, int corrector, int has_std_y, int has_path_coef,
                                      int inpaint, int n_steps, int64_t* rows, int cap) {
  CSD_REQUIRE(net && B >= 1 && n_steps >= 1 && cap >= 0 && (rows || cap == 0), "pc_noise_draws: null handle / rows, or bad B, n_steps, cap");
  PCSchedule sc;
  int rc = pc_schedule(&sc, net, B, predictor, corrector, has_std_y != 0, has_path_coef != 0, inpaint);
  if (rc) return rc;
  int64_t n = 0;
  auto row = [&](int i, const PCDraw& d) {
    const PCDrawAt at = sc.draw(i, d.kind, d.phase);
    if (n < cap) {
      const int64_t r[6] = {i, d.kind, d.phase, (int64_t)at.elems, (int64_t)at.offset, (int64_t)at.stream};
      std::copy(r, r + 6, rows + 6 * n);
    }
    ++n;
  };
  if (sc.n_pre) row(-1, PCDraw{DRAW_ZY0, PHASE_NONE, sc.pre_elems, 0});
  for (int i = 0; i < n_steps; ++i)
    for (int k = 0; k < sc.n_step; ++k) row(i, sc.step[k]);
  return n;
}

// one validated view of a csd_pc_* call: scratch carved up, the draw schedule
struct PCCtx : PCScratch, PCSchedule {
  Evaluator ev; const float* pk; float* ws;
  const csd_pc_params* p;
  // what the call re-imposes after every phase: the known pixels (csd_pc_inpaint_*), the gray channel (csd_pc_colorize_*) or nothing
  PCBlend bl;
  float* x; const float* y;
  int B, nchunk;
  int64_t per, net_stride;
  hipStream_t s;
  // a scheduled draw: its place on the tape (reference order), or its Philox stream filled into dst
  const float* noise(const PCDrawAt& d, float* dst) const {
    if (!d.stream) { set_error("pc_sample: a draw outside the schedule"); return nullptr; }
    if (p->noise_tape) return p->noise_tape + d.offset;
    if (randn_launch(dst, (int64_t)d.elems, p->seed, d.stream, s)) return nullptr;
    return dst;
  }
};

static int pc_setup(PCCtx* c, csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                    size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p, void* stream,
                    const PCBlend& bl = PCBlend()) {
  int rc = CSD_OK;
  if (net && p && (rc = pc_schedule(c, net, B, p->predictor, p->corrector, p->std_y != nullptr, p->path_coef != nullptr, bl.mode))) return rc;
  if ((rc = check_forward_args(net, packed, workspace, workspace_bytes, B, &c->ev))) return rc;
  CSD_REQUIRE(p && x && scratch, "pc_sample: null argument");
  CSD_REQUIRE(p->n_steps >= 1 && p->labels && p->std_x, "pc_sample: per-step scalar arrays missing");
  CSD_REQUIRE(p->predictor != 0 || p->G, "pc_sample: the reverse-diffusion predictor needs G");
  CSD_REQUIRE(p->predictor != 1 || p->pred_coef, "pc_sample: predictor table missing");
  CSD_REQUIRE(p->corrector != 1 || p->corr_coef, "pc_sample: corrector table missing");
  CSD_REQUIRE(p->predictor == 0 || (!p->rd_drift && !p->probability_flow),
              "pc_sample: rd_drift / probability_flow belong to the reverse-diffusion predictor (an affine table carries its own)");
  CSD_REQUIRE((p->rd_sub_x == 0 || p->rd_sub_x == 1) && (p->probability_flow == 0 || p->probability_flow == 1) &&
              (p->rd_sub_x == 0 || p->rd_drift), "pc_sample: bad rd_sub_x / probability_flow");
  const csd_unet_config& cf = net->net.cfg;
  CSD_REQUIRE((cf.y_channels == 0) == (y == nullptr), "pc_sample: y must be given iff y_channels > 0");
  if (scratch_bytes < csd_pc_scratch_bytes(net, B)) {
    set_error("pc_sample: scratch too small");
    return CSD_ERR_WORKSPACE;
  }
  CSD_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "pc_sample: scratch must be 256-byte aligned");
  const size_t hw = sample_elems(cf);
  c->pk = static_cast<const float*>(packed); c->ws = static_cast<float*>(workspace);
  c->p = p; c->x = x; c->y = y; c->B = B; c->s = (hipStream_t)stream;
  const csd_pc_inpaint_params* ip = bl.ip;
  const csd_pc_colorize_params* cp = bl.cp;
  CSD_REQUIRE(bl.mode != BLEND_INPAINT || (ip && ip->data && ip->mask && ip->mean_scale && ip->std),
              "pc_inpaint: data, mask, mean_scale and std are required");
  CSD_REQUIRE(bl.mode != BLEND_COLORIZE || (cp && cp->gray0 && cp->mean_scale && cp->std), "pc_colorize: gray0, mean_scale and std are required");
  c->bl = bl;
  static_cast<PCScratch&>(*c) = pc_scratch(scratch, cf, B);
  c->per = (int64_t)cf.x_channels * hw;
  c->nchunk = sumsq_nchunk(c->per);
  // paired networks emit [score_x | score_y] per sample: the x block of sample b starts at b*out_channels*hw
  c->net_stride = (int64_t)out_sample_elems(cf);
  return CSD_OK;
}

// inpainting: re-impose the known pixels behind the update of a phase (sampling/unconditional.py:268-271).  The blend's draw follows
// the phase's own; without a tape the kernel makes it in registers.  x_mean is only ever read after the last predictor phase.
// colorization: the gray channel instead, in the decoupled channel space (colorize_blend_kernel); its draw stands where the blend's does.
static int pc_blend(const PCCtx& c, int i, int phase) {
  const csd_pc_params* p = c.p;
  float* mean = (phase == 1 && i == p->n_steps - 1 && p->denoise) ? c.x_mean : nullptr;
  const PCDrawAt d = c.draw(i, c.bl.mode == BLEND_COLORIZE ? DRAW_COLORIZE : DRAW_BLEND, phase);
  const float* z = p->noise_tape ? p->noise_tape + d.offset : nullptr;
  switch (c.bl.mode) {
    case BLEND_INPAINT: {
      const csd_pc_inpaint_params& ip = *c.bl.ip;
      ProfScope prof(CSD_PROF_SAMPLER, 0, (z ? 5.0 : 4.0) * c.nx * 4, c.s);
      return inpaint_blend_launch(c.x, mean, ip.data, ip.mask, z, ip.mean_scale[i], ip.std[i], c.nx, p->seed, d.stream, c.s);
    }
    case BLEND_COLORIZE: {
      const csd_pc_colorize_params& cp = *c.bl.cp;
      const size_t hw = c.nx / ((size_t)c.B * 3);
      ProfScope prof(CSD_PROF_SAMPLER, 0, ((z ? 7.0 : 6.0) + 1.0) * c.nx * 4 / 3, c.s);
      return colorize_blend_launch(c.x, mean, cp.gray0, z, cp.mean_scale[i], cp.std[i], c.B, hw, 0, cp.matrix, cp.inv_matrix, p->seed,
                                   d.stream, c.s);
    }
  }
  return CSD_OK;                                   // BLEND_NONE: nothing to re-impose
}

// phase 0: corrector (sampling/conditional.py:208-209), phase 1: predictor (:211).  part bit 0: network + noise + (corrector:
// norm partials); bit 1: the update.  norm_sums != null: the corrector's step size comes from those two (all-reduced) sums.
static int pc_phase(const PCCtx& c, int i, int phase, int part, float* sums_out, const float* sums_in, int Bg) {
  int rc;
  const csd_pc_params* p = c.p;
  if (!c.has[phase]) {                       // 'none': x stays, x_mean = x (sampling/predictors.py:182-200, correctors.py:145-163)
    if (c.bl.mode != BLEND_NONE) return (part & 2) ? pc_blend(c, i, phase) : CSD_OK;      // (the reference wraps the 'none' update functions as well)
    if ((part & 2) && c.is_last(phase) && i == p->n_steps - 1 && p->denoise)
      CSD_CHECK_HIP(hipMemcpyAsync(c.x_mean, c.x, c.nx * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    return CSD_OK;
  }
  const PCDrawAt dz = c.draw(i, DRAW_Z, phase);
  const float* zp = p->noise_tape ? p->noise_tape + dz.offset : c.z;       // (part 2 alone: the z that part 1 drew)
  if (part & 1) {
    if (c.evaluates_first(phase)) {                // (the labels: once per step)
      hipLaunchKernelGGL(fill_labels_kernel, dim3(cdiv(c.B, 256)), dim3(256), 0, c.s, c.labels, p->labels[i], c.B);
      CSD_LAUNCH_CHECK();
    }
    const float* zyp = nullptr;
    if (c.perturb_y) { zyp = c.noise(c.draw(i, DRAW_ZY, phase), c.zy); if (!zyp) return CSD_ERR_HIP; }
    rc = c.ev.run(c.pk, c.ws, c.x, c.path ? c.ystate : c.y, c.labels, c.net_out, zyp, c.perturb_y ? p->std_y[i] : 0.f, c.s);
    if (rc) return rc;
    zp = c.noise(dz, c.z);
    if (!zp) return CSD_ERR_HIP;
    if (phase == 0 && p->corrector == 0) {
      ProfScope prof(CSD_PROF_SAMPLER, 0, 2.0 * c.nx * 4, c.s);
      if ((rc = sumsq_rows_launch(c.net_out, c.net_stride, zp, c.partial, c.B, c.per, c.nchunk, c.s))) return rc;
      if (sums_out && (rc = norm_sums_launch(c.partial, c.nchunk, p->std_x[i], c.B, sums_out, c.s))) return rc;
    }
  }
  if (part & 2) {
    ProfScope prof(CSD_PROF_SAMPLER, 0, 6.0 * c.nx * 4, c.s);
    const int rule = phase == 0 ? p->corrector : p->predictor;
    if (rule == 1) {                               // affine table: x_mean = p x + a score, x = x_mean + b z
      const float* co = (phase == 0 ? p->corr_coef : p->pred_coef) + (size_t)i * 3;
      rc = affine_net_update_launch(c.x, c.x_mean, c.net_out, c.net_stride, zp, p->std_x[i], co[0], co[1], co[2], c.B, c.per, c.s);
    } else if (phase == 0) {
      const float alpha = p->corr_alpha ? p->corr_alpha[i] : 1.0f;      // sde.alphas[timestep] (VP / subVP); 1 for the VE SDEs
      rc = sums_in ? langevin_update_global_launch(c.x, c.x_mean, c.net_out, c.net_stride, zp, sums_in, Bg, p->std_x[i], p->snr,
                                                   alpha, c.B, c.per, c.s, c.nonfinite)
                   : langevin_update_launch(c.x, c.x_mean, c.net_out, c.net_stride, zp, c.partial, c.nchunk, p->std_x[i],
                                            p->snr, alpha, c.B, c.per, c.s, c.nonfinite);
    } else if (p->rd_drift || p->probability_flow) {      // a forward drift (VP / sub-VP) and / or the probability flow
      const float* d = p->rd_drift ? p->rd_drift + (size_t)i * 2 : nullptr;
      const bool pf = p->probability_flow != 0;
      rc = reverse_diffusion_drift_update_launch(c.x, c.x_mean, c.net_out, c.net_stride, zp, p->std_x[i], p->G[i], d ? d[0] : 0.f,
                                                 d ? d[1] : 0.f, d != nullptr, p->rd_sub_x, pf ? 0.5f : 1.f, pf ? 0.f : p->G[i],
                                                 c.B, c.per, c.s);
    } else {
      rc = reverse_diffusion_update_launch(c.x, c.x_mean, c.net_out, c.net_stride, zp, p->std_x[i], p->G[i], c.B, c.per, c.s);
    }
    if (rc) return rc;
    if ((rc = pc_blend(c, i, phase))) return rc;
  }
  return CSD_OK;
}

static int pc_step_tail(const PCCtx& c, int i) {
  const csd_pc_params* p = c.p;
  if (p->record)
    CSD_CHECK_HIP(hipMemcpyAsync(p->record + (size_t)i * c.nx, c.x, c.nx * sizeof(float), hipMemcpyDeviceToDevice, c.s));
  if (i == p->n_steps - 1 && p->denoise)
    CSD_CHECK_HIP(hipMemcpyAsync(c.x, c.x_mean, c.nx * sizeof(float), hipMemcpyDeviceToDevice, c.s));
  return CSD_OK;
}

// The finiteness contract of the fused loop (BASELINE.json north_star: outputs within 1e-3 of the reference - a NaN image is not):
// every Langevin step's norms and one pass over the returned state set a device flag; the loop's LAST call reads it back behind the
// stream (the only synchronisation of the sampler) and fails with CSD_ERR_NONFINITE instead of returning NaN images silently.
static int pc_read_flag(const PCCtx& c) {
  int flag = 0;
  CSD_CHECK_HIP(hipMemcpyAsync(&flag, c.nonfinite, sizeof(int), hipMemcpyDeviceToHost, c.s));
  CSD_CHECK_HIP(hipStreamSynchronize(c.s));
  if (flag) {
    set_error("pc_sample: the sampler's state or a corrector norm is not finite - an operand of an fp16-operand mode (fp16x3 / fp16f8 / fp16) "
              "left the fp16 range (65504); run this network with csd_precision = 'fp32'");
    return CSD_ERR_NONFINITE;
  }
  return CSD_OK;
}

static int pc_finish(const PCCtx& c) {
  int rc = finite_check_launch(c.x, c.nx, c.nonfinite, c.s);
  if (rc) return rc;
  return pc_read_flag(c);
}

// The whole loop of a validated call, enqueued: the flag cleared, every step, the pass over the returned state.  Nothing here waits for
// the device: csd_pc_sample / csd_pc_inpaint_sample read the flag back behind it (pc_read_flag), csd_pc_cascade_sample enqueues the
// next stage first and reads every stage's flag behind the last one.
static int pc_enqueue(const PCCtx& c) {
  int rc;
  const csd_pc_params* p = c.p;
  CSD_CHECK_HIP(hipMemsetAsync(c.nonfinite, 0, sizeof(int), c.s));
  if (c.path) {                                 // y_{T+tau} = y + sigma_y(T+tau) z (sampling/conditional.py:146-149)
    const float* z0 = c.noise(c.draw(-1, DRAW_ZY0, PHASE_NONE), c.zy);
    if (!z0) return CSD_ERR_HIP;
    if ((rc = bridge_update_launch(c.y, c.ystate, z0, 1.f, 0.f, p->path_std0, 0, c.ny, c.s))) return rc;
  }
  for (int i = 0; i < p->n_steps; ++i) {
    g_prof.step_on = (i % g_prof.step_stride) == 0;
    if (c.path) {                               // y_t from the bridge; both phases then run on the same y_t (:151-170)
      const float* zy = c.noise(c.draw(i, DRAW_ZY_PATH, PHASE_NONE), c.zy);
      if (!zy) return CSD_ERR_HIP;
      const float* co = p->path_coef + (size_t)i * 3;
      if ((rc = bridge_update_launch(c.y, c.ystate, zy, co[0], co[1], co[2], 1, c.ny, c.s))) return rc;
    }
    for (int phase : c.order)                   // corrector, then predictor (sampling/conditional.py:208-211); use_path: the reverse
      if ((rc = pc_phase(c, i, phase, 3, nullptr, nullptr, 0))) return rc;
    if ((rc = pc_step_tail(c, i))) return rc;
  }
  g_prof.step_on = true;
  return finite_check_launch(c.x, c.nx, c.nonfinite, c.s);
}

static int pc_sample_run(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                         size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                         const PCBlend& bl, void* stream) {
  PCCtx c;
  int rc = pc_setup(&c, net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, stream, bl);
  if (rc) return rc;
  if ((rc = pc_enqueue(c))) return rc;
  return pc_read_flag(c);
}

static int pc_step_begin_run(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                             size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                             const PCBlend& bl, int step, float* norm_sums, void* stream) {
  PCCtx c;
  int rc = pc_setup(&c, net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, stream, bl);
  if (rc) return rc;
  CSD_REQUIRE(norm_sums && step >= 0 && step < p->n_steps, "pc_step_begin: bad step %d / null norm_sums", step);
  CSD_REQUIRE(!c.path, "pc_step_begin: use_path runs through csd_pc_sample only");
  if (step == 0) CSD_CHECK_HIP(hipMemsetAsync(c.nonfinite, 0, sizeof(int), c.s));
  return pc_phase(c, step, 0, 1, norm_sums, nullptr, 0);
}

static int pc_step_end_run(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                           size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                           const PCBlend& bl, int step, const float* norm_sums, int global_batch, void* stream) {
  PCCtx c;
  int rc = pc_setup(&c, net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, stream, bl);
  if (rc) return rc;
  CSD_REQUIRE(norm_sums && global_batch >= B && step >= 0 && step < p->n_steps, "pc_step_end: bad arguments");
  if ((rc = pc_phase(c, step, 0, 2, nullptr, norm_sums, global_batch))) return rc;
  if ((rc = pc_phase(c, step, 1, 3, nullptr, nullptr, 0))) return rc;
  if ((rc = pc_step_tail(c, step))) return rc;
  return step == p->n_steps - 1 ? pc_finish(c) : CSD_OK;
}

extern "C" int csd_pc_sample(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes,
                             void* scratch, size_t scratch_bytes, float* x, const float* y, int B,
                             const csd_pc_params* p, void* stream) {
  return pc_sample_run(net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, PCBlend(), stream);
}

extern "C" int csd_pc_step_begin(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                                 size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p, int step,
                                 float* norm_sums, void* stream) {
  return pc_step_begin_run(net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, PCBlend(), step, norm_sums,
                           stream);
}

extern "C" int csd_pc_step_end(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                               size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p, int step,
                               const float* norm_sums, int global_batch, void* stream) {
  return pc_step_end_run(net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, PCBlend(), step, norm_sums,
                         global_batch, stream);
}

// ---- inpainting on the same loop (include/csd.h: csd_pc_inpaint_params) -------------------------------------------------------------
extern "C" size_t csd_pc_inpaint_scratch_bytes(const csd_unet* net, int B) { return csd_pc_scratch_bytes(net, B); }      // (the blend needs no buffer)

extern "C" int csd_pc_inpaint_sample(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                                     size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                                     const csd_pc_inpaint_params* ip, void* stream) {
  return pc_sample_run(net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, PCBlend{BLEND_INPAINT, ip, nullptr}, stream);
}

extern "C" int csd_pc_inpaint_step_begin(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                                         size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                                         const csd_pc_inpaint_params* ip, int step, float* norm_sums, void* stream) {
  return pc_step_begin_run(net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, PCBlend{BLEND_INPAINT, ip, nullptr}, step,
                           norm_sums, stream);
}

extern "C" int csd_pc_inpaint_step_end(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                                       size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                                       const csd_pc_inpaint_params* ip, int step, const float* norm_sums, int global_batch,
                                       void* stream) {
  return pc_step_end_run(net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, PCBlend{BLEND_INPAINT, ip, nullptr}, step,
                         norm_sums, global_batch, stream);
}

// ---- colorization on the same loop (include/csd.h: csd_pc_colorize_params) ----------------------------------------------------------
extern "C" int csd_pc_colorize_sample(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                                      size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                                      const csd_pc_colorize_params* cp, void* stream) {
  return pc_sample_run(net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, PCBlend{BLEND_COLORIZE, nullptr, cp}, stream);
}

extern "C" int csd_pc_colorize_step_begin(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                                          size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                                          const csd_pc_colorize_params* cp, int step, float* norm_sums, void* stream) {
  return pc_step_begin_run(net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, PCBlend{BLEND_COLORIZE, nullptr, cp},
                           step, norm_sums, stream);
}

extern "C" int csd_pc_colorize_step_end(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                                        size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                                        const csd_pc_colorize_params* cp, int step, const float* norm_sums, int global_batch,
                                        void* stream) {
  return pc_step_end_run(net, packed, workspace, workspace_bytes, scratch, scratch_bytes, x, y, B, p, PCBlend{BLEND_COLORIZE, nullptr, cp},
                         step, norm_sums, global_batch, stream);
}

// ---- sequential cascades (include/csd.h: csd_cascade_stage, csd_pc_cascade_sample) ----------------------------------------------------
// Every stage is validated and set up (pc_setup) before the first kernel is enqueued; the stages then run pc_enqueue back to back on
// the one stream, each with its flag of the finiteness contract in stage_flags[k], and the flags are read back once behind the last.
static inline size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

// a pc_setup / launch failure of stage k keeps its text, behind the stage's index
static int cascade_fail(int rc, int k, int n) {
  const std::string why = get_error();
  set_error("pc_cascade: stage %d of %d (stages[%d]): %s", k + 1, n, k, why.c_str());
  return rc;
}

extern "C" int csd_pc_cascade_sample(const csd_cascade_stage* st, int n, int final_link, const float* y0, int B, void* workspace,
                                     size_t workspace_bytes, void* scratch, size_t scratch_bytes, int32_t* stage_flags,
                                     const float* band_matrix, void* stream) {
  CSD_REQUIRE(st && n >= 1 && n <= 64, "pc_cascade: null stages / bad n_stages %d", n);
  CSD_REQUIRE(B >= 1 && workspace && scratch && stage_flags, "pc_cascade: B = %d / a null workspace, scratch or stage_flags", B);
  CSD_REQUIRE(final_link >= 0 && final_link <= 2, "pc_cascade: bad final_link %d", final_link);
  CSD_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "pc_cascade: scratch must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
#define STAGE_REQUIRE(cond, fmt, ...) CSD_REQUIRE(cond, "pc_cascade: stage %d of %d (stages[%d]): " fmt, k + 1, n, k, ##__VA_ARGS__)
  // 1. what each stage is, and the extents at every link
  size_t pc_bytes = 0, hand_bytes = 0;
  int pc_stage = 0;
  for (int k = 0; k < n; ++k) {
    const csd_cascade_stage& g = st[k];
    STAGE_REQUIRE(g.net && g.packed && g.pc && g.x, "null handle, packed weights, pc params or x");
    const csd_unet_config& cf = g.net->net.cfg;
    STAGE_REQUIRE(!is3d(g.net->net), "3-D handles (arch 2) do not run in a cascade");
    STAGE_REQUIRE(!cf.y_scale, "handles with y_scale (the Kx networks) do not run in a cascade");
    STAGE_REQUIRE(!(cf.y_channels > 0 && g.inpaint), "a conditional stage (y_channels = %d) was given inpaint params", cf.y_channels);
    STAGE_REQUIRE(!(cf.y_channels == 0 && !g.inpaint), "an unconditional stage needs inpaint params");
    STAGE_REQUIRE(!g.inpaint || (g.inpaint->data && g.inpaint->mask), "inpaint params without data / mask");
    STAGE_REQUIRE(g.link >= 0 && g.link <= 2 && (k > 0 || g.link == 0), "bad link %d%s", g.link, k == 0 ? " (stage 1 takes y0: link 0)" : "");
    if (k == 0) {
      STAGE_REQUIRE((cf.y_channels > 0) == (y0 != nullptr), "y0 must be given iff the stage has a condition (y_channels = %d)", cf.y_channels);
    } else {
      const csd_unet_config& pf = st[k - 1].net->net.cfg;
      const int pS = pf.image_size, S = cf.image_size;
      if (g.link == 0) {
        const int ci = pf.x_squeeze ? pf.x_channels / 4 : pf.x_channels, side = pf.x_squeeze ? 2 * pS : pS;
        STAGE_REQUIRE(cf.y_channels == ci && S == side, "link 0: the previous stage's x is %d x %d^2, this stage's y %d x %d^2", ci, side,
                      cf.y_channels, S);
      } else if (g.link == 1) {
        const int C = pf.y_channels;
        STAGE_REQUIRE(C > 0 && !pf.x_squeeze && pf.x_channels == 3 * C && cf.y_channels == C && S == 2 * pS,
                      "link 1: needs previous y C x S^2, previous x 3C x S^2 and this y C x (2S)^2; got previous y %d, x %d at %d^2 "
                      "(x_squeeze %d), this y %d at %d^2", pf.y_channels, pf.x_channels, pS, pf.x_squeeze, cf.y_channels, S);
      } else {
        STAGE_REQUIRE(st[k - 1].inpaint && g.inpaint, "link 2 joins two inpainting stages");
        STAGE_REQUIRE(pf.x_channels % 4 == 0 && !pf.x_squeeze && !cf.x_squeeze && cf.x_channels == pf.x_channels && S == 2 * pS,
                      "link 2: needs previous x 4C x S^2 and this x 4C x (2S)^2; got previous x %d at %d^2, this x %d at %d^2",
                      pf.x_channels, pS, cf.x_channels, S);
        STAGE_REQUIRE(!st[k - 1].out, "link 2 writes the merged image into this stage's data: the previous stage's out must be NULL");
      }
    }
    if (k == n - 1 && final_link) {
      if (final_link == 1)
        STAGE_REQUIRE(cf.y_channels > 0 && !cf.x_squeeze && cf.x_channels == 3 * cf.y_channels, "final_link 1: needs y C, x 3C; got y %d, x %d",
                      cf.y_channels, cf.x_channels);
      else
        STAGE_REQUIRE(g.inpaint && !cf.x_squeeze && cf.x_channels % 4 == 0, "final_link 2: needs an inpainting stage with x 4C; got x %d",
                      cf.x_channels);
      STAGE_REQUIRE(g.out, "final_link %d: the last stage's out is required", final_link);
    }
    const size_t pcb = round256(csd_pc_scratch_bytes(g.net, B));
    if (pcb > pc_bytes) { pc_bytes = pcb; pc_stage = k; }
    if (k + 1 < n && st[k + 1].link == 1 && !g.out)
      hand_bytes += round256((size_t)B * std::max(cf.y_channels, 0) * 4 * sample_elems(cf) * sizeof(float));
  }
  // 2. the two shared buffers
  for (int k = 0; k < n; ++k) {
    const size_t need = csd_unet_workspace_bytes(st[k].net, B);
    if (workspace_bytes < need) {
      set_error("pc_cascade: stage %d of %d (stages[%d]): workspace too small: %zu bytes, the stage needs %zu", k + 1, n, k, workspace_bytes, need);
      return CSD_ERR_WORKSPACE;
    }
  }
  if (scratch_bytes < pc_bytes + hand_bytes) {
    set_error("pc_cascade: stage %d of %d (stages[%d]): scratch too small: %zu bytes; the stage's loop needs %zu and the hand-over images "
              "without a caller buffer %zu", pc_stage + 1, n, pc_stage, scratch_bytes, pc_bytes, hand_bytes);
    return CSD_ERR_WORKSPACE;
  }
  // 3. every stage's condition pointer and validated loop, before anything is enqueued
  std::vector<PCCtx> ctx(n);
  std::vector<float*> handed(n, nullptr);              // stage k's merged image, where a link 1 / final link makes one
  char* hand = static_cast<char*>(scratch) + pc_bytes;
  for (int k = 0; k < n; ++k) {
    const csd_cascade_stage& g = st[k];
    const csd_unet_config& cf = g.net->net.cfg;
    const float* y = nullptr;
    if (k == 0) y = y0;
    else if (g.link == 0) y = st[k - 1].x;
    else if (g.link == 1) y = handed[k - 1];
    if (k + 1 < n && st[k + 1].link == 1) {
      handed[k] = g.out;
      if (!g.out) {
        handed[k] = reinterpret_cast<float*>(hand);
        hand += round256((size_t)B * cf.y_channels * 4 * sample_elems(cf) * sizeof(float));
      }
    } else if (k == n - 1 && final_link) {
      handed[k] = g.out;
    }
    int rc = pc_setup(&ctx[k], g.net, g.packed, workspace, workspace_bytes, scratch, pc_bytes, g.x, y, B, g.pc, stream,
                      PCBlend{g.inpaint ? BLEND_INPAINT : BLEND_NONE, g.inpaint, nullptr});
    if (rc) return cascade_fail(rc, k, n);
    STAGE_REQUIRE(!ctx[k].path, "use_path (pc->path_coef) does not run in a cascade");
    ctx[k].nonfinite = stage_flags + k;
  }
#undef STAGE_REQUIRE
  // 4. enqueue: [the link's merge] the stage's loop ... [the final merge]; then the one synchronisation
  auto merge_of = [&](int k, float* dst, size_t dst_ld) -> int {      // stage k's bands -> the image of twice its side
    const csd_unet_config& cf = st[k].net->net.cfg;
    const size_t hw = sample_elems(cf);
    ProfScope prof(CSD_PROF_OTHER, 0, 2.0 * B * (st[k].inpaint ? cf.x_channels : 4 * cf.y_channels) * hw * 4, s);
    if (st[k].inpaint) {
      const int C = cf.x_channels / 4;
      const int64_t ld = (int64_t)cf.x_channels * hw;
      return band_merge_launch(st[k].inpaint->data, ld, st[k].x + (size_t)C * hw, ld, dst, (int64_t)dst_ld, B, C, cf.image_size, band_matrix, s);
    }
    const int C = cf.y_channels;
    return band_merge_launch(ctx[k].y, (int64_t)C * hw, st[k].x, (int64_t)3 * C * hw, dst, (int64_t)dst_ld, B, C, cf.image_size, band_matrix, s);
  };
  for (int k = 0; k < n; ++k) {
    int rc = CSD_OK;
    const csd_unet_config& cf = st[k].net->net.cfg;
    if (k > 0 && st[k].link == 1) {
      rc = merge_of(k - 1, handed[k - 1], (size_t)cf.y_channels * sample_elems(cf));
    } else if (k > 0 && st[k].link == 2) {
      float* data = const_cast<float*>(st[k].inpaint->data);
      if (hipMemsetAsync(data, 0, ctx[k].nx * sizeof(float), s) != hipSuccess) {
        set_error("hipMemsetAsync of the stage's data failed");
        rc = CSD_ERR_HIP;
      }
      if (!rc) rc = merge_of(k - 1, data, (size_t)cf.x_channels * sample_elems(cf));
      if (!rc) rc = inpaint_blend_launch(st[k].x, nullptr, data, st[k].inpaint->mask, nullptr, 1.f, 0.f, ctx[k].nx, 0, 0, s);
    }
    if (!rc) rc = pc_enqueue(ctx[k]);
    if (!rc && k == n - 1 && final_link)
      rc = merge_of(k, handed[k], (size_t)(st[k].inpaint ? cf.x_channels / 4 : cf.y_channels) * 4 * sample_elems(cf));
    if (rc) return cascade_fail(rc, k, n);
  }
  std::vector<int32_t> flags(n, 0);
  CSD_CHECK_HIP(hipMemcpyAsync(flags.data(), stage_flags, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  CSD_CHECK_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < n; ++k)
    if (flags[k]) {
      set_error("pc_cascade: stage %d of %d (stages[%d]): the sampler's state or a corrector norm is not finite (stage_flags[%d] = %d; the "
                "stages before it stayed finite, the ones behind it ran on its result) - a non-finite condition or prior, or an operand of "
                "an fp16-operand mode beyond 65504: run that network with csd_precision = 'fp32'", k + 1, n, k, k, (int)flags[k]);
      return CSD_ERR_NONFINITE;
    }
  return CSD_OK;
}
