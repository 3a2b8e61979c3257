/*
 * csd.h - C ABI of libcsd_hip.so: the MI355X (gfx950) score-network + predictor-corrector
 * sampler hot path of GBATZOLIS/conditional_score_diffusion.
 *
 * Conventions:
 *   - extern "C", plain pointers and sizes; no C++/torch types cross the boundary.
 *   - every function returns 0 on success or a negative csd_status; csd_last_error() gives the
 *     text of the calling thread's last failure.  Nothing throws.
 *   - the CALLER owns every device buffer (inputs, outputs, packed weights, workspace); the
 *     library owns only opaque host-side handles.  All work is enqueued on the caller's
 *     hipStream_t (passed as void*) and never synchronises it, except where stated.
 *   - boundary tensors are the reference's: NCHW fp32 contiguous.  (Internally activations are
 *     NHWC fp32; that layout never leaks.)
 *   - one handle per (device, stream, host thread); handles are independent of each other.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository root).
 */
#ifndef CSD_H_
#define CSD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum csd_status {
  CSD_OK = 0,
  CSD_ERR_INVALID = -1,      /* bad argument / unsupported configuration            */
  CSD_ERR_HIP = -2,          /* a HIP runtime call or kernel launch failed           */
  CSD_ERR_STATE = -3,        /* call sequence violated (e.g. forward before pack)    */
  CSD_ERR_NOT_FOUND = -4,    /* unknown parameter name                               */
  CSD_ERR_WORKSPACE = -5,    /* caller-supplied buffer too small                     */
  CSD_ERR_NONFINITE = -6     /* the sampler's state left the finite range (csd_pc_sample / csd_pc_step_end of the last step:
                                an fp16-operand mode met an operand beyond 65504 - run the network in CSD_PREC_F32)          */
} csd_status;

/* activation ids (models/layers.py:29-41 get_act) */
enum { CSD_ACT_NONE = 0, CSD_ACT_SWISH = 1, CSD_ACT_RELU = 2, CSD_ACT_LRELU = 3, CSD_ACT_ELU = 4 };

/* arithmetic of the convolution / 1x1 contractions */
enum {
  CSD_PREC_F32 = 0,          /* fp32 in, fp32 MFMA (v_mfma_f32_32x32x2_f32): exact fp32 fmaf chain */
  CSD_PREC_F16X3 = 1,        /* split-fp16 (hi+lo) operands, 3 fp16 MFMAs, fp32 accumulate        */
  CSD_PREC_F16 = 2,          /* fp16 operands, fp32 accumulate                                      */
  CSD_PREC_F16F8 = 3         /* split operands; hi*hi on the fp16 MFMA, the two correction products K-concatenated on the fp8 MFMA
                                (v_mfma_scale_f32_32x32x64_f8f6f4, e4m3 operands, block scale 2^-11) in the fused-prologue block
                                convolution; every other layer as CSD_PREC_F16X3.  Measured network error, full-size SR3-160 against the
                                reference: 1.3e-5 norm-wise / 4.5e-5 element-wise per evaluation (fp16x3: 1.9e-6 / 5.8e-6; fp16: 9e-4 / 3.9e-3) */
};

const char* csd_version(void);
const char* csd_last_error(void);

/* In-library profiler: while enabled, every kernel launch of csd_unet_forward / csd_pc_sample is
 * bracketed by HIP events on the stream the kernel runs on.  csd_profile_stop synchronises the last event
 * and returns, per launch class, total milliseconds, launch count, the algorithmic flops (2 * MACs) and the bytes
 * THE KERNEL has to move (its operand planes in, fp32 out, a residual read where it has one); csd_profile_stop_ex
 * also returns the ALGORITHMIC bytes of SURVEY.md 8(d): input + output tensor of the layer, fp32, nothing else. */
enum {
  CSD_PROF_CONV3X3 = 0,           /* 3x3 stride-1 convolutions on the mode's dominant kernel (fp16x3: conv_xk_kernel;
                                     a mode without a fused-prologue kernel: every 3x3 stride-1 convolution)             */
  CSD_PROF_CONV3X3_RESAMPLE = 1,  /* stride-2 / nearest-x2-fused 3x3 convolutions            */
  CSD_PROF_CONV1X1 = 2,           /* NIN / 1x1 contractions                                   */
  CSD_PROF_GN_STATS = 3,
  CSD_PROF_GN_FINAL = 4,
  CSD_PROF_ATTENTION = 5,
  CSD_PROF_SAMPLER = 6,           /* predictor / corrector updates (+ norms)                  */
  CSD_PROF_OTHER = 7,             /* input assembly, time embedding, dense layers             */
  CSD_PROF_GN_APPLY = 8,          /* GroupNorm+activation+fp16 split pass (fp16 conv modes)   */
  CSD_PROF_CONV3X3_OTHER = 9,     /* 3x3 stride-1 convolutions NOT on the dominant kernel: the first layer, the <= 20^2 levels */
  CSD_PROF_NUM_CLASSES = 10
};
/* Restrict the events to the launch classes whose bit (1u << CSD_PROF_*) is set and, inside csd_pc_sample, to every
 * step_stride-th PC step (defaults: all classes, every step).  An event pair costs ~5-15 us of stream time (the records
 * serialise back-to-back launches): ~5 ms per PC step with everything on - a timed region that only needs the dominant
 * kernel selects that class on a sample of the steps. */
int csd_profile_select(unsigned class_mask, int step_stride);
int csd_profile_start(void);
int csd_profile_stop(int n_classes, double* ms, int64_t* launches, double* flops, double* bytes);
int csd_profile_stop_ex(int n_classes, double* ms, int64_t* launches, double* flops, double* bytes, double* alg_bytes);

/* ------------------------------------------------------------------------------------------
 * Score network (U-Net) - replaces models/ddpm.py:80-213 (DDPM), :275-298 (DDPM_paired_SR3,
 * DDPM_paired) behind models/utils.py:27-47,114-120 (registry / create_model).
 * ---------------------------------------------------------------------------------------- */
#define CSD_MAX_LEVELS 8
#define CSD_MAX_ATTN 8
/* arch 0 (DDPM family): x_channels + y_channels and out_channels may each be up to this many (the 16-slice MRI -> PET slabs: 16 + 16 in,
 * 32 out; the Haar-band models: 12; the SR-flow Haar models: 9 + 3).  Above 8 input channels the assembled input is padded to the next
 * multiple of 16 with exact zeros.  arch 1 (NCSN++) takes the same widths with a condition (y_channels > 0;
 * out_channels == x_channels + y_channels; without one it keeps x_channels <= 8); its input pyramids read the padded assembled tensor, its output pyramid and head store up to 32 channels. */
#define CSD_MAX_IO_CHANNELS 32

typedef struct csd_unet_config {
  int32_t arch;                 /* 0 = DDPM family (models/ddpm.py); 1 = NCSN++ (models/ncsnpp.py); 2 = 3-D DDPM family
                                   (models/ddpm3D.py), see below */
  int32_t nf;                   /* config.model.nf                                           */
  int32_t n_levels;             /* len(config.model.ch_mult)                                 */
  int32_t ch_mult[CSD_MAX_LEVELS];
  int32_t num_res_blocks;
  int32_t n_attn;               /* len(config.model.attn_resolutions)                        */
  int32_t attn_resolutions[CSD_MAX_ATTN];
  int32_t image_size;           /* config.data.effective_image_size                          */
  int32_t x_channels;           /* channels of x (arch 0: x + y <= CSD_MAX_IO_CHANNELS)        */
  int32_t y_channels;           /* channels of the condition y (0: unconditional 'ddpm')     */
  int32_t out_channels;         /* config.model.output_channels (arch 0: <= CSD_MAX_IO_CHANNELS) */
  int32_t resamp_with_conv;
  int32_t conditional;          /* config.model.conditional (time embedding on/off)          */
  int32_t centered;             /* config.data.centered: 0 -> h = 2x-1 (models/ddpm.py:163-168)*/
  int32_t act;                  /* CSD_ACT_*                                                 */
  int32_t precision;            /* CSD_PREC_*                                                */
  /* ---- arch 1 (NCSN++, models/ncsnpp.py:44-236) only; resblock_type 'biggan', fir = True, combine 'sum' ---- */
  int32_t skip_rescale;         /* config.model.skip_rescale: (x + h)/sqrt(2)                */
  int32_t progressive;          /* 0 'none', 1 'output_skip'                                 */
  int32_t progressive_input;    /* 0 'none', 1 'input_skip', 2 'residual' with fir = True (Downsample Conv2d_0: FIR + VALID
                                   stride-2 conv), 3 'residual' with fir = False (Downsample Conv_0: pad (0,1,0,1) + stride-2 conv) */
  int32_t embedding_type;       /* 0 'positional', 1 'fourier' (W [nf] is parameter all_modules.0.W) */
  int32_t n_fir;                /* taps of config.model.fir_kernel (<= 8)                    */
  float fir_kernel[8];
  /* ---- arch 2 only: 1 = the handle serves the planned training graph (csd_unet_train_*, csd_unet_backward*, csd_unet_backward_marks*;
   * csrc/train_graph3d.h).  0 (a zero-initialised struct): those entries refuse the handle, naming 3-D, as they did before the graph
   * existed (csd_unet_train_workspace_bytes returns 0).  arch 0 / 1 always have their graph and ignore the field. ---- */
  int32_t planned_train;
  /* ---- arch 0 / 1: the direct Kx super-resolution networks (models/ddpm.py:316-331 ddpm_KxSR, models/ncsnpp.py:435-450 NCSNpp_KxSR).
   * K >= 2: y is the LOW-resolution image [B, y_channels, S / K, S / K] (S = image_size); the network sees its bilinear upsample to
   * S x S and returns its y channels downsampled to S / K.  Both resizes are torch's F.interpolate(mode = 'bilinear',
   * align_corners = False) WITHOUT antialiasing (what torchvision's Resize did on tensors when the reference was written).  The
   * library's boundary kernels compute the taps themselves: no full-resolution copy of y exists in inference.  See "y_scale" below.
   * 0 (a zero-initialised struct): y is [B, y_channels, S, S] as before.  The field stands in front of vol and x_squeeze, which stay the
   * struct's last two fields (tests/test_sr_host.py pins them there); like every field here it is read by name, never by position. ---- */
  int32_t y_scale;
  /* ---- arch 2 (3-D DDPM family, models/ddpm3D.py) only: the extents of the volume behind the channel, D, H, W (config.data.shape_x[1:]).
   * arch 2 ignores image_size, the attention fields and the arch-1 fields above; arch 0 / 1 ignore vol. ---- */
  int32_t vol[3];
  /* ---- arch 0, and arch 1 with y_channels > 0: the 2x super-resolution networks (models/ddpm.py:39-52,300-314, DDPM_2xSR; models/ncsnpp.py:403-432, NCSNpp_2xSR).  1: x is the HIGH-resolution image
   * [B, x_channels / 4, 2S, 2S] (S = image_size) and the network sees its space-to-depth squeeze,
   *     x'[b, 4c + 2dy + dx, i, j] = x[b, c, 2i + dy, 2j + dx],
   * so x_channels stays the count the NETWORK sees (a multiple of 4).  The library's boundary kernels address the image directly: no
   * squeezed copy of x exists.  See "x_squeeze" below.  0 (a zero-initialised struct): x is [B, x_channels, S, S] as before. ---- */
  int32_t x_squeeze;
} csd_unet_config;
/* sizeof(csd_unet_config) of the library at hand.  The struct grows with the library (y_scale was inserted in front of vol and
 * x_squeeze, so their offsets moved): a caller compiled against an older header must be recompiled, and can tell by comparing this
 * with its own sizeof before the first csd_unet_create (the Python binding does, conditional_score_diffusion_amd/_lib.py). */
size_t csd_unet_config_size(void);

/* y_scale = K >= 2 (arch 0 / 1; csd_unet_create returns CSD_ERR_INVALID, naming the field, for arch 2, together with x_squeeze, for
 * y_channels == 0, image_size % K != 0, x_channels + y_channels > 8 and out_channels < x_channels).  With s = S / K:
 *   y, y_noise (csd_unet_forward, csd_unet_train_forward, csd_pc_sample / csd_pc_step_begin / _end, the use_path bridge)
 *                                                                              [B, y_channels, s, s]
 *   the perturbation y + y_sigma y_noise / y + std_y z happens at s x s, then the upsample; a y draw of the sampler has this size
 *   out, d_out: per sample x_channels * S * S floats - the x block [x_channels, S, S] - then (out_channels - x_channels) * s * s
 *   floats, the other channels downsampled: the mean of the 2 x 2 block at rows / columns K i + K / 2 - 1, K i + K / 2 (K even) or the
 *   pixel K i + (K - 1) / 2 (K odd), which is what the bilinear formula gives for an integer K
 *   x, d_x, the sampler's state, its noise and every `record` row               [B, x_channels, S, S] as before
 * csd_unet_workspace_bytes grows by one [B, out_channels, S, S] tensor (the head's output before the downsample).
 * csd_pc_inpaint_* and csd_unet_debug_digest return CSD_ERR_INVALID for such a handle. */

/* x_squeeze = 1 (arch 0; csd_unet_create refuses it for arch 1 / 2 and refuses x_channels % 4 != 0, out_channels < x_channels and
 * image_size > 1024, naming the field).  With
 * Ci = x_channels / 4 and HW = S * S, every per-sample element count is unchanged (x_channels * HW), only the layout of the x block is
 * the image's:
 *   x (csd_unet_forward, csd_unet_train_forward), d_x (csd_unet_backward_ex), the state x and every `record` row of csd_pc_sample /
 *   csd_pc_step_begin / csd_pc_step_end                                       [B, Ci, 2S, 2S]
 *   out, d_out: per sample out_channels * HW floats - first the x block as the image [Ci, 2S, 2S] (x_channels * HW floats), then
 *   the remaining out_channels - x_channels channels as [., S, S]; needs out_channels >= x_channels
 *   y, y_noise                                                                 [B, y_channels, S, S] as before
 * csd_pc_inpaint_* and csd_unet_debug_digest return CSD_ERR_INVALID for a squeezed handle. */

/* arch 2: x [B, x_channels, D, H, W], y [B, y_channels, D, H, W] (NULL iff y_channels == 0; ddpm3D has none, the paired classes take
 * both counts from shape_x[0] / shape_y[0]), out [B, out_channels, D, H, W], all NCDHW.  The handle serves csd_unet_create / destroy,
 * num_params / param_info / set_param, packed_bytes / pack / workspace_bytes, forward / stats and csd_pc_scratch_bytes / csd_pc_sample /
 * csd_pc_step_begin / csd_pc_step_end with unchanged signatures: csd_unet_pack runs csd_conv3d_block's weight pack once per layer,
 * csd_unet_forward is the layer list of DDPM3D.forward on the kernels of csd_conv3d_block / csd_groupnorm_scale_shift /
 * csd_avgpool3d_2_ndhwc / csd_nearest_up2_3d_ndhwc at fixed workspace offsets (bitwise what the per-operator calls give, repeatable,
 * independent of the batch position).  csd_unet_create refuses, with the reason: resamp_with_conv, conditional = 0, nf % 32 != 0, an
 * extent that is odd or below 2 at a pooled level, a precision other than CSD_PREC_F32 / CSD_PREC_F16X3, and a ch_mult for which an up
 * block's concatenated input is as wide as its output (that block has no Conv_2).  The training entries (csd_unet_train_*,
 * csd_unet_backward*, csd_unet_backward_marks*) serve an arch-2 handle created with planned_train = 1 (below); without it they return
 * CSD_ERR_INVALID (csd_unet_train_workspace_bytes returns 0) with a message that names 3-D.  csd_pc_inpaint_* and csd_unet_debug_digest
 * return CSD_ERR_INVALID for every arch-2 handle with a message that names 3-D; the probability-flow entries (csd_pf_ode_*) take no handle, and
 * their Python caller refuses the 3-D networks. */

typedef struct csd_unet csd_unet;

int csd_unet_create(const csd_unet_config* cfg, csd_unet** out);
void csd_unet_destroy(csd_unet* net);

/* Parameter table, in reference state_dict order/naming ("all_modules.3.Conv_0.weight", ...).
 * Layouts are the reference's: conv OIHW, NIN.W [in,out], Linear [out,in].  arch 0 / 1: `shape` receives 4 entries.  arch 2: the
 * convolution weights are [Cout, Cin, 3, 3, 3] (ndim 5) and `shape` must hold 5 entries (all 5 are written for every parameter). */
int csd_unet_num_params(const csd_unet* net);
int csd_unet_param_info(const csd_unet* net, int index, const char** name, int* ndim, int64_t shape[]);
/* Register the device address of one parameter (fp32, contiguous, reference layout). */
int csd_unet_set_param(csd_unet* net, const char* name, const void* dev_ptr, int64_t numel);

/* Repack every registered parameter into the library's MFMA-fragment layout.  `packed` is a
 * caller-owned device buffer of csd_unet_packed_bytes(); must be re-run after weights change. */
size_t csd_unet_packed_bytes(const csd_unet* net);
int csd_unet_pack(csd_unet* net, void* packed, void* stream);

/* Activation workspace needed for batch size B. */
size_t csd_unet_workspace_bytes(csd_unet* net, int B);

/* One network evaluation = model(x | {'x','y'}, labels) of models/utils.py:134-150 in eval mode.
 *   x      [B, x_channels, S, S]   y [B, y_channels, S, S] (NULL iff y_channels == 0)
 *   labels [B]                     out [B, out_channels, S, S]          (arch 2: D, H, W in place of S, S)
 *   y_noise/y_sigma: optional fused perturbation y_t = y + y_sigma * y_noise
 *                    (sampling/conditional.py:104-110); pass NULL / 0 to use y as is. */
int csd_unet_forward(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes,
                     const float* x, const float* y, const float* labels, float* out, int B,
                     const float* y_noise, float y_sigma, void* stream);

/* number of kernel launches / algorithmic flops+bytes of one forward at batch B (for bench) */
int csd_unet_stats(csd_unet* net, int B, int64_t* launches, double* flops, double* bytes);

/* ------------------------------------------------------------------------------------------
 * Fused predictor-corrector sampler - replaces the loop of sampling/conditional.py:180-226 and
 * sampling/unconditional.py:194-226 for the registered predictors and correctors on a single VE, VP or sub-VP SDE and on
 * the two-SDE VE pair (sampling/predictors.py:52-200, sampling/correctors.py:51-163, sde_lib.py:49-63,186-195,353-362,410-418).
 * A zero-initialised struct with the first block of fields set is the (reverse_diffusion, langevin) VE pair.
 * Per-step scalars are computed by the host mirror in fp32 exactly as the reference does and
 * handed over as arrays of length n_steps.
 * ---------------------------------------------------------------------------------------- */
typedef struct csd_pc_params {
  int32_t n_steps;              /* p_steps                                                   */
  const float* labels;          /* [n_steps] network label for step i (t*(N-1) or sigma(t))  */
  const float* std_x;           /* [n_steps] sigma_x(t): score = net / std_x                 */
  const float* G;               /* [n_steps] reverse-diffusion G_i                            */
  const float* std_y;           /* [n_steps] sigma_y(t) or NULL (SR3 / unconditional)        */
  float snr;                    /* Langevin target snr                                       */
  int32_t denoise;              /* return x_mean of the last predictor step                  */
  /* noise source: a tape (parity mode) or on-device Philox (throughput mode) */
  const float* noise_tape;      /* draws in reference order, or NULL         */
  uint64_t seed;                /* Philox key when noise_tape == NULL                        */
  float* record;                /* optional [n_steps, B, C, S, S]: x after every step, or NULL*/
  /* the other registered update rules on the same device loop (zero-initialised = the pair above).  They are all affine in
   * (x, score, z) with per-step host scalars: x_mean = p*x + a*score, x = x_mean + b*z  (sampling/predictors.py:52-76 Euler-
   * Maruyama, :105-135 ancestral sampling; sampling/correctors.py:111-142 annealed Langevin dynamics). */
  int32_t predictor;            /* 0 reverse diffusion (G); 1 affine table pred_coef; 2 none (no evaluation, no draw) */
  int32_t corrector;            /* 0 Langevin (snr, batch-mean norms); 1 affine table corr_coef; 2 none               */
  const float* pred_coef;       /* [n_steps][3] = (p, a, b) when predictor == 1                                      */
  const float* corr_coef;       /* [n_steps][3] when corrector == 1                                                  */
  /* `use_path` of the two-SDE samplers (sampling/conditional.py:85-100,124-178; sde_lib.py:323-339): y_t is not redrawn from the
   * marginal for every evaluation but follows the bridge p(y_t | y_0, y_{t+tau}): once per step y_t = w0*y + w1*y_{t+tau} + s*z,
   * the PREDICTOR runs first, then the corrector, both on that y_t.  path_coef != NULL selects it (std_y must be NULL);
   * y_{T+tau} = y + path_std0 * z (the draw z_y0 of csd_pc_noise_draws). */
  const float* path_coef;       /* [n_steps][3] = (w0, w1, s), or NULL                                                */
  float path_std0;              /* sigma_y(T + tau)                                                                    */
  /* Langevin corrector of the VP / subVP SDEs (sampling/correctors.py:63-65,94-96): step size times alphas[timestep_i]     */
  const float* corr_alpha;      /* [n_steps] or NULL (= 1: the VE SDEs)                                                */
  /* predictor == 0 on an SDE with a forward drift, or as the probability flow (sde_lib.py:65-102): f = (a*x)*b, minus x when
   * rd_sub_x (VP discretize, :186-195: a = sqrt(alpha_i), b = 1; the Euler default sub-VP inherits, :49-63: a = phi(t), b = dt);
   * rev_f = f - G^2*score*kappa, x_mean = x - rev_f, x = x_mean + G_noise*z.  All three zero = the VE update above, same kernel. */
  const float* rd_drift;        /* [n_steps][2] = (a, b), or NULL (f = 0: the VE SDEs)                                 */
  int32_t rd_sub_x;             /* 1: f = (a*x)*b - x; needs rd_drift                                                  */
  int32_t probability_flow;     /* 1: kappa = 1/2 and G_noise = 0 (the draw is still consumed); 0: kappa = 1, G_noise = G */
} csd_pc_params;

/* x: [B, x_channels, S, S] in: prior sample (VE: already scaled by sigma_max); out: result.
 * y: [B, y_channels, S, S] or NULL.  scratch: csd_pc_scratch_bytes() device bytes, 256-byte aligned: net_out [B, out_channels, HW] |
 * x_mean, z [B, x_channels, HW] each | zy [B, max(y_channels, 1), HW] | labels [B] | y_t, the same size as zy, in 64-float granules,
 * then the norm partials [B, 64, 2] doubles and 256 bytes for the finiteness flag (pc_scratch in csrc/pc_loop.h is the one description;
 * a y_scale handle gets the same full-resolution regions).  An arch-2 handle runs the same loop on volumes
 * ([.., D, H, W] in place of [.., S, S]): same update kernels, noise draws and contract.
 * Finiteness contract: the Langevin corrector's norms (which see every element of the score and of the noise) and one pass over the
 * returned state set a device flag; csd_pc_sample reads it back behind the stream before it returns - its ONE synchronisation - and
 * fails with CSD_ERR_NONFINITE rather than hand back NaN images (csd_pc_step_end does the same after the last step). */
size_t csd_pc_scratch_bytes(const csd_unet* net, int B);
int csd_pc_sample(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes,
                  void* scratch, size_t scratch_bytes, float* x, const float* y, int B,
                  const csd_pc_params* p, void* stream);
/* The noise draws of the loop.  ONE rule: the draws behind the prior form one sequence in the order the loop consumes them; draw j
 * of it is Philox stream 1 + j of p->seed (stream 0 is the caller's prior) and lies on p->noise_tape behind the draws before it.  An x
 * draw (z, z_blend) has the state's size, a y draw (z_y0, z_y, zy) that of y (at S / K for a y_scale handle).  A phase whose rule is
 * `none` has no zy / z; a probability-flow predictor still consumes its z.  Per step, by mode:
 *   plain                  [z corrector] [z predictor]
 *   std_y                  [zy z corrector] [zy z predictor]        (zy: the y_t of that phase's evaluation)
 *   path_coef (use_path)   z_y0 in front of the loop | z_y of the bridge, [z predictor], [z corrector]
 *   inpainting             [z corrector] z_blend [z predictor] z_blend       (a `none` phase draws its z_blend)
 *   colorization           [z corrector] z_colorize [z predictor] z_colorize (the same places; only channel 0 of the draw is used)
 * csd_pc_noise_draws lists them for a handle, a batch size and the fields of csd_pc_params the schedule depends on (has_std_y,
 * has_path_coef: the pointer is given; inpaint: 1 = a csd_pc_inpaint_* call, 2 = a csd_pc_colorize_* call).  It returns the number of
 * draws behind the prior and fills up to `cap` rows of 6: {step (-1: in front of the loop), kind (0 z_y0, 1 z_y, 2 zy, 3 z, 4 z_blend,
 * 5 z_colorize), phase (0 corrector, 1 predictor, 2 none), elements, tape offset in floats, Philox stream}.  It needs no GPU.  It
 * refuses, with CSD_ERR_INVALID and the message of the sampling entries (which make the same check): both rules `none`; std_y or
 * path_coef with y_channels == 0; std_y and path_coef together; inpainting or colorization with y_channels > 0, std_y, path_coef,
 * x_squeeze, y_scale or an arch-2 handle; colorization with x_channels != 3. */
int64_t csd_pc_noise_draws(const csd_unet* net, int B, int predictor, int corrector, int has_std_y, int has_path_coef, int inpaint,
                           int n_steps, int64_t* rows, int cap);
/* The same loop one PC step at a time, for the GLOBAL-NORM exactness mode of batch-sharded sampling (identical to
 * ONE reference process holding the global batch; the Langevin step size uses batch-mean norms, sampling/correctors.py:100-106).
 *   csd_pc_step_begin(step): corrector network evaluation + its noise draw; norm_sums[0] = sum_b ||score_b||_2 and
 *                            norm_sums[1] = sum_b ||z_b||_2 over THIS rank's B samples (two fp32 on the device).
 *   -- the caller all-reduces (SUM) the two floats over the ranks: one 8-byte RCCL collective, no host synchronisation --
 *   csd_pc_step_end(step):   Langevin update with gbar = norm_sums[0] / global_batch, nbar = norm_sums[1] / global_batch,
 *                            then the predictor half of the step; after the last step x holds x_mean when p->denoise.
 * Same params / scratch / noise order as csd_pc_sample (with global_batch == B and no all-reduce the two calls per step
 * reproduce it); p->record is honoured. */
int csd_pc_step_begin(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                      size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p, int step,
                      float* norm_sums, void* stream);
int csd_pc_step_end(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                    size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p, int step,
                    const float* norm_sums, int global_batch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Inpainting with an unconditional network on the same device loop (sampling/unconditional.py:230-345): after the update of
 * EVERY phase - a phase whose rule is `none` included, the reference wraps every update function - the known pixels are re-imposed
 * at the step's noise level (:268-271), in fp32 and in this order:
 *     masked_mean = mean_scale[i]*data ; masked = masked_mean + std[i]*z ;
 *     x = x*(1 - mask) + masked*mask ; x_mean = x*(1 - mask) + masked_mean*mask        (x_mean from the NEW x)
 * x (in): the initial state prior*(1 - mask) + data*mask.  mask is 1 on known pixels; any value in [0, 1] is blended as written.
 * Unconditional networks only: y_channels > 0, std_y or path_coef are refused with CSD_ERR_INVALID.
 * The draws are those of the step-by-step inpainter's randn_like calls (csd_pc_noise_draws above lists them); the blend makes its
 * normals in registers, bit-identical to a csd_randn fill of the draw's stream id.
 * denoise returns the re-imposed x_mean of the last predictor phase; record, the finiteness contract and the single final
 * synchronisation are those of the loop above, and the two step calls with global_batch == B and no all-reduce reproduce the one
 * call.  The entry points without an inpainting struct keep their noise numbering and results bit for bit.
 * ---------------------------------------------------------------------------------------- */
typedef struct csd_pc_inpaint_params {
  const float* data;            /* device [B, x_channels, S, S]: the image whose known pixels are imposed             */
  const float* mask;            /* device, same shape: 1 = known pixel                                                */
  const float* mean_scale;      /* host [n_steps]: mean of p_t(x | data) = mean_scale * data (1 for the VE SDEs)      */
  const float* std;             /* host [n_steps]: std of p_t(x | data), the SDE's marginal std                       */
} csd_pc_inpaint_params;

size_t csd_pc_inpaint_scratch_bytes(const csd_unet* net, int B);
int csd_pc_inpaint_sample(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                          size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                          const csd_pc_inpaint_params* ip, void* stream);
int csd_pc_inpaint_step_begin(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                              size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                              const csd_pc_inpaint_params* ip, int step, float* norm_sums, void* stream);
int csd_pc_inpaint_step_end(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                            size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                            const csd_pc_inpaint_params* ip, int step, const float* norm_sums, int global_batch, void* stream);
/* The re-imposition alone, in place on x over n elements (x_mean may be NULL).  z: the normals to use, or NULL: Philox4x32-10 +
 * Box-Muller of (seed, stream_id) in registers - element e is lane e % 4 of counter e / 4, exactly the fill of the randn operator
 * below - and nothing is drawn when std == 0.  16-byte loads and stores when every pointer is 16-byte aligned. */
int csd_inpaint_blend(float* x, float* x_mean, const float* data, const float* mask, const float* z, float mean_scale,
                      float std, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Colorization with an unconditional 3-channel network on the same device loop (controllable_generation.py:95-191 of the reference).
 * The constraint lives in a rotated channel space: decouple(v)[b, j] = sum_i v[b, i] * M[i][j] with a fixed orthonormal 3 x 3 M,
 * couple the same contraction with M^-1; channel 0 of the decoupled space is the gray channel.  After the update of EVERY phase (a
 * `none` phase included), in fp32, every contraction summed as (v0*A0j + v1*A1j) + v2*A2j:
 *     masked_mean = mean_scale[i]*gray0 ; masked = masked_mean + z0*std[i]          (gray0 = decouple(gray)[:, 0], z0 = z[:, 0])
 *     x = couple(masked, decouple(x)[1], decouple(x)[2]) ; x_mean = couple(masked_mean, decouple(x)[1], decouple(x)[2]) with the NEW x
 * x (in): the initial state couple(decouple(gray)*mask + decouple(prior*(1 - mask))), mask = 1 on channel 0 - the prior is masked in
 * IMAGE space (the reference's order): csd_colorize_blend with init = 1 makes it from the prior.
 * Draws: one x draw (kind 5, z_colorize) behind every phase, where inpainting has its z_blend - a full-size draw like the reference's
 * randn_like, of which only the channel-0 plane is read; without a tape the blend makes exactly those elements of the draw's Philox
 * stream in registers.  csd_pc_noise_draws lists the schedule with inpaint = 2.
 * matrix / inv_matrix: HOST 3 x 3 row-major, NULL = the reference's M / the float64 inverse of matrix rounded once to fp32.  Refused
 * with CSD_ERR_INVALID: max |M M^T - I| > 1e-6, an inv_matrix with max |M inv - I| > 1e-6, and - before any buffer is touched - an
 * arch-2 handle, x_squeeze, y_scale, y_channels > 0, x_channels != 3, std_y and path_coef.
 * scratch: csd_pc_scratch_bytes of the handle (the blend needs no buffer; the name below is an alias, not a second sizing entry).
 * denoise, record, the finiteness contract, the single synchronisation and the two step calls are those of csd_pc_inpaint_*.
 * ---------------------------------------------------------------------------------------- */
typedef struct csd_pc_colorize_params {
  const float* gray0;           /* device [B, 1, S, S]: channel 0 of decouple(gray), csd_colorize_gray0                */
  const float* mean_scale;      /* host [n_steps]: mean of p_t(x | data) = mean_scale * data (1 for the VE SDEs)      */
  const float* std;             /* host [n_steps]: the SDE's marginal std                                             */
  const float* matrix;          /* host 3 x 3 M or NULL                                                               */
  const float* inv_matrix;      /* host 3 x 3 M^-1 or NULL                                                            */
} csd_pc_colorize_params;

#define csd_pc_colorize_scratch_bytes csd_pc_scratch_bytes
int csd_pc_colorize_sample(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                           size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                           const csd_pc_colorize_params* cp, void* stream);
int csd_pc_colorize_step_begin(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                               size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                               const csd_pc_colorize_params* cp, int step, float* norm_sums, void* stream);
int csd_pc_colorize_step_end(csd_unet* net, const void* packed, void* workspace, size_t workspace_bytes, void* scratch,
                             size_t scratch_bytes, float* x, const float* y, int B, const csd_pc_params* p,
                             const csd_pc_colorize_params* cp, int step, const float* norm_sums, int global_batch, void* stream);
/* The re-imposition alone, in place on x [B, 3, hw] (x_mean may be NULL).  z: a tensor of x's size whose channel-0 plane holds the
 * normals, or NULL: those elements of the randn fill of (seed, stream_id) in registers; nothing is drawn when std == 0.  init = 1: x
 * holds the prior and becomes the initial state (mean_scale = 1; z, std and x_mean are not used).  16-byte loads and stores when every
 * pointer is 16-byte aligned and hw is a multiple of 4, element-wise otherwise.  No atomics: bitwise repeatable. */
int csd_colorize_blend(float* x, float* x_mean, const float* gray0, const float* z, float mean_scale, float std, int B, int64_t hw,
                       int init, const float* matrix, const float* inv_matrix, uint64_t seed, uint64_t stream_id, void* stream);
/* gray0 [B, 1, hw] = channel 0 of decouple(gray [B, 3, hw]): once per sampler call */
int csd_colorize_gray0(const float* gray, float* gray0, int B, int64_t hw, const float* matrix, void* stream);

/* ------------------------------------------------------------------------------------------
 * Band split / merge (csrc/band.hip): the 2x2-block, stride-2 orthogonal transform of the Haar multi-scale models, per image channel,
 * NCHW fp32 - what the reference does with iunets.layers.InvertibleDownsampling2D(init='haar') followed by permute_channels
 * (lightning_modules/HaarMultiScaleSdeGenerativeModel.py:15-39, ConditionalSdeGenerativeModel.py:207-247).  With a_dydx = x[b, c, 2i+dy, 2j+dx]:
 *   csd_band_split: x [B, C, 2S, 2S] -> bands [B, 4C, S, S], band-major: bands[b, C*k + c, i, j] = sum_{dy,dx} M[k][2dy+dx] * a_dydx
 *   csd_band_merge: the transpose; lo [B, C, S, S] (band 0) and hi [B, 3C, S, S] (bands 1 - 3) through two pointers (no cat) ->
 *                   x[b, c, 2i+dy, 2j+dx] = sum_k M[k][2dy+dx] * band_k[b, c, i, j]
 * matrix: HOST 4 x 4 row-major M, or NULL = the orthonormal Haar matrix
 *   b0 = (a00 + a01 + a10 + a11) / 2    b1 = (a00 - a01 + a10 - a11) / 2    b2 = (a00 + a01 - a10 - a11) / 2    b3 = (a00 - a01 - a10 + a11) / 2
 * A matrix with max |M M^T - I| > 1e-6 is refused (CSD_ERR_INVALID, the message gives the figure).  The matrix is an argument because
 * the ORDER AND SIGNS OF BANDS 1 - 3 of the reference's layer could not be checked: iunets was not available when this was written.
 * Band 0 (the low band, all +1/2) is fixed by init='haar'; a caller who has that library passes its 4 x 4 kernel here.
 * x_ld, bands_ld, lo_ld, hi_ld: floats between consecutive samples of that tensor (>= its dense per-sample size), so the merge can write
 * the first C channels of a wider [B, 4C, 2S, 2S] buffer and either call can address a channel slice.  S >= 1 is the side of the bands
 * (the image side 2S is even by construction; the Python operators refuse an odd image side).  Every output element is a fixed-order
 * four-term fp32 fma chain: bitwise repeatable.  8-byte accesses on the image, coalesced 4-byte accesses on the bands; 16-byte accesses on
 * both when S % 4 == 0 and every pointer is 16-byte aligned and every stride a multiple of 4 (else: the image pointer 8-byte aligned and
 * x_ld even are REQUIRED).  No LDS, no scratch. */
int csd_band_split(const float* x, int64_t x_ld, float* bands, int64_t bands_ld, int B, int C, int S, const float* matrix, void* stream);
int csd_band_merge(const float* lo, int64_t lo_ld, const float* hi, int64_t hi_ld, float* x, int64_t x_ld, int B, int C, int S,
                   const float* matrix, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sequential super-resolution cascades (run_lib.py:113-222 multi_scale_test: bicubic_autoregressive_sampler,
 * haar_autoregressive_sampler; the inpainting form of lightning_modules/HaarMultiScaleSdeGenerativeModel.py:62-89): n_stages fused PC
 * loops enqueued back to back on one stream, each stage's condition made on the device from the stage before, ONE synchronisation
 * behind the last stage.  A stage is what csd_pc_sample (inpaint == NULL) or csd_pc_inpaint_sample (inpaint != NULL) takes:
 *   x: in = the caller's prior for this stage (an inpainting stage 0: already blended with its data), out = the stage's result.
 *   link (stage k >= 1; stage 0 takes the call's y0 - NULL iff it has no condition - and must have link 0):
 *     0  bicubic: the previous stage's x IS this stage's y (the pointer is handed over, no copy).  Previous x_channels / 4 (a 2x
 *        network, x_squeeze) or x_channels image channels at side 2S or S must be this stage's y_channels at its side.
 *     1  Haar, conditional: y = csd_band_merge(previous y, previous x).  Previous y_channels = C, x_channels = 3C at side S; this stage
 *        y_channels = C at side 2S.  The merged image is written to the PREVIOUS stage's `out`, or, out == NULL, to a region of the scratch.
 *     2  Haar, inpainting (both stages have inpaint): this stage's inpaint->data buffer [B, 4C, 2S, 2S] - which the stage owns; the
 *        library writes it - is zeroed, csd_band_merge(previous data[:, :C], previous x[:, C:]) is written into its first C channels,
 *        and the state is started as x = x * (1 - mask) + data * mask (csd_inpaint_blend with std = 0).  Previous x_channels = 4C at
 *        side S; this stage x_channels = 4C at side 2S.  The previous stage's `out` must be NULL.
 *   final_link: what becomes of the LAST stage's result: 0 nothing (x is the result); 1 / 2: the last stage's `out` (required)
 *     [B, C, 2S, 2S] = the merge of link 1 / 2 applied to the last stage.
 *   band_matrix: csd_band_merge's matrix for every link (host, NULL = Haar).
 * Buffers, shared by the stages one after the other (results do not depend on what they held):
 *   workspace_bytes >= max over stages of csd_unet_workspace_bytes(net, B)
 *   scratch_bytes   >= max over stages of csd_pc_scratch_bytes(net, B), rounded up to 256, + for every stage that is followed by a
 *                      link-1 stage and has out == NULL: B * C * 2S * 2S * 4 bytes rounded up to 256      (scratch 256-byte aligned)
 * A short buffer is CSD_ERR_WORKSPACE naming the stage that needs more.
 * stage_flags: device int32_t [n_stages], written by the call: stage k's flag of the finiteness contract of csd_pc_sample.  The call
 * reads them back behind the last stage - its one synchronisation - and fails with CSD_ERR_NONFINITE naming the FIRST stage whose flag
 * is set (the later stages then ran on garbage: wasted work, nothing else).
 * Refused with CSD_ERR_INVALID naming the stage: extents that do not match at a link, 3-D handles, handles with y_scale, a
 * conditional stage with inpaint or an unconditional one without, a NULL handle / packed / pc / x; B < 1 and a NULL stage_flags are
 * refused too.  pc->record is honoured.  Each stage keeps the noise numbering and the bits of its single-stage entry.
 * ---------------------------------------------------------------------------------------- */
typedef struct csd_cascade_stage {
  csd_unet* net;
  const void* packed;                    /* the handle's packed weights (csd_unet_pack)                                    */
  const csd_pc_params* pc;
  const csd_pc_inpaint_params* inpaint;  /* NULL: a conditional stage; else an inpainting stage (link 2 writes inpaint->data) */
  float* x;                              /* the stage's state: prior in, result out                                        */
  int32_t link;                          /* 0, 1, 2: how this stage's condition comes from the stage before (see above)    */
  float* out;                            /* the image this stage hands on through a merge, or NULL                         */
} csd_cascade_stage;
int csd_pc_cascade_sample(const csd_cascade_stage* stages, int n_stages, int final_link, const float* y0, int B, void* workspace,
                          size_t workspace_bytes, void* scratch, size_t scratch_bytes, int32_t* stage_flags, const float* band_matrix,
                          void* stream);

/* Stand-alone update kernels (the "noise-add" steps), usable with any score source:
 *   csd_langevin_step: sampling/correctors.py:51-78,88-108: step = (snr * mean||z|| / mean||score||)^2 * 2 * alpha with
 *                      alpha = sde.alphas[timestep] for the VP / subVP SDEs (:63-65,94-96) and 1 for the VE SDEs
 *   csd_reverse_diffusion_step: sampling/predictors.py:84-89,97-102 with f = 0
 *   csd_reverse_diffusion_step_ex: the same lines for every SDE and for the probability flow: drift_form 0: f = 0; 1: f =
 *                      (drift_a*x)*drift_b (Euler default, sub-VP); 2: that minus x (VP discretize); rev_f = f - G^2*score*kappa,
 *                      x_mean = x - rev_f, x = x_mean + g_noise*z (reverse SDE: kappa = 1, g_noise = G; flow: 1/2 and 0)
 * net: raw network output; score = net / std.  x is updated in place, x_mean written.
 * scratch: >= csd_update_scratch_bytes(B) bytes. */
size_t csd_update_scratch_bytes(int B);
int csd_langevin_step(float* x, float* x_mean, const float* net, const float* z, float std,
                      float snr, float alpha, int B, int64_t per_sample, void* scratch, void* stream);
int csd_reverse_diffusion_step(float* x, float* x_mean, const float* net, const float* z, float std,
                               float G, int B, int64_t per_sample, void* stream);
int csd_reverse_diffusion_step_ex(float* x, float* x_mean, const float* net, const float* z, float std, float G,
                                  float drift_a, float drift_b, int drift_form, float kappa, float g_noise, int B,
                                  int64_t per_sample, void* stream);
/* General one-step update  x_mean = p*x + a*score,  x = x_mean + c*z  (n elements, scalars per call): the
 * Euler-Maruyama and ancestral-sampling predictors (sampling/predictors.py:52-76,105-179) and the annealed
 * Langevin corrector (sampling/correctors.py:111-142); `score` is the score itself (already divided by std). */
int csd_affine_noise_step(float* x, float* x_mean, const float* score, const float* z, float p, float a,
                          float c, int64_t n, void* stream);
/* out[b] = ||a_b||_2 over per_sample elements (fp64 accumulation): the per-sample norms behind the Langevin step size
 * (sampling/correctors.py:102-103), for the global-batch exactness mode that all-reduces them across ranks */
int csd_row_norms(const float* a, float* out, int B, int64_t per_sample, void* stream);
/* standard-normal fill (Philox4x32-10 + Box-Muller); counter-based: (seed, stream_id) */
int csd_randn(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);
/* out[b,:] = in[b,:] * scale[b]  or / scale[b] (divide_by_sigmas, models/utils.py:50-74) */
int csd_scale_rows(float* out, const float* in, const float* scale, int divide, int B,
                   int64_t per_sample, void* stream);

/* ------------------------------------------------------------------------------------------
 * Individual operators (NCHW fp32 boundary) - the kernels the network is built from, exported
 * for per-op parity tests and for callers that use the reference's functional ops directly.
 * ---------------------------------------------------------------------------------------- */
/* y = act(GroupNorm(x; G groups, eps) * gamma + beta)  - nn.GroupNorm + get_act
 * (models/layers.py:571,638,646).  scratch: csd_groupnorm_scratch_bytes(B, C, H, W).  The size queries of GroupNorm (this one and
 * csd_groupnorm_nhwc_scratch_bytes) do not take `groups`: they cover up to CSD_GN_SCRATCH_MAX_GROUPS groups, and csd_groupnorm_act /
 * csd_groupnorm_act_nhwc return CSD_ERR_INVALID for more. */
#define CSD_GN_SCRATCH_MAX_GROUPS 64
size_t csd_groupnorm_scratch_bytes(int B, int C, int H, int W);
int csd_groupnorm_act(const float* x, const float* gamma, const float* beta, float* y, int B, int C,
                      int H, int W, int groups, float eps, int act, void* scratch, void* stream);

/* 3x3 / 1x1 convolution (models/layers.py:100-132 ddpm_conv1x1/ddpm_conv3x3; NIN :555-564 via
 * ksize=1).  weight OIHW, stride in {1,2}; pad_mode 0: symmetric pad (ksize/2); 1: the
 * reference Downsample's (0,1,0,1) pad + stride 2 (models/layers.py:619-625); up2: nearest x2
 * upsample of x first (models/layers.py:600-604).  scratch: csd_conv_scratch_bytes(). */
size_t csd_conv_scratch_bytes(int B, int Cin, int Cout, int H, int W, int ksize, int up2);
int csd_conv2d(const float* x, const float* weight, const float* bias, float* y, int B, int Cin,
               int Cout, int H, int W, int ksize, int stride, int pad_mode, int up2, int precision,
               void* scratch, void* stream);

/* single-head self-attention core of AttnBlock (models/layers.py:584-588):
 * q,k,v,out [B, C, H, W]; w = softmax(q.k * C^-1/2) over keys; out = w.v */
size_t csd_attention_scratch_bytes(int B, int C, int H, int W);
int csd_attention(const float* q, const float* k, const float* v, float* out, int B, int C, int H,
                  int W, void* scratch, void* stream);

/* upfirdn2d (op/upfirdn2d.py:147-158, op/upfirdn2d_kernel.cu:107-207): x [N, C, H, W],
 * kernel [kh, kw]; out [N, C, (H*up+pad0+pad1-kh)/down+1, ...]. */
int csd_upfirdn2d(const float* x, const float* kernel, float* out, int N, int C, int H, int W, int kh,
                  int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0,
                  int pad_y1, void* stream);
/* fused_bias_act (op/fused_bias_act_kernel.cu:18-49): out = lrelu(x + b[c], alpha) * scale,
 * act: 1 linear, 3 lrelu; grad 0 forward, 1 backward w.r.t. x using `ref` = forward output. */
/* NCSN++ residual input pyramid (layerspp.Downsample(with_conv=True), layerspp.py:129-163; fir_pyramid.hip):
 *   out = (Downsample(x) + res) * out_scale     (res == NULL: Downsample(x) * out_scale)
 * x NHWC [B, H, H, Cin] with x_pixel_stride (>= Cin) floats per pixel; w [Cout, Cin, 3, 3] OIHW, bias [Cout] (may be NULL);
 * res / out NHWC [B, H/2, H/2, Cout].  fir_kernel (host, 4 taps): conv_downsample_2d = upfirdn2d with the normalised FIR, pads
 * (2, 2), then a VALID stride-2 conv (up_or_down_sampling.py:144-178); fir_kernel == NULL: F.pad(0,1,0,1) + stride-2 conv (fir = False).
 * Computed as one 6x6 stride-2 convolution with the FIR folded into the weight (fp64 fold), fp32 arithmetic, deterministic.
 * scratch: csd_fir_pyr_conv_scratch_bytes(Cin, Cout). */
size_t csd_fir_pyr_conv_scratch_bytes(int Cin, int Cout);
int csd_fir_pyr_conv(const float* x, const float* w, const float* bias, const float* res, float* out, int B, int Cin, int Cout, int H,
                     int x_pixel_stride, const float* fir_kernel, float out_scale, void* scratch, void* stream);
/* FIR resampling by 2 of an NHWC tensor with a separable 4-tap kernel (host pointer): upsample_2d / downsample_2d of
 * models/up_or_down_sampling.py:196-257, as the NCSN++ plans run it on their pyramids and BigGAN blocks.  x [B, H, W, C] ->
 * out [B, 2H, 2W, C] (up != 0) or [B, H/2, W/2, C]; any C >= 1 (C % 4 == 0 with 16-byte aligned x and out takes the 16-byte form, the
 * same sums in the same order), deterministic. */
int csd_fir_resample_nhwc(const float* x, float* out, int B, int H, int W, int C, const float* fir_kernel, int up, void* stream);
int csd_fused_bias_act(const float* x, const float* bias, const float* ref, float* out, int64_t numel,
                       int C, int64_t inner, int act, int grad, float alpha, float scale, void* stream);
/* nearest-neighbour x2 upsample (F.interpolate in models/layers.py:601) */
int csd_nearest_up2(const float* x, float* out, int N, int C, int H, int W, void* stream);
/* sinusoidal timestep embedding (models/layers.py:524-538): out [B, dim] */
int csd_timestep_embedding(const float* t, float* out, int B, int dim, void* stream);

/* ------------------------------------------------------------------------------------------
 * Small operators for graphs orchestrated above the C ABI (the NCSN++ adapter, models/ncsnpp.py:238-388):
 * ---------------------------------------------------------------------------------------- */
/* nn.Linear on the activated input: out[b] = act_in(in[b]) . weight^T + bias; weight [N, K] (temb MLP
 * models/ncsnpp.py:96-102,257-263; Dense_0 models/layerspp.py:253-255) */
int csd_linear(const float* in, const float* weight, const float* bias, float* out, int B, int K, int N,
               int act_in, void* stream);
/* GaussianFourierProjection (models/layerspp.py:32-41): out [B, 2E] = [sin(2 pi W t), cos(2 pi W t)] */
int csd_fourier_embedding(const float* t, const float* W, float* out, int B, int E, void* stream);
/* out = (alpha*a + beta*b + gamma) * post, b may be NULL: x + h, (x + h)/sqrt(2) (layerspp.py:271-274),
 * Combine 'sum' (:56-57), 2x - 1 (ncsnpp.py:266-268), pyramid sums (:352) */
int csd_axpby(const float* a, const float* b, float* out, float alpha, float beta, float gamma, float post,
              int64_t n, void* stream);
/* The resamplers of csd_unet_config.y_scale as operators, on n contiguous planes (the same device functions as the network's boundary
 * kernels): csd_bilinear_up y [n, side, side] -> out [n, scale * side, scale * side]; csd_bilinear_down v [n, side, side] -> out
 * [n, side / scale, side / scale] (side % scale == 0); csd_bilinear_down_adjoint g [n, side / scale, side / scale] -> out
 * [n, side, side], the transpose of csd_bilinear_down (every element of out is written).  scale >= 2. */
int csd_bilinear_up(const float* y, float* out, int64_t n, int side, int scale, void* stream);
int csd_bilinear_down(const float* v, float* out, int64_t n, int side, int scale, void* stream);
int csd_bilinear_down_adjoint(const float* g, float* out, int64_t n, int side, int scale, void* stream);
/* out[b,c,:] = act(x[b,c,:] + bias[b*bias_stride + c]): h += Dense_0(act(temb))[:, :, None, None] */
int csd_bias_add_nchw(const float* x, const float* bias, float* out, int B, int C, int64_t inner,
                      int bias_stride, int act, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient operators (csrc/backward.hip) - the autograd backward the reference gets from torch for its layers
 * (the training step of run_lib.py:55-73 / losses.py:99-232).  NCHW fp32 like the forward
 * operators.  The DATA gradient of a convolution is csd_conv2d on dy with the flipped, transposed weight (stride 2:
 * dy zero-inserted with csd_upfirdn2d; nearest-x2: a 2x2 sum of the result), so only the weight gradient is new.
 * ---------------------------------------------------------------------------------------- */
/* dw[Cout, Cin, k, k] = sum over batch and pixels of dy (x) x for the convolution csd_conv2d(x; ksize, stride,
 * pad_mode, up2) with x [B, Cin, H, W], dy [B, Cout, OH, OW].  fp32 MFMA, deterministic split-K reduction. */
size_t csd_conv_wgrad_scratch_bytes(int B, int Cin, int Cout, int H, int W, int ksize, int stride, int up2);
int csd_conv2d_wgrad(const float* x, const float* dy, float* dw, int B, int Cin, int Cout, int H, int W, int ksize,
                     int stride, int pad_mode, int up2, void* scratch, void* stream);
/* backward of csd_groupnorm_act: dx [B,C,H,W]; dgamma_rows / dbeta_rows [B, C] hold the per-sample sums
 * (dgamma = csd_sum_rows of them) */
int csd_groupnorm_act_backward(const float* x, const float* gamma, const float* beta, const float* dy, float* dx,
                               float* dgamma_rows, float* dbeta_rows, int B, int C, int H, int W, int groups, float eps,
                               int act, void* stream);
/* backward of csd_attention: dq, dk, dv from dout; scratch csd_attention_backward_scratch_bytes() */
size_t csd_attention_backward_scratch_bytes(int B, int C, int H, int W);
int csd_attention_backward(const float* q, const float* k, const float* v, const float* dout, float* dq, float* dk,
                           float* dv, int B, int C, int H, int W, void* scratch, void* stream);
/* strided batched fp32 GEMM  C[z][m*scm + n*scn] = alpha * sum_k A[z][m*sam + k*sak] * B[z][k*sbk + n*sbn]
 * (z-strides za, zb, zc): the Linear / NIN-free contractions of the backward (dIn = dOut.W, dW = dOut^T.act(in)) */
int csd_bgemm(const float* A, const float* B, float* C, int M, int N, int K, int64_t sam, int64_t sak, int64_t sbk,
              int64_t sbn, int64_t scm, int64_t scn, int batch, int64_t za, int64_t zb, int64_t zc, float alpha,
              void* stream);
/* out[r] = sum of row r ([rows, inner], fp64 accumulation): per-(sample, channel) sums of dy = gradient of a
 * broadcast bias / time-embedding add;  out[c] = sum_r x[r][c]: the batch reduction that follows */
int csd_sum_inner(const float* x, float* out, int64_t rows, int64_t inner, void* stream);
int csd_sum_rows(const float* x, float* out, int R, int C, void* stream);
/* dy == NULL: out = act(x); else out = dy * act'(x) */
int csd_act(const float* x, const float* dy, float* out, int act, int64_t n, void* stream);
int csd_mul(const float* a, const float* b, float* out, int64_t n, void* stream);
/* nn.Dropout(p) in training mode (models/layers.py:647,662): mask = (u >= p)/(1-p) from Philox4x32-10 keyed by
 * (seed, stream_id), out = x * mask; the backward is csd_mul(dy, mask) */
int csd_dropout(const float* x, float* out, float* mask, float p, uint64_t seed, uint64_t stream_id, int64_t n,
                void* stream);

/* ------------------------------------------------------------------------------------------
 * Parameter update of a training step on flat fp32 buffers (csrc/optim.hip): global-norm clipping
 * (torch.nn.utils.clip_grad_norm_, losses.py:48-49; grad_norm = device scalar ||grad||_2 from csd_global_norm, NULL
 * or max_norm < 0: no clipping) + torch.optim.Adam (losses.py:12-23) + the EMA of models/ema.py:61-90 (ema may be
 * NULL) in one pass.  `step` is the 1-based update count (bias correction); lr already carries the warm-up factor.
 * ---------------------------------------------------------------------------------------- */
int csd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                  const float* grad_norm, int64_t n, int step, float lr, float beta1, float beta2, float eps,
                  float weight_decay, float max_norm, float ema_decay, void* stream);
/* out[0] = ||a||_2 of one long vector (fp64 partials of 1024 workgroups added in index order): the total gradient norm */
size_t csd_global_norm_scratch_bytes(void);
int csd_global_norm(const float* a, float* out, int64_t n, void* scratch, void* stream);
/* ema -= (1 - decay) * (ema - param)  (models/ema.py:85-89) */
int csd_ema_update(float* ema, const float* param, int64_t n, float decay, void* stream);

/* ------------------------------------------------------------------------------------------
 * The denoising score-matching objective of a training step (csrc/dsm_loss.hip; losses.py:55-232 of the reference) as two passes
 * around csd_unet_train_forward.  Every score function is score = s_b h with a per-sample factor, so each variant of the objective is
 *     loss = sum_b sum_segments w_b sum_i (a_b h[b, i] + b_b z[b, i])^2
 * over 1 or 2 segments of the network's flat per-sample output row: the caller folds the SDE (marginal std, g^2, the score scaling),
 * the per-sample reduction (mean or half sum) and the batch mean (1 / B) into the per-sample device arrays a, b, w [B] - written on
 * the host and uploaded in one copy per step; neither entry synchronises with the host.
 * Noise: z is a device tensor, or NULL = element b * length + i of a csd_randn fill of (seed, stream_id) made in registers -
 * bit-identical to passing that fill, without writing or reading it.  csd_dsm_perturb and csd_dsm_residual given the same
 * (seed, stream_id) see the same normals.  A training step that keys its dropout masks by (seed, (call << 16) + k) - the planned
 * network does, call < 2^47 - keeps the noise disjoint from them with stream ids that have bit 63 set.
 * Both entries validate before they touch the device (CSD_ERR_INVALID, csd_last_error names the cause); results are bitwise repeatable
 * and a sample's values depend on its batch position only through its Philox element numbers.
 * ---------------------------------------------------------------------------------------- */
/* xt[b, i] = fl(fl(m[b] x[b, i]) + fl(std[b] z[b, i])): three single roundings, no contraction.  x, xt [B, per_sample] (distinct buffers);
 * m, std device [B]; m == NULL: m[b] = 1 (the VE SDEs).  16-byte accesses when x, xt and z allow them. */
int csd_dsm_perturb(float* xt, const float* x, const float* m, const float* std, const float* z, int B, int64_t per_sample,
                    uint64_t seed, uint64_t stream_id, void* stream);
#define CSD_DSM_PARTS 64
typedef struct csd_dsm_segment {
  int64_t offset, length;     /* floats: the segment is [offset, offset + length) of every sample's row */
  const float* a;             /* device [B] each */
  const float* b;
  const float* w;
  const float* z;             /* device [B, length], or NULL: the csd_randn fill of (seed, stream_id) */
  uint64_t stream_id;
} csd_dsm_segment;
/* net: sample b's row starts at net + b * net_stride.  segments: a HOST array of n_seg = 1 or 2 disjoint segments inside
 * [0, net_stride) (the x block and the y block of a paired network, in either order).
 *   d_out (or NULL: nothing written) [B, net_stride]: 2 w a (a h + b z) on the segments - the gradient of *loss with respect to net,
 *       csd_unet_backward_acc's d_out - and 0 at every row position outside them;
 *   partials: B * n_seg * CSD_DSM_PARTS doubles of scratch, every one written before it is read;
 *   loss_rows [B] doubles: sum of w (a h + b z)^2 over the sample's segments, fp64, added in a fixed order;
 *   loss: one float = the rows added in index order (with 1 / B in w: the batch mean of the per-sample losses).
 * Refused: B < 1 or > 65535, n_seg outside 1..2, a null or misaligned pointer (floats 4 bytes, doubles 8), a segment that is empty or
 * reaches beyond net_stride, overlapping segments. */
int csd_dsm_residual(const float* net, int64_t net_stride, const csd_dsm_segment* segments, int n_seg, float* d_out, double* partials,
                     double* loss_rows, float* loss, int B, uint64_t seed, void* stream);

/* ------------------------------------------------------------------------------------------
 * NHWC forms of the training operators (csrc/train_nhwc.hip): the differentiable DDPM-family graph keeps activations in
 * the library's internal layout [B, H, W, C], so no layer pays an NCHW<->NHWC change.  Same kernels as above.
 * ---------------------------------------------------------------------------------------- */
/* The DDPM family's first layer as an operator (models/ddpm.py:163-168 + :283 + the first conv3x3): out [B, S, S, Cout] NHWC =
 * conv3x3(2 cat(x, y + y_sigma y_noise) - 1) (no 2v - 1 when centered), x [B, Cx, S, S], y [B, Cy, S, S] (NULL iff Cy == 0), y_noise
 * like y or NULL, weight OIHW [Cout, Cx + Cy, 3, 3], bias [Cout]; Cx + Cy <= CSD_MAX_IO_CHANNELS.
 *   fused = 1: the one-launch layer of csrc/stem.hip (fp16-operand precisions, S % 16 == 0, Cout % 64 == 0 or % 96 == 0; up to 8 input
 *              channels stem_kernel, 9 .. 32 stem_wide_kernel); stats (or NULL): [B * (S / 16) * (S / 8)][Cout][2] doubles, the (sum, sum of
 *              squares) of every 16 x 8 tile of the written tensor.  An unsupported shape is CSD_ERR_INVALID, never another kernel.
 *   fused = 0: what a network's plan runs where the fused layer does not apply: the input assembled at its padded width (up to 8
 *              channels: 8 in CSD_PREC_F32, 16 otherwise; above 8 the next multiple of 16; exact zeros in the padding), then the generic
 *              3x3 convolution of that precision.  stats must be NULL.
 * scratch: csd_conv_scratch_bytes(B, 32, Cout, S, S, 3, 0) device bytes - those of a 32-input-channel 3x3 convolution - 256-byte aligned
 * (assembled input, packed weight, padded bias). */
int csd_input_conv(const float* x, const float* y, const float* y_noise, float y_sigma, const float* weight, const float* bias, float* out,
                   double* stats, int B, int Cx, int Cy, int Cout, int S, int centered, int precision, int fused, void* scratch,
                   void* stream);
/* csd_input_conv for the first layer of a csd_unet_config.y_scale network: y, y_noise [B, Cy, S / y_scale, S / y_scale], the layer sees
 * the bilinear upsample of y + y_sigma y_noise (perturbed at low resolution).  y_scale >= 2, Cx + Cy <= 8; fused: Cx <= 4, Cy <= 4.
 * Scratch as csd_input_conv. */
int csd_input_conv_kx(const float* x, const float* y, const float* y_noise, float y_sigma, const float* weight, const float* bias,
                      float* out, double* stats, int B, int Cx, int Cy, int Cout, int S, int y_scale, int centered, int precision,
                      int fused, void* scratch, void* stream);

/* The ResnetBlock convolution with its prologue fused (csrc/conv_ff.hip; reference models/layers.py:632-675: Conv(act(GroupNorm(x)))
 * [+ Dense(temb)] [+ x]): 3x3, stride 1, pad 1 on NHWC fp32 tensors.  x0 [B,H,W,C0] (+ x1 [B,H,W,C1] or NULL: virtual concat),
 * H % 16 == 0, W % 16 == 0 (CSD_PREC_F16X3 layers of the Winograd form - an even number >= 4 of 16-channel stages - also H % 8 == 0, W % 8 == 0
 * with tiles at least 65 % full, e.g. 40 x 40: ragged 16 x 16 tiles, csrc/conv_xk.hip), C0 / C1 multiples of 32, Cout a multiple of 96 (three 32-cout tiles per workgroup: the nf = 96 nets) or of
 * 64 (two: the nf = 128 nets); weight OIHW [Cout, C0+C1, 3, 3]; nscale / nshift
 * [B, C0+C1] = the GroupNorm's per-(sample, channel) rstd*gamma and beta - mean*rstd*gamma, applied as SiLU(x*scale + shift)
 * while the operand is staged (both NULL: the convolution reads x as it is); temb [B, temb_stride] or NULL (column c of sample b
 * is added to cout c), res [B,H,W,Cout] or NULL (added), out_scale multiplies the result.  stats (or NULL):
 * [B*ceil(H/16)*ceil(W/16)][Cout][2] doubles = per-tile (sum, sum of squares) of the written tensor (valid pixels only).  precision: CSD_PREC_F16X3, CSD_PREC_F16F8 (the
 * split operands with the two correction products on the fp8 matrix cores; 1.3e-5 / 4.5e-5 network error, see csd_precision) or CSD_PREC_F16.  scratch holds the packed weight: csd_conv3x3_block_scratch_bytes(C0 + C1, Cout). */
size_t csd_conv3x3_block_scratch_bytes(int Cin, int Cout);
int csd_conv3x3_block(const float* x0, const float* x1, const float* weight, const float* bias, const float* nscale,
                      const float* nshift, const float* temb, int temb_stride, const float* res, float out_scale, float* y,
                      double* stats, int B, int C0, int C1, int Cout, int H, int W, int precision, void* scratch, void* stream);

/* csd_conv2d / csd_conv2d_wgrad with layout flags: bit 0 = first tensor operand (x) is NHWC, bit 1 = second (y resp. dy) is
 * NHWC.  An NHWC x needs Cin % 8 == 0.  csd_conv2d_ex bit 2: `weight` is the OIHW weight [Cin, Cout, k, k] of the TRANSPOSED
 * convolution and is applied transposed + spatially flipped (the data gradient, without materialising that weight).
 * csd_conv2d_wgrad_ex bit 2: the stride-1 weight gradient may run with split-bf16
 * operands on the bf16 matrix cores (hi*hi + hi*lo + lo*hi, ~2^-16 relative error per product) instead of exact fp32 MFMA. */
enum {
  CSD_IN_NHWC = 1,           /* bit 0 */
  CSD_OUT_NHWC = 2,          /* bit 1 */
  CSD_WEIGHT_T = 4,          /* bit 2 of csd_conv2d_ex */
  CSD_SPLIT_BF16 = 4         /* bit 2 of csd_conv2d_wgrad_ex */
};
int csd_conv2d_ex(const float* x, const float* weight, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                  int ksize, int stride, int pad_mode, int up2, int precision, int layout, void* scratch, void* stream);
int csd_conv2d_wgrad_ex(const float* x, const float* dy, float* dw, int B, int Cin, int Cout, int H, int W, int ksize,
                        int stride, int pad_mode, int up2, int layout, void* scratch, void* stream);
/* GroupNorm(+act) on [B, HW, C]; rs / ms [B, C] receive (rstd, -mean*rstd) per channel for the backward */
size_t csd_groupnorm_nhwc_scratch_bytes(int B, int C, int HW);
int csd_groupnorm_act_nhwc(const float* x, const float* gamma, const float* beta, float* y, float* rs, float* ms, int B,
                           int C, int HW, int groups, float eps, int act, void* scratch, void* stream);
int csd_groupnorm_act_backward_nhwc(const float* x, const float* gamma, const float* beta, const float* rs, const float* ms,
                                    const float* dy, float* dx, float* dgamma_rows, float* dbeta_rows, int row_stride, int B, int C,
                                    int HW, int groups, int act, void* scratch, void* stream);
/* out[b,p,c] = x[b,p,c] + bias[b,c];  csd_sum_pixels_nhwc: out[b,c] = sum_p x[b,p,c] (the gradient of that add; a conv bias gradient after
 * csd_sum_rows).  csd_groupnorm_act_backward_nhwc writes row b of dgamma / dbeta at b*row_stride, so both
 * can live in one [B, 2C] buffer that a single csd_sum_rows reduces. */
int csd_bias_add_nhwc(const float* x, const float* bias, float* out, int B, int HW, int C, void* stream);
size_t csd_sum_pixels_scratch_bytes(int B, int HW, int C);
int csd_sum_pixels_nhwc(const float* x, float* out, int B, int HW, int C, void* scratch, void* stream);
/* data-gradient helpers of the resampling convolutions: dy on the odd positions of a 2h x 2w grid; 2x2 block sums */
int csd_zero_insert_odd_nhwc(const float* dy, float* z, int B, int h, int w, int C, void* stream);
int csd_sumpool2_nhwc(const float* in, float* out, int B, int h, int w, int C, void* stream);
/* attention core and its backward on the packed qkv tensor [B, L, 3C] (q | k | v per pixel); out, dout [B, L, C];
 * scratch of the backward: csd_attention_backward_scratch_bytes(B, C, L, 1) */
int csd_attention_nhwc(const float* qkv, float* out, int B, int L, int C, void* stream);
/* the same forward core in the arithmetic csd_unet_forward uses in precision mode `precision` (CSD_PREC_*): F32 = the call above;
 * F16X3 / F16F8 = operands split hi + lo on the fp16 matrix cores (fp32-class); F16 = plain fp16 operands */
int csd_attention_nhwc_prec(const float* qkv, float* out, int B, int L, int C, int precision, void* stream);
int csd_attention_backward_nhwc(const float* qkv, const float* dout, float* dqkv, int B, int L, int C, void* scratch,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * Training step of the DDPM-family network as ONE planned graph (replaces torch autograd over
 * models/ddpm.py:149-213 + models/layers.py:524-675 in `model.train()` mode, run_lib.py:55-73).
 *   csd_unet_train_forward: the forward with nn.Dropout(dropout_p) active (mask = Philox keyed by (dropout_seed,
 *     (call_index << 16) + running dropout index), models/layers.py:647,662); every tensor a gradient needs stays in `workspace`.
 *   csd_unet_backward: given d loss / d out ([B, out_channels, S, S]), writes d loss / d parameter i to grads[i] (overwrite; csd_unet_backward_acc
 *     below adds instead).
 * params[i] / grads[i]: device pointers of parameter i in csd_unet_param_info order and layout (fp32, 16-byte aligned).
 * One backward per forward, same handle / workspace / B / call_index; the workspace must not be touched in between: a second
 * forward into the same workspace before the backward makes that backward fail with CSD_ERR_STATE (it names the first forward's
 * call_index) - two forwards of one network may be alive at once when each has its own workspace.
 * csd_unet_train_workspace_bytes depends on B and on whether dropout_p > 0.  All architectures: arch 0 (models/ddpm.py:149-213),
 * arch 1 (NCSN++, models/ncsnpp.py:238-388: BigGAN blocks with FIR up / down sampling, Combine 'sum', input / output pyramids) and
 * arch 2 with csd_unet_config.planned_train = 1 (the 3-D DDPM family, models/ddpm3D.py:107-171; csrc/train_graph3d.h): x, y, out, d_out and d_x are NCDHW with D, H, W in place
 * of S, S; the layers, kernels and dropout streams are those of the per-operator training path (csd_conv3d_block without prologue,
 * csd_groupnorm_act_nhwc with S = D*H*W, csd_conv3d_wgrad, the data gradient scaled by csd_conv3d_dgrad_scale's power of two), so the
 * same (dropout_seed, call_index) draws the same masks on both.  Every option below holds for arch 2 as it does for arch 0 / 1.
 * ---------------------------------------------------------------------------------------- */
size_t csd_unet_train_workspace_bytes(csd_unet* net, int B, float dropout_p);
int csd_unet_train_forward(csd_unet* net, const float* const* params, void* workspace, size_t workspace_bytes, const float* x,
                           const float* y, const float* labels, float* out, int B, float dropout_p, uint64_t dropout_seed,
                           uint64_t call_index, void* stream);
int csd_unet_backward(csd_unet* net, const float* const* params, float* const* grads, void* workspace, size_t workspace_bytes,
                      const float* d_out, int B, uint64_t call_index, void* stream);
/* csd_unet_backward_ex: csd_unet_backward with optional outputs.
 *   grads == NULL: no parameter gradient is formed (no wgrad, no bias sums, no temb-MLP backward, no gradient-ready marks).
 *   d_x != NULL:   d loss / d x, [B, x_channels, S, S] NCHW fp32 (arch 2: [B, x_channels, D, H, W]; the x channels of the input only,
 *     times the 2v - 1 input map's factor when not centred; y takes no gradient).
 * csd_unet_backward(...) is csd_unet_backward_ex(..., grads, NULL).  The data-gradient kernels are the same with or without grads,
 * so d_x does not depend on whether parameter gradients are formed.  Both architectures; NCSN++ with every progressive_input:
 * 'input_skip' (the input pyramid's gradient chain: d pyr_l = Conv_0^T(dh_l) + FIR-down^T(d pyr_l+1), d x += FIR-down^T(d pyr_1)),
 * 'residual' (the pyramid convolution's data gradient flows into the previous level's combined h - always, the parameter gradients
 * depend on it - and, at level 0, into d_x). */
int csd_unet_backward_ex(csd_unet* net, const float* const* params, float* const* grads, float* d_x, void* workspace,
                         size_t workspace_bytes, const float* d_out, int B, uint64_t call_index, void* stream);
/* csd_unet_backward_acc: csd_unet_backward_ex for gradient accumulation over micro-batches (Lightning's accumulate_grad_batches,
 * run_lib.py:58,68,98).  csd_unet_backward_ex(...) is csd_unet_backward_acc(..., accumulate = 0, record_marks = 1).
 *   accumulate = 1: grads[i] = grads[i] + v for every parameter, v bit for bit the fp32 value the overwrite form stores (a value that
 *     comes out of an fp64 reduction is rounded to fp32 first), the sum ONE fp32 addition: autograd's p.grad += g.  The add sits in
 *     the final writer of each gradient (no pass over all parameters, no atomics, the same split-K order: bitwise repeatable).
 *     The slot of a parameter that takes no gradient (the fixed Gaussian-Fourier W) is left untouched.  Needs grads != NULL.
 *     d_x does not depend on `accumulate`.
 *   record_marks = 0: the gradient-ready events (csd_unet_backward_marks) are not recorded and csd_unet_backward_marks_epoch does not
 *     advance - the micro-batches of a window whose gradients are not final yet; the window's last backward passes 1. */
int csd_unet_backward_acc(csd_unet* net, const float* const* params, float* const* grads, float* d_x, void* workspace,
                          size_t workspace_bytes, const float* d_out, int B, uint64_t call_index, int accumulate, int record_marks,
                          void* stream);
/* The library keeps one recorded training graph per (handle, workspace).  A caller that frees a workspace (a monitoring forward's
 * private one) tells the library so: the record is dropped (no error if there is none).  csd_unet_destroy drops all of a handle's. */
int csd_unet_train_release(csd_unet* net, const void* workspace);
/* The same for the record of ONE forward: dropped only if it still is the record of csd_unet_train_forward call `call_index` (a late
 * release must not erase the record of a newer forward that was given the same workspace address). */
int csd_unet_train_release_call(csd_unet* net, const void* workspace, uint64_t call_index);
/* Gradient-ready marks - what Lightning-DDP's bucketed all-reduce hooks into autograd for (run_lib.py:55-73), for a backward that is
 * ONE call: while csd_unet_backward enqueues its kernels on `stream`, it records events[k] on that stream as soon as every gradient
 * of the modules with all_modules index >= first_module[k] is final (the backward walks all_modules back to front; the embedding
 * MLP's gradients come last).  A data-parallel caller makes its communication stream wait for events[k] and launches the
 * all-reduce of that bucket there: the reduction of the late layers' gradients overlaps the backward of the early ones.
 * The marks stay registered on the handle until replaced or cleared (n = 0); the events are the caller's.
 * csd_unet_backward_marks_epoch: number of csd_unet_backward calls of this handle that recorded every mark (a caller checks that it
 * advanced before trusting the events). */
int csd_unet_backward_marks(csd_unet* net, const int* first_module, void* const* events, int n);
uint64_t csd_unet_backward_marks_epoch(csd_unet* net);
void* csd_event_create(void);                         /* hipEventDisableTiming; NULL on failure */
int csd_event_destroy(void* event);
int csd_stream_wait_event(void* stream, void* event);
int csd_event_query(void* event);                     /* 1: complete, 0: not yet, < 0: error */

/* ------------------------------------------------------------------------------------------
 * Probability-flow ODE right-hand side of the likelihood (csrc/likelihood.hip; reference likelihood.py:53-103 get_likelihood_fn
 * with the Hutchinson-Skilling divergence of get_div_fn).  Rows b < B of D = x_channels * S * S values; the state is scipy's
 * flattened float64 vector: y = [x (B * D) | log p (B)].
 *   csd_pf_ode_state: x32 [B, D] = float(y_x), labels32 [B] = float(labels)   (the network's fp32 operands; labels may be NULL)
 *   csd_pf_ode_rhs:   out [B * D + B] float64:
 *       out[b*D + i] = a[b] * y[b*D + i] + c[b] * h[b*net_stride + i]                     (drift = f + c * h, f = a * x)
 *       out[B*D + b] = a[b] * sum_i eps_i^2 + c[b] * sum_i v[b*D + i] * eps_i               (eps_i = eps[b*net_stride + i])
 *     h = the raw network output, eps = the Hutchinson noise as the backward's d_out, both [B, net_stride] with the x channels
 *     first (net_stride = out_channels * S * S); v = d (h . eps) / d x [B, D] (csd_unet_backward_ex's d_x).  The row sums are
 *     fp64, deterministic: fixed-order partials of several workgroups per row, then a fixed-order finalize.
 *     scratch: csd_pf_ode_scratch_bytes(B, D).
 * ---------------------------------------------------------------------------------------- */
int csd_pf_ode_state(const double* y, const double* labels, float* x32, float* labels32, int B, int64_t D, void* stream);
size_t csd_pf_ode_scratch_bytes(int B, int64_t D);
int csd_pf_ode_rhs(const double* y, const float* h, const float* v, const float* eps, int64_t net_stride, const double* a,
                   const double* c, double* out, int B, int64_t D, void* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Embedded Runge-Kutta 5(4) on a device-resident state (csrc/ode_rk45.hip): the vector arithmetic of one Dormand-Prince step for
 * the probability-flow ODE sampler and the likelihood, so that the state and the stage derivatives never leave the device and a
 * step costs the host one 8-byte read.  y, ynew, out [n] and K [7 rows, row j at K + j * k_stride, |k_stride| >= n] are float64.
 * A negative k_stride walks the rows backwards: the last stage of an accepted step becomes the first of the next without a copy.
 * For the likelihood n = B * D + B (csd_pf_ode_rhs's layout: a K row is its `out`), for the sampler n = B * D.  A tableau row is
 * passed by value (csd_ode_coef): no device table, no upload.
 *   csd_ode_combine:      out[i] = y[i] + h * sum_{j < s} coef.c[j] * K[j * k_stride + i], 1 <= s <= 7 (j ascending); with
 *       nx > 0 the same pass writes x32[i] = float(out[i]) for i < nx <= n (the network's fp32 input: no csd_pf_ode_state pass).
 *       out may alias neither y nor the s rows of K that are read.
 *   csd_ode_error_sumsq:  result[0] = sum_i (h * sum_{j < 7} E.c[j] * K[j * k_stride + i] / (atol + rtol * max(|y[i]|, |ynew[i]|)))^2
 *   csd_ode_scaled_sumsq: result[0] = sum_i ((alpha * u[i] + beta * w[i]) / (atol + rtol * |y[i]|))^2; w may be NULL (beta unused).
 *   csd_ode_drift:        out[b*D + i] = a[b] * y[b*D + i] + c[b] * h[b*net_stride + i]: csd_pf_ode_rhs without the divergence
 *       sums (the ODE sampler's right-hand side); a, c [B] float64 on the device, h the raw network output (fp32).
 *     y, ynew, K, out, x32 and scratch are 16-byte aligned (rows of an odd k_stride are read with 8-byte accesses).  result is a
 *     device double.  The sums are fp64 and deterministic: one partial per workgroup, lanes in a fixed tree, then one workgroup adds
 *     the partials in index order; no atomics.  scratch: csd_ode_scratch_bytes bytes for this n, not shared between streams.
 * ---------------------------------------------------------------------------------------- */
typedef struct { double c[7]; } csd_ode_coef;
size_t csd_ode_scratch_bytes(int64_t n);
int csd_ode_combine(const double* y, const double* K, int64_t k_stride, int s, csd_ode_coef coef, double h, double* out, float* x32,
                    int64_t nx, int64_t n, void* stream);
int csd_ode_error_sumsq(const double* y, const double* ynew, const double* K, int64_t k_stride, csd_ode_coef E, double h, double atol,
                        double rtol, int64_t n, double* result, void* scratch, void* stream);
int csd_ode_scaled_sumsq(const double* u, const double* w, double alpha, double beta, const double* y, double atol, double rtol,
                         int64_t n, double* result, void* scratch, void* stream);
int csd_ode_drift(const double* y, const float* h, int64_t net_stride, const double* a, const double* c, double* out, int B, int64_t D,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * 3-D operators of the ddpm3D score networks (csrc/conv3d.hip; reference models/ddpm3D.py:38-171 with models/layers.py:119-132 ddpm_conv3x3
 * dim = 3, :593-629 Upsample / Downsample dim = 3, :632-675 ResnetBlockDDPM dim = 3).  Channels-last fp32 tensors [B, D, H, W, C].
 * ---------------------------------------------------------------------------------------- */
/* The 3-D counterpart of csd_conv3x3_block: y = (Conv3x3x3(act(x*nscale + nshift)) + bias + temb + res) * out_scale, stride 1, zero padding 1
 * in all three dimensions.  x = x0 [B,D,H,W,C0] (| x1 [B,D,H,W,C1] or NULL with C1 = 0: virtual concat, no copy); weight in the
 * reference's state_dict layout [Cout, C0+C1, 3, 3, 3]; bias [Cout] or NULL; nscale / nshift [B, C0+C1] (csd_groupnorm_scale_shift) or both
 * NULL: the convolution reads x as it is and `act` is ignored (the stem, the shortcut Conv_2); act = CSD_ACT_*; temb [B, temb_stride] or
 * NULL (column c of sample b is added to cout c); res [B,D,H,W,Cout] or NULL (added).  The padding is applied AFTER the prologue: a voxel
 * outside the volume contributes exactly 0.  The result is bitwise repeatable and independent of the sample's position in the batch.
 * precision: CSD_PREC_F16X3 (split-fp16 operands on v_mfma_f32_32x32x16_f16, fp32 accumulate) or CSD_PREC_F32 (the exact yardstick: one
 * fp32 fmaf chain per output, swish with expf and a true division, not tuned); CSD_PREC_F16 / CSD_PREC_F16F8 return CSD_ERR_INVALID.
 * Domain: any B, D, H, W >= 1 and Cout >= 1; with C1 = 0 any C0 >= 1 (C0 not a multiple of 16 runs on the direct fp32 kernel in both
 * modes); with C1 > 0 both C0 and C1 multiples of 16; one sample of the widest tensor below 2 GiB.  Anything else returns
 * CSD_ERR_INVALID and writes nothing.  scratch holds the packed weight: csd_conv3d_block_scratch_bytes(C0 + C1, Cout). */
size_t csd_conv3d_block_scratch_bytes(int Cin, int Cout);
int csd_conv3d_block(const float* x0, const float* x1, const float* weight, const float* bias, const float* nscale, const float* nshift,
                     int act, const float* temb, int temb_stride, const float* res, float out_scale, float* y, int B, int C0, int C1,
                     int Cout, int D, int H, int W, int precision, void* scratch, void* stream);
/* Weight gradient of csd_conv3d_block's convolution: dw[co][ci][kd][kh][kw] = sum over b and voxels v of dy[b, v, co] * a[b, v + tap, ci],
 * a [B,D,H,W,Cin] (the convolution's input AFTER its prologue), dy [B,D,H,W,Cout], channels-last fp32; dw [Cout, Cin, 3, 3, 3] (the
 * reference's state_dict layout, overwritten).  Zero padding 1, stride 1: a voxel outside the volume contributes exactly 0 (masked).
 * precision: CSD_PREC_F16X3 = split-bf16 operands on v_mfma_f32_32x32x16_bf16 (hi = truncated bf16, lo = bf16(x - hi), products
 * hi*hi + hi*lo + lo*hi, fp32 accumulate: no exponent-range limit, unlike the forward's fp16 halves); CSD_PREC_F32 = the exact yardstick
 * (one fp32 fmaf chain per weight and K split, not tuned).  Rule for thin layers: with min(Cin, Cout) < 8 (the 1- / 2-channel stem and
 * head) CSD_PREC_F16X3 runs the fp32 kernel too - a 32 x 32 MFMA tile would be at least 75 % padding.
 * K splits are runs of voxels of ONE sample, their number depends on the volume and the channel counts only, and they are summed in
 * fp64 in split order: no atomics, bitwise repeatable, and a sample's contribution does not depend on B or on the other samples.
 * Domain: any B, D, H, W >= 1, any Cin, Cout >= 1 (one sample of the widest tensor below 2 GiB); anything else, another precision or a
 * null pointer returns CSD_ERR_INVALID and writes nothing.  scratch: csd_conv3d_wgrad_scratch_bytes(...) device bytes (0 = invalid). */
size_t csd_conv3d_wgrad_scratch_bytes(int B, int Cin, int Cout, int D, int H, int W, int precision);
int csd_conv3d_wgrad(const float* a, const float* dy, float* dw, int B, int Cin, int Cout, int D, int H, int W, int precision,
                     void* scratch, void* stream);
/* Range-safe data gradient dx = csd_conv3d_block(dy; flip(W)^T): the forward kernel's fp16 hi | lo operands lose their lo half below
 * ~6e-5, where loss gradients live.  rowscale[b] = 2^(4 - floor(log2 max|dy_b|)) (1 for an all-zero or non-finite sample), and
 * nscale[b][c] = rowscale[b], nshift[b][c] = 0 for c < C are csd_conv3d_block's prologue operands with act = none: an EXACT multiply in
 * its staging that puts max|dy_b| into [16, 32).  csd_scale_rows(dx, dx, rowscale, divide = 1) undoes it exactly.
 * dy [B, per_sample]; scratch: csd_conv3d_dgrad_scale_scratch_bytes(B). */
size_t csd_conv3d_dgrad_scale_scratch_bytes(int B);
int csd_conv3d_dgrad_scale(const float* dy, float* rowscale, float* nscale, float* nshift, int B, int64_t per_sample, int C, void* scratch,
                           void* stream);
/* nn.AvgPool3d(kernel_size=2, stride=2) (models/layers.py:617): x [B,D,H,W,C] -> out [B,D/2,H/2,W/2,C]; D, H, W even */
int csd_avgpool3d_2_ndhwc(const float* x, float* out, int B, int D, int H, int W, int C, void* stream);
/* F.interpolate(x, 2 * size, mode='nearest') on a volume (models/layers.py:601): x [B,D,H,W,C] -> out [B,2D,2H,2W,C] */
int csd_nearest_up2_3d_ndhwc(const float* x, float* out, int B, int D, int H, int W, int C, void* stream);
/* GroupNorm statistics without the normalised tensor: nscale / nshift [B, C0+C1] = rstd*gamma and beta - mean*rstd*gamma per
 * (sample, channel) of x = x0 [B,S,C0] (| x1 [B,S,C1] or NULL with C1 = 0) over S positions - the prologue operands of csd_conv3d_block
 * and csd_conv3x3_block.  C0 and C1 multiples of 4.  scratch: csd_groupnorm_scale_shift_scratch_bytes(B, C0+C1, S, groups). */
size_t csd_groupnorm_scale_shift_scratch_bytes(int B, int C, int S, int groups);
int csd_groupnorm_scale_shift(const float* x0, const float* x1, const float* gamma, const float* beta, float* nscale, float* nshift, int B,
                              int C0, int C1, int S, int groups, float eps, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CSD_H_ */
