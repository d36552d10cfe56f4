/*
 * a2p_hip.h -- C ABI of liba2p_hip.so, the MI355X (gfx950) implementation of
 * audio2photoreal's audio-to-motion diffusion sampling hot path.
 *
 * The reference is pure Python/PyTorch and has NO FFI for this path (SURVEY.md
 * §0, §8b "C-ABI to define (new; nothing to mirror)").  Each entry point below
 * therefore cites the reference *Python* interface it replaces
 * (paths relative to /root/reference); INTEGRATION.md shows the ctypes binding a
 * reference maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *  - tensors are dense row-major fp32 unless stated; int64 for timesteps
 *    (the reference passes torch.long, gaussian_diffusion.py:911);
 *  - all work is enqueued on `stream` (a hipStream_t passed as void*); nothing
 *    synchronises the device except a2p_ctx_destroy, a2p_kernel_time_ms, a2p_dual_audio
 *    (which reads one float back) and a2p_conversation_audio under A2P_NORMALIZE_PEAK (two floats);
 *  - return value: 0 = ok, negative = A2P_ERR_* (no exceptions cross the ABI);
 *    a2p_last_error() returns a static thread-local message;
 *  - inputs are borrowed for the duration of the enqueued work, outputs are
 *    caller-allocated (ownership rules of the reference: SURVEY.md §8b
 *    "Ownership / errors / threading").
 */
#ifndef A2P_HIP_H
#define A2P_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A2P_OK 0
#define A2P_ERR_ARG (-1)      /* bad argument / shape (reference: Python assert, gaussian_diffusion.py:286,318-322) */
#define A2P_ERR_STATE (-2)    /* call order: weights not finalized / conditioning not prepared */
#define A2P_ERR_HIP (-3)      /* HIP runtime error */
#define A2P_ERR_NOWEIGHT (-4) /* unknown / missing / mis-sized parameter (reference: load_model asserts, utils/model_util.py:30-38) */
#define A2P_ERR_NONFINITE (-5) /* a2p_check_finite: a denoiser output held inf / nan (16-bit operand overflow, or non-finite inputs / weights) */
#define A2P_ERR_NOCONVERGE (-6) /* a2p_eval_eigh: the Jacobi sweeps hit their cap */

#define A2P_FACE 0
#define A2P_POSE 1

#define A2P_PREC_F32 0  /* fp32 operands, v_mfma_f32_16x16x4_f32: the parity mode (<=1e-3 vs CPU reference) */
#define A2P_PREC_BF16 1 /* bf16 operands, fp32 accumulate/statistics/residual: the throughput mode      */

/* cond_drop_prob selector of FiLMTransformer.forward (model/diffusion.py:338-344);
 * A2P_PASS_CFG = ClassifierFreeSampleModel.forward (model/cfg_sampler.py:30-33). */
#define A2P_PASS_COND 0
#define A2P_PASS_UNCOND 1
#define A2P_PASS_CFG 2
/* Body model: audio and keyframes dropped separately.  Write e(K, A) for the output with the keyframe tokens kept (K) or replaced
 * by null_pose_embed, and the audio tokens + pooled hidden kept (A) or replaced by null_cond_embed / null_cond_hidden; a trained
 * checkpoint has seen all four (both conditions draw their own dropout mask, model/diffusion.py:325-328 and :366-369).
 *   A2P_PASS_KEYS      B sequences:  e(K, 0)
 *   A2P_PASS_CFG_AUDIO 2B sequences: e(K, 0) + scale * (e(K, A) - e(K, 0))
 *   A2P_PASS_CFG_DUAL  3B sequences: e(0, 0) + scale_keyframes * (e(K, 0) - e(0, 0)) + scale * (e(K, A) - e(K, 0));
 *                      scale_keyframes from a2p_set_guidance; needs 3 B <= 2 * max_batch. */
#define A2P_PASS_KEYS 3
#define A2P_PASS_CFG_AUDIO 4
#define A2P_PASS_CFG_DUAL 5
/* What the guided entry points (a2p_sample_step and its variants) evaluate: A2P_PASS_CFG, _CFG_AUDIO or _CFG_DUAL. */
#define A2P_GUIDE_JOINT 0
#define A2P_GUIDE_AUDIO 1
#define A2P_GUIDE_DUAL 2

#define A2P_SAMPLER_DDIM 0 /* GaussianDiffusion.ddim_sample (gaussian_diffusion.py:667-718) */
#define A2P_SAMPLER_DDPM 1 /* GaussianDiffusion.p_sample    (gaussian_diffusion.py:434-477, noise restored) */

typedef struct a2p_ctx a2p_ctx;

/* Constructor contract of FiLMTransformer (model/diffusion.py:83-99) as produced by
 * utils/model_util.py:49-76, plus the capacity the workspace is sized for. */
typedef struct a2p_config {
  int32_t data_format;      /* A2P_FACE | A2P_POSE                      */
  int32_t nfeats;           /* 256 | 104                                 */
  int32_t latent_dim;       /* 512 | 256   (must be 256 or 512)          */
  int32_t ff_size;          /* 1024                                      */
  int32_t num_layers;       /* 8 | 6                                     */
  int32_t num_heads;        /* 8   (latent_dim/num_heads must be 32|64)  */
  int32_t cond_feature_dim; /* 2038 | 1024                               */
  int32_t max_frames;       /* args.max_seq_length = 600                 */
  int32_t emb_len;          /* 1998 (model/diffusion.py:136)             */
  int32_t keyframe_dim;     /* 104                                       */
  int32_t keyframe_step;    /* 30                                        */
  int32_t precision;        /* A2P_PREC_*                                */
  int32_t max_batch;        /* largest B (samples) of any later call     */
  int32_t reserved;
} a2p_config;

/* ---- lifetime --------------------------------------------------------------- */
int a2p_ctx_create(const a2p_config* cfg, a2p_ctx** out);
int a2p_ctx_destroy(a2p_ctx* ctx);
const char* a2p_last_error(void);
const char* a2p_version(void);

/* ---- weights: nn.Module.load_state_dict (utils/model_util.py:30-38) ----------
 * `name` is the reference state_dict key (SURVEY.md §8b "Weights"), `data` a device
 * fp32 pointer of `numel` elements (copied).  Unknown names that belong to the
 * out-of-scope conditioning producers (audio_model.*, lip_model.*, *.rotary.freqs,
 * transformer.*, tokenizer.*) are accepted and ignored (returns 1). */
int a2p_set_weight(a2p_ctx* ctx, const char* name, const float* data, int64_t numel, void* stream);
/* Checks every hot-path parameter was provided, builds the packed compute-dtype
 * copies, rotary tables and the batch-invariant unconditional K/V caches. */
int a2p_finalize_weights(a2p_ctx* ctx, void* stream);

/* ---- hoisted conditioning (t-independent part of FiLMTransformer.forward,
 *      model/diffusion.py:360-381 + the audio-token K/V of every decoder layer) ----
 * cond_embed : [B, n_tok, cond_feature_dim]  = what encode_audio/encode_lip return
 *              (model/diffusion.py:355-358); n_tok = 1998 for 600 frames, 798 for 240.
 * keyframes  : pose only, [B, n_key, keyframe_dim]   (y["keyframes"])
 * key_mask   : pose only, uint8 [B, n_key], 1 = known (y["mask"][..., ::step]); NULL = all known
 * frames     : T of the motion sequence that will be denoised. */
int a2p_prepare_cond(a2p_ctx* ctx, const float* cond_embed, int32_t batch, int32_t n_tok,
                     const float* keyframes, const uint8_t* key_mask, int32_t n_key,
                     int32_t frames, void* stream);

/* ---- one denoiser evaluation -------------------------------------------------
 * FiLMTransformer.forward / ClassifierFreeSampleModel.forward.
 * x [B, nfeats, 1, T] ; t_orig int64 [B] (already mapped to 0..999, respace.py:140-145);
 * scale fp32 [B] (y["scale"], A2P_PASS_CFG only) ; out [B, T, nfeats]. */
int a2p_denoise_forward(a2p_ctx* ctx, const float* x, const int64_t* t_orig, const float* scale,
                        int32_t pass, float* out, void* stream);

/* ---- guiding audio and keyframes separately (body model) ----------------------
 * Selects what every following guided call evaluates (a2p_sample_step and its inpaint / windowed / multistep variants), until
 * it is called again: mode A2P_GUIDE_JOINT (the default: A2P_PASS_CFG), A2P_GUIDE_AUDIO or A2P_GUIDE_DUAL.  scale_keyframes
 * fp32 [B] on the device is read by every A2P_PASS_CFG_DUAL evaluation, a2p_denoise_forward's included, and stays owned by the
 * caller; the other modes ignore it.  The face model takes A2P_GUIDE_JOINT only.  The three-way combine runs as one kernel
 * behind the forward and leaves the guided output in both sequence blocks the step tails read, so their arithmetic is that of
 * A2P_GUIDE_JOINT: scale * (g - g) + g. */
int a2p_set_guidance(a2p_ctx* ctx, int32_t mode, const float* scale_keyframes);

/* ---- fused sampler step: p_mean_variance + ddim_sample / p_sample -------------
 * tables: fp32 [A2P_NTAB, n_steps] rows in the order of a2p_table_id, built by the host
 * from the float64 schedule exactly as _extract_into_tensor does (.float());
 * t_idx int64 [B]: step index into the (respaced) chain; timestep_map int64 [n_steps].
 * noise may be NULL for DDIM with eta == 0.  Outputs: x_next, pred_xstart, both
 * [B, nfeats, 1, T] (x_next may alias x). */
enum a2p_table_id {
  A2P_TAB_POST_COEF1 = 0,
  A2P_TAB_POST_COEF2,
  A2P_TAB_POST_VAR,
  A2P_TAB_POST_LOGVAR,
  A2P_TAB_SQRT_RECIP_ACP,
  A2P_TAB_SQRT_RECIPM1_ACP,
  A2P_TAB_ACP,
  A2P_TAB_ACP_PREV,
  A2P_TAB_SQRT_ACP,
  A2P_TAB_SQRT_1M_ACP,
  A2P_TAB_ACP_NEXT,
  A2P_NTAB
};
int a2p_sample_step(a2p_ctx* ctx, int32_t sampler, const float* x, const int64_t* t_idx,
                    const int64_t* timestep_map, const float* tables, int32_t n_steps,
                    const float* scale, const float* noise, float eta, int32_t clip_denoised,
                    float* x_next, float* pred_xstart, void* stream);

/* ---- sampling with held elements: inpainting and clip continuation (sample/inpaint.py) -----
 * a2p_sample_step with MDM's x0 replacement.  known fp32 and known_mask uint8 are [B, nfeats, 1, T] in x's layout (x's
 * normalised space); both are required.  Per element: the guided output g = u + scale[b] * (a - u) (non-finite g ORs the
 * a2p_check_finite flag, held or not), x0 = g clamped to [-1, 1] when clip_denoised, x0 = known where known_mask != 0 (not
 * clamped; a non-finite held value ORs the flag too), pred_xstart = x0, then the DDIM / DDPM update of a2p_sample_step with the
 * same noise layout.  An all-zero mask gives a2p_sample_step's bits.  x_next may alias x. */
int a2p_sample_step_inpaint(a2p_ctx* ctx, int32_t sampler, const float* x, const int64_t* t_idx,
                            const int64_t* timestep_map, const float* tables, int32_t n_steps,
                            const float* scale, const float* noise, float eta, int32_t clip_denoised,
                            const float* known, const uint8_t* known_mask, float* x_next, float* pred_xstart, void* stream);

/* ---- windowed joint sampling of recordings longer than one window (sample/long_form.py) -----
 * W windows of T_w = the prepared frames start at win_starts_host[W] (HOST int32: ascending, the first at 0, the last ending at
 * T_total, no gaps; W <= A2P_WINDOW_MAX).  The prepared batch is R * W sequences, b = r * W + w: x_win, x_next_win, x0_win are
 * [R*W, nfeats, 1, T_w], t_idx [R*W], scale [R*W].  One step: the a2p_sample_step forward, then for every global frame the
 * guided x0 predictions of the covering windows are blended with win_weights fp32 [W, T_w] in ascending w, clamped when
 * clip_denoised, and the DDIM / DDPM update is computed once from the blend (x from the first covering window, noise_global
 * [R, nfeats, 1, T_total] or NULL for DDIM with eta == 0).  The same bits are written to every window copy of the frame and,
 * when non-NULL, to x_global / x0_global [R, nfeats, 1, T_total].  x_next_win may alias x_win. */
#define A2P_WINDOW_MAX 256
int a2p_sample_step_windowed(a2p_ctx* ctx, int32_t sampler, const float* x_win, const int64_t* t_idx,
                             const int64_t* timestep_map, const float* tables, int32_t n_steps, const float* scale,
                             const float* noise_global, float eta, int32_t clip_denoised, const int32_t* win_starts_host,
                             const float* win_weights, int32_t W, int32_t T_total, float* x_next_win, float* x0_win,
                             float* x_global, float* x0_global, void* stream);

/* ---- DPM-Solver++(2M): multistep sampling in fewer steps (GaussianDiffusion.dpm_solver_sample_loop) -----
 * coefs fp32 [A2P_NMS, n_steps] rows in the order of a2p_ms_coef_id, built by the host in float64 and cast
 * (GaussianDiffusion.multistep_table).  Per element, after the guided output g = u + scale[b] * (a - u) (non-finite g ORs the
 * a2p_check_finite flag), x0 = g clamped to [-1, 1] when clip_denoised, and x0 = known where known_mask != 0 (a2p_sample_step_inpaint's
 * rule): pred_xstart = x0 and, with t = t_idx[b],
 *   t == 0            x_next = x0
 *   x0_prev == NULL   x_next = fmaf(CX[t], x, B1[t] * x0)
 *   otherwise         x_next = fmaf(CX[t], x, fmaf(B2[t], x0, P2[t] * x0_prev))
 * x0_prev [B, nfeats, 1, T] is the previous step's pred_xstart (NULL on the first step of a call).  known and known_mask are both
 * NULL (plain step) or both set ([B, nfeats, 1, T] fp32 / uint8).  x_next may alias x; pred_xstart must not alias x0_prev
 * (A2P_ERR_ARG). */
enum a2p_ms_coef_id { A2P_MS_CX = 0, A2P_MS_B1, A2P_MS_B2, A2P_MS_P2, A2P_NMS };
int a2p_sample_step_multistep(a2p_ctx* ctx, const float* x, const int64_t* t_idx, const int64_t* timestep_map, int32_t n_steps,
                              const float* scale, const float* coefs, const float* x0_prev, int32_t clip_denoised,
                              const float* known, const uint8_t* known_mask, float* x_next, float* pred_xstart, void* stream);
/* The windowed form (a2p_sample_step_windowed's windows, blend and outputs): the update above is computed once per global frame
 * from the blended x0, with x and x0_prev_win [R*W, nfeats, 1, T_w] (or NULL) read from the first covering window; the same
 * bits go to every window copy and to x_global / x0_global when non-NULL.  x_next_win may alias x_win; x0_win and x0_global
 * must not alias x0_prev_win (A2P_ERR_ARG). */
int a2p_sample_step_windowed_multistep(a2p_ctx* ctx, const float* x_win, const int64_t* t_idx, const int64_t* timestep_map,
                                       int32_t n_steps, const float* scale, const float* coefs, const float* x0_prev_win,
                                       int32_t clip_denoised, const int32_t* win_starts_host, const float* win_weights, int32_t W,
                                       int32_t T_total, float* x_next_win, float* x0_win, float* x_global, float* x0_global,
                                       void* stream);
/* Windows of a per-frame signal: channels last, src [reps, T_total * k, ch] -> dst [reps * W, T_w * k, ch] (k samples of ch
 * channels per frame, e.g. the dual audio: k = 1600, ch = 2); channels_first (k = 1), src [reps, ch, T_total] -> dst
 * [reps * W, ch, T_w].  dst[r * W + w] is the slice of src[r] from frame win_starts_host[w] (same rules as above). */
int a2p_window_gather(const float* src, int32_t reps, int32_t T_total, int32_t k, int32_t ch, int32_t channels_first,
                      const int32_t* win_starts_host, int32_t W, int32_t T_w, float* dst, void* stream);

/* ---- stand-alone sampler arithmetic (any model callable on the host side) ------
 * model_out [B, T, C] -> pred_xstart/mean [B, C, 1, T]: GaussianDiffusion.p_mean_variance
 * (gaussian_diffusion.py:305-316) + q_posterior_mean_variance (:235-257). */
int a2p_p_mean_variance(const float* model_out, const float* x, const int64_t* t_idx, const float* tables,
                        int32_t n_steps, int32_t batch, int32_t nfeats, int32_t frames, int32_t clip_denoised,
                        float* pred_xstart, float* mean, void* stream);
/* ddim_sample update (gaussian_diffusion.py:699-717) from pred_xstart. */
int a2p_ddim_update(const float* pred_xstart, const float* x, const int64_t* t_idx, const float* tables,
                    int32_t n_steps, const float* noise, float eta, int32_t batch, int64_t per_sample,
                    float* sample, void* stream);
/* DPM-Solver++(2M) update of a2p_sample_step_multistep from pred_xstart (x, pred_xstart, x0_prev, sample all
 * [batch, per_sample]; x0_prev NULL: first order).  sample may alias x; pred_xstart must not alias x0_prev (A2P_ERR_ARG). */
int a2p_multistep_update(const float* x, const float* pred_xstart, const float* x0_prev, const int64_t* t_idx,
                         const float* coefs, int32_t n_steps, int32_t batch, int64_t per_sample, float* sample, void* stream);
/* p_sample update (gaussian_diffusion.py:470-476): mean + [t!=0] exp(.5 logvar) noise. */
int a2p_p_sample_update(const float* mean, const int64_t* t_idx, const float* tables, int32_t n_steps,
                        const float* noise, int32_t batch, int64_t per_sample, float* sample, void* stream);
/* _predict_eps_from_xstart (gaussian_diffusion.py:347-351). */
int a2p_eps_from_xstart(const float* x, const float* pred_xstart, const int64_t* t_idx, const float* tables,
                        int32_t n_steps, int32_t batch, int64_t per_sample, float* eps, void* stream);
/* plms_sample arithmetic (gaussian_diffusion.py:990-1041).  eps0 is the newest eps, eps1..3 older ones (NULL when the mode
 * does not read them).  PREDICT writes the Euler predictor x0 sqrt(abar_prev) + sqrt(1-abar_prev) eps0 that the
 * reference feeds to the model at t-1; AB1..AB4 / EULER write the step's "sample" (pred_xstart where t == 0). */
enum a2p_plms_mode { A2P_PLMS_PREDICT = 0, A2P_PLMS_AB1, A2P_PLMS_AB2, A2P_PLMS_AB3, A2P_PLMS_AB4, A2P_PLMS_EULER };
int a2p_plms_update(const float* x, const float* pred_xstart, const int64_t* t_idx, const float* tables, int32_t n_steps,
                    const float* eps0, const float* eps1, const float* eps2, const float* eps3, int32_t mode,
                    int32_t batch, int64_t per_sample, float* sample, void* stream);
/* ddim_reverse_sample update, eta = 0 (gaussian_diffusion.py:781-813). */
int a2p_ddim_reverse_update(const float* pred_xstart, const float* x, const int64_t* t_idx, const float* tables,
                            int32_t n_steps, int32_t batch, int64_t per_sample, float* sample, void* stream);
/* q_sample (gaussian_diffusion.py:215-233). */
int a2p_q_sample(const float* x_start, const int64_t* t_idx, const float* tables, int32_t n_steps,
                 const float* noise, int32_t batch, int64_t per_sample, float* out, void* stream);

/* ---- recording -> y["audio"] (demo/demo.py:156-189, generate_results; audio2photoreal_amd/audio.py) ----------
 * torchaudio.functional.resample (sinc_interp_hann / sinc_interp_kaiser): in fp32 [batch, len, in_channels] (channels
 * interleaved and averaged to mono on the way in; in_channels = 1: [batch, len]) -> out fp32 [batch, ceil(n len / o)], with
 * o = orig_freq / g, n = new_freq / g, g = gcd.  table fp32 [n_phase = n, n_taps = 2 width + o]: the filter bank of
 * _get_sinc_resample_kernel, built by the caller.  out[b][m] = sum_j table[m mod n][j] xpad[(m div n) o + j], xpad = the mono
 * row with `width` zeros on the left.  orig_freq == new_freq: table may be NULL and out = the (averaged) input. */
#define A2P_RESAMPLE_MAX_TABLE_BYTES (16 << 20)
#define A2P_RESAMPLE_MAX_CHANNELS 64
int a2p_resample(const float* in, int32_t batch, int64_t len, int32_t in_channels, int32_t orig_freq, int32_t new_freq,
                 const float* table, int32_t n_phase, int32_t n_taps, int32_t width, float* out, void* stream);
/* The demo's dual audio from the resampled mono signal mono fp32 [len] (already cut to whole 4 s blocks):
 * peak = max(mono) (A2P_ERR_ARG when it is not > 0: silent input), then for every repetition r < reps
 *   out[r][i][0] = float(((double)(mono[i] / peak) - mean0) / std_flat),  out[r][i][1] = float((noise[i][1] - mean1) / std_flat)
 * with noise fp64 [len, 2] (the caller's N(0, 0.001) draws); out fp32 [reps, len, 2].  peak_scratch: A2P_DUAL_AUDIO_SCRATCH
 * floats of device memory.  Synchronises `stream` once, to read the peak. */
#define A2P_DUAL_AUDIO_SCRATCH 257
int a2p_dual_audio(const float* mono, int64_t len, float* peak_scratch, const double* noise, double mean0, double mean1,
                   double std_flat, int32_t reps, float* out, void* stream);
/* Conversations (sample/conversation.py; the dataset's two-channel audio, data_loaders/get_data.py:79-92, 83-88 flip_person).
 * a2p_resample_channels: a2p_resample of every channel on its own: in fp32 [len, channels] interleaved -> out fp32 planar
 * [channels, ceil(n len / o)]; row c is bit-identical to a2p_resample (batch 1, in_channels 1) of channel c extracted as a mono
 * row.  Same table rules; orig_freq == new_freq: table may be NULL and the channels are copied. */
int a2p_resample_channels(const float* in, int64_t len, int32_t channels, int32_t orig_freq, int32_t new_freq,
                          const float* table, int32_t n_phase, int32_t n_taps, int32_t width, float* out, void* stream);
/* a2p_conversation_audio: y["audio"] of both people of a two-channel recording.  channels fp32 planar [2, ld] (channel k = person
 * k's microphone), of which the first len samples are used.  Person p's own voice is channel p, the partner's channel 1 - p:
 *   u_k = channels[k][i] / peak_k (float32; peak_k = max over [0, len) of channel k)  under A2P_NORMALIZE_PEAK,
 *   u_k = channels[k][i]                                                                under A2P_NORMALIZE_NONE,
 *   out[p * reps + r][i] = (float((u_p - mean0_p) / std_p), float((u_{1-p} - mean1_p) / std_p))   (float64 arithmetic)
 * for every person p in the bitmask `people` (bit p) and repetition r < reps; the rows of a person outside `people` are not
 * written.  out fp32 [2 reps, len, 2].  stats_host: fp64 [2][3] = (mean0_p, mean1_p, std_p) on the host.  Under
 * A2P_NORMALIZE_PEAK peak_scratch holds A2P_CONVERSATION_SCRATCH floats of device memory, a channel whose peak is not > 0 or not
 * finite is refused with A2P_ERR_ARG, and `stream` is synchronised once to read the two peaks back. */
#define A2P_NORMALIZE_NONE 0
#define A2P_NORMALIZE_PEAK 1
#define A2P_CONVERSATION_SCRATCH 514
int a2p_conversation_audio(const float* channels, int64_t ld, int64_t len, int32_t normalize, float* peak_scratch, int32_t people,
                           const double* stats_host, int32_t reps, float* out, void* stream);

/* ---- unit entry points (parity tests of single kernels / one decoder layer) -----
 * FiLMTransformerDecoderLayer.forward (model/modules/transformer_modules.py:178-217):
 * x [N, T, d] updated in place; memory [N, S, d]; t [N, d]; memory2 [N, S2, d] or NULL.
 * Uses the weights of decoder layer `layer`. */
int a2p_decoder_layer_forward(a2p_ctx* ctx, int32_t layer, float* x, const float* memory, const float* t,
                              const float* memory2, int32_t nseq, int32_t frames, int32_t mem_len,
                              int32_t mem2_len, void* stream);
/* C[M,N] = A[M,K] W[N,K]^T + bias on the MFMA GEMM kernel of the context's precision. */
int a2p_gemm(a2p_ctx* ctx, const float* A, const float* W, const float* bias, float* C, int32_t M, int32_t N,
             int32_t K, void* stream);
/* Test-only (never on the product path): ONE launch of the GEMM dispatcher with every epilogue field in the caller's hands, so that
 * each kernel instance and epilogue can be compared with a float64 restatement on its own (tests/test_gemm_family_hip.py).
 *   acc[m][n] = sum over tap < ntaps, k < K of A[m + tap * a_tap_rows][k] * W[tap][n][k]   (+ bias[n])
 * A fp32 [a_rows, K], W fp32 [ntaps, N, K], skip fp32 [M, K] (columns < N are read), all dense.  The operands are cast to the
 * context's type exactly as the forwards cast them, K zero-padded to the k-step (32 fp32 / 64 16-bit); split != 0 (16-bit modes):
 * as split-operand rows A' = [hi | lo | hi], W' = [hi | hi | lo] instead.  epi / act: the kernels' EPI_* (0 store, 1 transposed
 * store, 2 FiLM residual, 3 conv) and ACT_* (0 none, 1 GELU, 4 LeakyReLU(0.2), 5 ReLU) values; a combination without a kernel
 * instance is A2P_ERR_ARG.
 *   store / conv:      out[out_off + (m + (m / rows_per_seq) * out_seq_pad) * ldo + n]; split_third > 0: the 16-bit row is
 *                      [hi | lo | hi] with the pieces split_third elements apart; dup_off > 0 (out_f32): a second copy dup_off further
 *   transposed store:  out[out_off + (m / rows_per_seq) * t_seq_stride + n * ldo + m % rows_per_seq]
 *   FiLM residual:     resid[m * ldx + n] += (film[seq * film_seq_stride + n] + 1) * acc + film[seq * film_seq_stride + film_shift_off + n]
 *                      (film NULL: += acc), seq = m / rows_per_seq; resid points at row 0 and resid_elems floats are addressable from it
 * out is the fp32 image of the WHOLE output buffer (out_elems elements, guard rows included).  A 16-bit store (16-bit mode,
 * out_f32 == 0) narrows the image to the 16-bit type, runs on that buffer and widens all of it back, so a value the kernel did
 * not write returns as it was when the 16-bit type holds it exactly.  ran_host (host memory, may be NULL) receives the
 * gemm_kernel instance the dispatcher chose: {element bits, MT, NB}.  Shapes whose write set would leave a buffer are
 * A2P_ERR_ARG and nothing is launched.  Synchronises `stream`. */
typedef struct a2p_gemm_case {
  const float* A;
  const float* W;
  const float* bias;
  float* out;
  float* resid;
  const float* film;
  const float* skip;
  int32_t* ran_host;
  int64_t a_rows, out_elems, out_off, ldo, t_seq_stride, ldx, resid_elems, film_elems, film_seq_stride, dup_off;
  int32_t M, N, K, ntaps, a_tap_rows, epi, act, out_f32, rows_per_seq, out_seq_pad, film_shift_off, split, split_third, reserved;
} a2p_gemm_case;
int a2p_gemm_ex(a2p_ctx* ctx, const a2p_gemm_case* gemm_case, void* stream);
/* Test-only: out[M, N] = act(A[M, K] W[N, K]^T + bias) on the skinny fp32 GEMM of the per-step time path; fp32 device rows with row
 * strides lda / ldw / ldo, K % 64 == 0, N % 16 == 0, bias may be NULL.  ncases == 1: launch_skinny (64 rows per launch);
 * ncases == 3: the grouped launch of three independent cases (one kernel when every M <= 64, three single launches otherwise).
 * Synchronises `stream`. */
typedef struct a2p_skinny_case {
  const float* A;
  const float* W;
  const float* bias;
  float* out;
  int64_t lda, ldw, ldo;
  int32_t M, N, K, act;
} a2p_skinny_case;
int a2p_skinny_gemm_ex(a2p_ctx* ctx, const a2p_skinny_case* cases, int32_t ncases, void* stream);
/* softmax(q k^T / sqrt(dh)) v per head; q [N, Tq, d], k/v [N, S, d], out [N, Tq, d]. */
int a2p_attention(a2p_ctx* ctx, const float* q, const float* k, const float* v, float* out, int32_t nseq,
                  int32_t tq, int32_t s, void* stream);
/* Test-only (never on the product path): ONE launch of the attention dispatcher with every field of the kernels' parameter block in
 * the caller's hands, so that each kernel instance can be compared with a float64 restatement on its own
 * (tests/test_attention_family_hip.py).  d = latent_dim, dh = d / num_heads, S = S_main + S_tail, Sp = S rounded up to 64:
 *   out[out_off + seq * o_seq_stride + t * ldo + h * dh + c] = sum_j softmax_j(q . k_j / sqrt(dh)) v_j[c]      t < Tq
 *   q   = qbuf[q_off + seq * q_seq_stride + t * ldq + h * dh ..]
 *   k_j = kbuf[k_off + slot * k_slot_stride + j * ldk + h * dh ..]                                             j < S_main
 *   v_j[c] = vt[vt_off + slot * vt_slot_stride + (h * dh + c) * ldvt + j]
 *   k_j, v_j = ktail / vtail[(seq % tail_mod) * tail_sample_stride + (j - S_main) * tail_row_stride + h * dh ..]   S_main <= j < S
 *   slot = slot_rule 1: 1 + seq;  2: 0;  3: seq < slot_b ? 1 + seq : 0;  0: kv_slot_host[seq], or seq when that is NULL
 * qbuf, kbuf (NULL: K lives in qbuf, the self-attention layout [T][Q | K]), vt and out are fp32 device images of the WHOLE buffers
 * (guard rows, padding rows and columns included; q_elems .. out_elems elements).  In a 16-bit mode every image is narrowed to the
 * 16-bit type before the launch -- a NaN or sentinel in padding reaches the kernel as it is -- and all of out is widened back after
 * it.  ktail / vtail stay fp32 (the kernels read them as fp32; tail_elems elements each).  kv_slot_host is a HOST array of nseq
 * slots.  Every K and V^T slot must hold Sp keys (the kernels move whole 64-key tiles), nslots of them lie in the buffers.
 * ksplit / nseq_rule: launch_attn's arguments of the same name.  kv_stream: the non-temporal policy of the K/V tile loads.
 * ran_host (host memory, may be NULL) receives the dispatcher's decision: {kernel (0 attn_kernel, 1 attn_ksplit_kernel, 2 unused,
 * 3 attn3_kernel), operand bits, head_dim, waves per workgroup, 16-query tiles per wave, query blocks per (sequence, head), workgroups,
 * xcd_remap}.  The context's logit-maximum slot is reset in front of the launch: a2p_attention_logit_max afterwards returns this
 * launch's maximum.  A case whose reads or writes would leave a buffer, whose slots or output sequences overlap, or which breaks an
 * alignment the kernels rely on is A2P_ERR_ARG and nothing is launched.  Synchronises `stream`. */
typedef struct a2p_attention_case {
  const float* qbuf;
  const float* kbuf;
  const float* vt;
  float* out;
  const float* ktail;
  const float* vtail;
  const int32_t* kv_slot_host;
  int32_t* ran_host;
  int64_t q_elems, k_elems, vt_elems, out_elems, tail_elems;
  int64_t q_off, k_off, vt_off, out_off;
  int64_t q_seq_stride, ldq, k_slot_stride, ldk, vt_slot_stride, ldvt, o_seq_stride, ldo, tail_sample_stride, tail_row_stride;
  int32_t nseq, Tq, S_main, S_tail, nslots, slot_rule, slot_b, tail_mod, kv_stream, ksplit, nseq_rule, reserved;
} a2p_attention_case;
int a2p_attention_ex(a2p_ctx* ctx, const a2p_attention_case* attention_case, void* stream);

/* ---- measurement (bench.py roofline leg) ----------------------------------------
 * When enabled, every launch of the kernel class `kind` is bracketed by hipEvents on
 * the launch stream; a2p_kernel_time_ms synchronises and returns total ms and count. */
#define A2P_KERNEL_GEMM 0
#define A2P_KERNEL_ATTN_SELF 1
#define A2P_KERNEL_ATTN_CROSS 2
#define A2P_KERNEL_LNROPE 3
#define A2P_KERNEL_CHAIN 4 /* fused row-panel chain kernels (projections + FiLM + LayerNorm + FFN), bf16 mode */
/* finer classes of the launches above (a launch is timed when its class OR its sub-class is selected) */
#define A2P_KERNEL_CHAIN_PRE 5     /* norm1 -> rotary -> [Q|K], V^T (first layer only; later layers: tail of POST) */
#define A2P_KERNEL_CHAIN_MID 6     /* out_proj -> FiLM + residual -> LayerNorm -> rotary -> Q */
#define A2P_KERNEL_CHAIN_POST 7    /* out_proj -> FiLM -> norm3 -> FFN -> FiLM [-> next layer's PRE work | final_layer] */
#define A2P_KERNEL_CHAIN_MIDPOST 8 /* body model: MID2 | keyframe attention | POST in one launch */
#define A2P_KERNEL_POSE_TAIL 9     /* body model: final_layer + 6 dilated convs + final_conv (a sub-class of A2P_KERNEL_GEMM) */
#define A2P_KERNEL_GUIDE_COMBINE 10 /* body model: the combine behind an A2P_PASS_CFG_AUDIO / _CFG_DUAL forward */
int a2p_kernel_timing(a2p_ctx* ctx, int32_t kind, int32_t enable);
int a2p_kernel_time_ms(a2p_ctx* ctx, double* total_ms, int64_t* launches);

/* ---- sample-parallel runs: the kernel family and attention kernel a forward takes depend on its size, and both choices differ in
 * operand rounding: fused row-panel chains for large forwards, small-tile GEMMs for small ones (row count); attn3_kernel or
 * attn_kernel (sequence count).  A rank that denoises a BLOCK of a larger batch names the size of the whole batch here, so that
 * every shard takes the kernel family and attention kernel the unsharded run takes -- in the denoiser forwards and the face model's
 * cond encoder (a2p_prepare_cond) -- and the gathered samples equal the single-process samples bit for bit (sample_parallel.py does
 * this; 0 = no hint: every choice follows the local batch).  Only the decisions follow the hint; grids stay local.  Entry points
 * called directly (a2p_attention, a2p_decoder_layer_forward, the audio front end) ignore it. */
int a2p_set_batch_hint(a2p_ctx* ctx, int32_t global_batch);

/* ---- non-finite detection ------------------------------------------------------
 * The 16-bit throughput modes stage Q|K|V, the FFN hidden activation and the split-operand rows as IEEE half (liba2p_hip_f16.so:
 * |x| <= 65504) or bfloat16; a checkpoint whose activations leave that range produces inf / nan, which the reference's fp32 path
 * would not.  Every denoiser evaluation (a2p_denoise_forward, a2p_sample_step) ORs "the model output held a non-finite value"
 * into a device flag of the context at no measurable cost (the fused step tail reads every output element anyway).
 * a2p_check_finite synchronises `stream`, reads and CLEARS the flag: returns 0 when every evaluation since the last check was
 * finite, A2P_ERR_NONFINITE otherwise (a2p_last_error names the remedy: precision "bf16" for range, "fp32" for parity mode).
 * The Python loops (GaussianDiffusion.*_sample_loop) call it once per sampling call and raise A2PError; the reference has no
 * counterpart (its torch CPU / CUDA fp32 path cannot overflow on these models). */
int a2p_check_finite(a2p_ctx* ctx, void* stream);

/* ---- validity envelope of the 16-bit modes ----------------------------------------
 * The largest row maximum of the scaled attention scores q.k / sqrt(head_dim) that any self- or cross-attention query of the
 * denoiser saw since the last call (synchronises `stream`, then resets; -inf when no attention ran).  The operand rounding of the
 * 16-bit modes becomes a logit error proportional to the logits' magnitude, and softmax turns logit errors into probability
 * errors one for one: measured on the CPU model of the rounding sites and on the GPU (profiles/r04_trained_like_budget.json,
 * tests/test_hip_round4.py), IEEE-half operands hold <= 1e-3 on the loop's return value up to a maximum of ~13-15 and reach
 * 2.4e-3 at ~29; bfloat16 is 8x worse throughout.  The Python model mirror warns (A2PPrecisionWarning) above 20 in the 16-bit
 * modes; precision="fp32" is the answer there.  No reference counterpart (its path is fp32). */
int a2p_attention_logit_max(a2p_ctx* ctx, float* max_logit_host, void* stream);
/* The same read-and-reset, plus the library's own verdict: *outside = 1 when the context computes on 16-bit operands AND the maximum
 * exceeds A2P_LOGIT_ENVELOPE_16BIT -- the caller should re-create the context with precision A2P_PREC_F32 (exact at any magnitude:
 * 1e-6..5e-6 on the same scenarios) and repeat the sampling call.  The Python mirror does exactly that, once and for good per model
 * (FiLMTransformer.check_finite: "escalation", sticky; GaussianDiffusion's loops check after the first step and at the end of a call
 * and re-run a call that ended outside).  fp32 contexts always report 0. */
#define A2P_LOGIT_ENVELOPE_16BIT 20.0f
int a2p_precision_verdict(a2p_ctx* ctx, float* max_logit_host, int32_t* outside, void* stream);

/* ---- run-time switches: the A2P_* environment variables that steer a forward (INTEGRATION.md "Environment switches") are read
 * when the context is created; a host that changes one afterwards calls this (the Python mirror does, model/diffusion.py). */
int a2p_reload_env(a2p_ctx* ctx);

/* ---- debugging aid: copies an internal buffer ("film", "ktail", "vtail", "tvec", "x", "qk", "vt", "ao", "mo") to host
 * memory after a device synchronise (race hunts, scratch/stress*.py); not part of the reference's interface. */
int a2p_debug_read(a2p_ctx* ctx, const char* name, void* host, int64_t bytes);

/* ---- guide transformer + residual-VQ decode --------------------------------------
 * GuideTransformer (model/guide.py:26-83) predicts the body model's keyframe tokens from the audio features;
 * TemporalVertexCodec.decode (model/vqvae.py:508-521) turns them into the `keyframes` the pose denoiser consumes
 * (sample/generate.py:51-71 `_replace_keyframes`).  fp32 throughout.  Parameter names are the reference's state_dict keys
 * (`audio_model.*` and `*.rotary.freqs` are accepted and ignored). */
typedef struct a2p_guide_ctx a2p_guide_ctx;
typedef struct a2p_guide_config {
  int32_t tokens;           /* codebook size; id `tokens` is the sequence-start token (model/guide.py:42-45) */
  int32_t dim, num_layers, num_heads, ff_size;
  int32_t cond_feature_dim; /* audio feature width (1024) */
  int32_t emb_len;          /* rows of null_cond_embed (1998) = upper bound of the audio tokens left after the conv stack */
  int32_t num_audio_layers; /* blocks of 6 dilated convs in `pre_audio` (model/guide.py:84-109) */
  int32_t max_batch;
  int32_t max_positions;    /* longest token prefix incl. the start token (self-attention cache depth) */
  int32_t reserved[2];
} a2p_guide_config;
int a2p_guide_create(const a2p_guide_config* cfg, a2p_guide_ctx** out);
int a2p_guide_destroy(a2p_guide_ctx* ctx);
int a2p_guide_set_weight(a2p_guide_ctx* ctx, const char* name, const float* dev_ptr, int64_t numel, void* stream);
int a2p_guide_finalize(a2p_guide_ctx* ctx, void* stream);
/* Token-independent part of GuideTransformer.forward (model/guide.py:150-169), hoisted out of the 80-step loop of
 * `generate`: pre_audio conv stack, cond projection, pooled FiLM vector, norm_cond, per-layer cross-attention K/V.
 * cond_embed [batch, n_tokens, cond_feature_dim] fp32 = what encode_audio returns (:111-119); cond_drop 0|1 selects the
 * null embeddings (:156-165). */
int a2p_guide_prepare(a2p_guide_ctx* ctx, const float* cond_embed, int32_t batch, int32_t n_tokens, int32_t cond_drop,
                      void* stream);
/* GuideTransformer.forward on the prepared condition: tokens int64 [batch, len] (causal) -> logits fp32 [batch, len, tokens]. */
int a2p_guide_forward(a2p_guide_ctx* ctx, const int64_t* tokens, int32_t batch, int32_t len, float* logits, void* stream);
/* GuideTransformer.generate (model/guide.py:175-222) as one persistent launch: n_steps tokens per sequence by nucleus
 * sampling (top_p); the categorical draw of step i, sequence b is the inverse CDF at uniforms[i * batch + b] in [0, 1).
 * tokens_out int64 [batch, n_steps]; sorted_probs_out (nullable) fp32 [n_steps, batch, tokens] = the renormalised sorted
 * nucleus probabilities the reference hands to Categorical (:212-214). */
int a2p_guide_generate(a2p_guide_ctx* ctx, int32_t batch, int32_t n_steps, float top_p, const float* uniforms,
                       int64_t* tokens_out, float* sorted_probs_out, void* stream);
/* a2p_guide_generate with positions whose token is given: forced int64 [batch, n_steps], -1 = draw, a value in [0, tokens) =
 * that position's token.  A forced position runs the decoder stack (its self-attention K/V cache rows are written as for a
 * drawn token), skips the softmax, sort and draw, writes its token to tokens_out, feeds it to the next position and zero-fills
 * its sorted_probs_out row.  A free position still reads uniforms[i * batch + b].  Any other value is never looked up: the
 * sequence writes -2 at that position and stops there.  forced == NULL is a2p_guide_generate. */
int a2p_guide_generate_forced(a2p_guide_ctx* ctx, int32_t batch, int32_t n_steps, float top_p, const float* uniforms,
                              const int64_t* forced, int64_t* tokens_out, float* sorted_probs_out, void* stream);
/* test / diagnostics: copy a prepared buffer ("pre_audio", "ct", "mem", "memr", "hidden", "film", "kc", "vc") to the host */
int a2p_guide_debug_read(a2p_guide_ctx* ctx, const char* name, void* host, int64_t bytes);
/* TemporalVertexCodec.decode: q int64 [batch, T, depth] -> out fp32 [batch, T, vertices].  codebooks: `depth` device
 * pointers [categories, latent] (quantizer.layers.i._codebook.embed); conv_w / conv_b: the 5 Conv1d of decoder.dec
 * (indices 0,2,4,6: [latent, latent, 2], dilation 1,2,3,1; index 8: [vertices, latent, 1]).  The pointer arrays are host memory. */
int a2p_vq_decode(const int64_t* q, int32_t batch, int32_t T, int32_t depth, int32_t categories, int32_t latent,
                  int32_t vertices, const float* const* codebooks, const float* const* conv_w, const float* const* conv_b,
                  float* out, void* stream);
/* TemporalVertexCodec.encode (model/vqvae.py:499-506): poses fp32 [batch, T, vertices] (keyframe-rate rows, normalised) ->
 * tokens_out int64 [batch, T, depth] and / or latents_out fp32 [batch, T, latent] (the encoder's output; either may be NULL, not
 * both).  Encoder: 7 zero rows of left padding, encoder.enc.0 (Conv1d vertices -> latent, k=1), LeakyReLU(0.2), enc.{2,4,6,8}
 * (Conv1d latent -> latent, k=2, dilation 1,2,3,1) with LeakyReLU between them and none after the last.  Residual quantisation:
 * per level idx = argmax(-(|x|^2 - 2 x.embed + |embed|^2)) in fp32, lowest index on an exact tie, then x -= embed[idx].
 * code_norms: `depth` device pointers [categories] holding |embed|^2.  The pointer arrays are host memory.  A2P_ERR_ARG when
 * 2 (T + 7) latent floats exceed 64 KB of LDS (T <= 121 at latent 64) or latent is not a multiple of 4. */
int a2p_vq_encode(const float* poses, int32_t batch, int32_t T, int32_t depth, int32_t categories, int32_t latent,
                  int32_t vertices, const float* const* codebooks, const float* const* code_norms, const float* const* conv_w,
                  const float* const* conv_b, int64_t* tokens_out, float* latents_out, void* stream);

/* ---- tokenizer training (train/train_vq.py ModelTrainer.run_train_step) ---------------------------------------------
 * One fused step of TemporalVertexCodec in training mode: forward, SmoothL1 losses (mean reduction, beta 1; the "velocity" term
 * differences the CHANNEL axis, as the reference does), backward through decoder, straight-through residual VQ (only level 0
 * carries commitment gradient) and encoder, AdamW (torch's single-tensor path, betas (0.9, 0.99), eps 1e-8) and the EMA codebook
 * update (cluster_size, embed_avg, embed = embed_avg / (laplace_smoothing(cluster_size) * cluster_size.sum())).  Every level
 * quantises with the books as they stood when the step began.  Dead-code expiry is not built: in the reference the EMA update
 * of the same forward overwrites what it writes.  fp32 state and activations (dot products accumulate in double and round once),
 * five launches whatever the shapes, no host synchronisation, no float
 * atomics: the same state and batch give the same bits.
 * params / exp_avg / exp_avg_sq: one flat fp32 buffer each, the tensors of TemporalVertexCodec.parameters() in order
 * (encoder.enc.{0,2,4,6,8}.{weight,bias}, decoder.project_mean_shape.{weight,bias}, decoder.dec.{0,2,4,6,8}.{weight,bias});
 * project_mean_shape never gets a gradient and is left untouched, moments included.  embed / embed_avg / cluster_size: `depth`
 * device pointers ([categories, latent] x2, [categories]); the pointer arrays are host memory.  All state is updated in place.
 * tokens_out int64 [batch, T, depth].  loss_record: 6 device floats the step ADDS to (loss, loss_motion, loss_commit, loss_vel,
 * perplexity of the last level, 1): zero it, run steps, read it when convenient.  grads_out: NULL or a flat buffer like params
 * that receives this step's gradient (the project_mean_shape range is not written).  workspace: 16-byte aligned device memory of
 * a2p_vq_train_workspace_bytes; it needs no initialisation.  Bounds as a2p_vq_encode; A2P_ERR_ARG, before any launch, when
 * 2 (T + 7) latent floats + 64 bytes exceed 64 KB of LDS (T <= 120 at latent 64). */
typedef struct a2p_vq_train_hyper {
  double lr, bias_correction1, bias_correction2;   /* 1 - beta^step of this step, as torch.optim.AdamW computes them */
  double weight_decay, commit, loss_vel;
  double ema_decay, ema_epsilon;                   /* the reference: 0.99, 1e-5 */
} a2p_vq_train_hyper;
int a2p_vq_train_workspace_bytes(int32_t batch, int32_t T, int32_t depth, int32_t categories, int32_t latent, int32_t vertices,
                                 int64_t* bytes_out);
int a2p_vq_train_step(const float* x, int32_t batch, int32_t T, int32_t depth, int32_t categories, int32_t latent,
                      int32_t vertices, float* params, float* exp_avg, float* exp_avg_sq, float* const* embed,
                      float* const* embed_avg, float* const* cluster_size, const a2p_vq_train_hyper* hyper, int64_t* tokens_out,
                      float* loss_record, float* grads_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- audio front end ------------------------------------------------------------------
 * What FiLMTransformer.forward computes from y["audio"] before anything else, in every step and pass (model/diffusion.py:
 * 354-358): encode_audio (:285-293, both stereo channels through the vq-wav2vec conv feature extractor of model/utils.py:18-26,
 * after torchaudio Resample(48000, 16000)) and, for the face model, encode_lip (:295-313: Audio2LipRegressionTransformer :37-79 =
 * Wav2VecEncoder (model/modules/audio_encoder.py:24-46) + RegressionTransformer (model/modules/transformer_modules.py:560-627)
 * + Linear, over 120-frame chunks; nearest-exact interpolation to the token count; concatenation).  Here it is one call per
 * clip.  fp32.  Parameter names are the reference's state_dict keys; the conv feature extractors take
 * `audio_model.feature_extractor.conv_layers.{i}.0.weight` / `lip_model.audio_encoder.wav2vec_model.feature_extractor.
 * conv_layers.{i}.0.weight` ([512, Cin, k], bias-free conv + ReLU, (k, stride) = (10,5) (8,4) (4,2) (4,2) (4,2) (1,1) (1,1) (1,1));
 * other `audio_model.*` / `lip_model.*` tensors of a checkpoint are accepted and ignored (a2p_frontend_set_weight returns 1). */
typedef struct a2p_frontend_ctx a2p_frontend_ctx;
typedef struct a2p_frontend_config {
  int32_t conv_dim;          /* 512 */
  int32_t resample;          /* 0: x[::3]; 1: torchaudio Resample(48000, 16000) windowed sinc (hann, width 6, rolloff 0.99) */
  int32_t lip;               /* 1: the lip regressor is present (face model) */
  int32_t d_model, num_heads, ff_size, enc_layers, dec_layers; /* RegressionTransformer: 512, 4, 1024, 2, 4 */
  int32_t lip_out;           /* n_vertices * 3 = 1014 */
  int32_t lip_pad;           /* zeros prepended at 16 kHz by Wav2VecEncoder (320) */
  int32_t chunk_frames;      /* 120 (model/diffusion.py:303) */
  int32_t samples_per_frame; /* 1600 at 48 kHz */
  int32_t max_batch, max_frames;
  int32_t conv_16bit;        /* 1: the two conv feature extractors (99 % of the front end's FLOPs) run on 16-bit MFMA operands -- IEEE half in
                              * liba2p_hip_f16.so, bfloat16 in liba2p_hip.so -- with fp32 accumulation; 0: exact-fp32 MFMA (parity mode).
                              * The resampler, the first conv layer's arithmetic and the lip regressor stay fp32 either way. */
  /* fairseq's published blocks (round 4; fairseq 0.12 models/wav2vec/wav2vec.py ConvFeatureExtractionModel / ConvAggregator -- the
   * package is absent offline: PARITY UNPINNED, restated in oracle/frontend_oracle.py).  All zero = the stub geometry of rounds 2-3
   * (bias-free Conv1d + ReLU, 8 layers, identity aggregator).  `a_*`: audio_model.feature_extractor (vq-wav2vec.pt, model/utils.py:18-26),
   * `l_*`: lip_model.audio_encoder.wav2vec_model (wav2vec_large.pt, model/modules/audio_encoder.py:24-46). */
  int32_t a_group_norm, l_group_norm;     /* 1: Conv1d -> Fp32GroupNorm(1, C, affine) -> activation; parameters conv_layers.{i}.2.{weight,bias} */
  int32_t a_activation, l_activation;     /* 0: ReLU, 1: GELU (erf) */
  int32_t a_log_compression, l_log_compression; /* 1: log(|x| + 1) behind the last conv layer */
  int32_t a_skip, l_skip;                 /* 1: skip connections between equal-width layers: (x + residual[..., ::r][..., :T]) * sqrt(residual_scale) */
  float a_residual_scale, l_residual_scale;
  int32_t l_layers;                       /* conv layers of the lip encoder's feature extractor: 0 or 8 = (10,5)(8,4)(4,2)x3(1,1)x3; 7 drops the last (1,1) */
  int32_t agg_layers;                     /* 0: identity aggregator; n <= 12: ConvAggregator layers of kernel 2, 3, ..., n + 1 (stride 1, causal padding),
                                           * parameters feature_aggregator.conv_layers.{j}.1.{weight[,bias]}, .3.{weight,bias} (GroupNorm) */
  int32_t agg_skip;                       /* 1: x = (block(x) + x) * sqrt(agg_residual_scale) */
  float agg_residual_scale;
  int32_t agg_conv_bias;                  /* 1: the aggregator's convolutions carry a bias */
  int32_t agg_zero_pad;                   /* 1: ZeroPad1d(k - 1, 0) instead of ReplicationPad1d((k - 1, 0)) */
  int32_t agg_activation;                 /* as a_activation */
  int32_t reserved[2];
} a2p_frontend_config;
int a2p_frontend_create(const a2p_frontend_config* cfg, a2p_frontend_ctx** out);
int a2p_frontend_destroy(a2p_frontend_ctx* ctx);
int a2p_frontend_set_weight(a2p_frontend_ctx* ctx, const char* name, const float* dev_ptr, int64_t numel, void* stream);
int a2p_frontend_finalize(a2p_frontend_ctx* ctx, void* stream);
/* encode_audio: audio fp32 [batch, samples, 2] (48 kHz stereo) -> out fp32 [batch, n_tokens, 2 * conv_dim]; fails if the conv
 * geometry does not give exactly n_tokens. */
int a2p_frontend_encode_audio(a2p_frontend_ctx* ctx, const float* audio, int32_t batch, int64_t samples, float* out,
                              int32_t n_tokens, void* stream);
/* encode_lip: out [batch, n_tokens, cond_dim + lip_out] = cat(cond_in [batch, n_tokens, cond_dim], interpolate(lip(audio[..., 0]))). */
int a2p_frontend_encode_lip(a2p_frontend_ctx* ctx, const float* audio, int32_t batch, int64_t samples, const float* cond_in,
                            int32_t n_tokens, int32_t cond_dim, float* out, void* stream);

/* ---- motion evaluation (reference utils/eval.py; audio2photoreal_amd/evaluate.py) -------------------------------------
 * Everything is fp64.  x is a motion batch [S, C, T] channels-first (the samplers' [S, C, 1, T] is the same memory), fp32
 * (x_f64 = 0) or fp64 (x_f64 = 1); 1 <= C <= A2P_EVAL_MAX_CHANNELS.  No floating-point atomics: results are the same bits on
 * every run.  nonfinite: one device int the kernels OR into (1: a non-finite input element, 2: a pair index out of range);
 * the caller zeroes it and reads it back.
 *
 * a2p_eval_moments (T >= 2): over the N = S T frames x[s, :, t], mu [C] and cov [C, C] normalised by N - 1 (np.cov), over the
 * S (T - 1) in-sequence velocities x[s, :, t + 1] - x[s, :, t], mu_v and cov_v.  Second moments are centred (two passes) and
 * the per-range partials are merged in a fixed order.  sums[0] = sum over (s, c) of the variance along T (ddof 0),
 * sums[1] = sum over the B C T elements of one repetition of the variance across the reps repetitions x[r B + b] (S = reps B;
 * reps = 0 skips it and writes 0).  workspace: A2P_EVAL_MOMENTS_WS_DOUBLES(C) doubles. */
#define A2P_EVAL_MAX_CHANNELS 256
#define A2P_EVAL_NSPLIT 16
#define A2P_EVAL_XV_PARTIALS 256
#define A2P_EVAL_MOMENTS_WS_DOUBLES(C) ((int64_t)A2P_EVAL_NSPLIT * (C) * (C) + (C) + A2P_EVAL_XV_PARTIALS)
int a2p_eval_moments(const void* x, int32_t x_f64, int32_t S, int32_t C, int32_t T, int32_t reps, double* mu, double* cov,
                     double* mu_v, double* cov_v, double* sums, double* workspace, int32_t* nonfinite, void* stream);
/* dist[i] = || frame idx1[i] - frame idx2[i] ||_2 (times pairs), frame f = x[f / T, :, f % T]: the rows of the reference's
 * transpose(0, 1, 3, 2).reshape(-1, C), read without a transposed copy.  idx1 / idx2: device int64. */
int a2p_eval_pair_dist(const void* x, int32_t x_f64, int32_t S, int32_t C, int32_t T, const int64_t* idx1, const int64_t* idx2,
                       int64_t times, double* dist, int32_t* nonfinite, void* stream);
/* c[i][j] = sum_k a[i a_rs + k a_cs] d[k] b[k b_rs + j b_cs] for n x n fp64 (d NULL: no scaling; the strides express transposes),
 * n <= A2P_EVAL_MAX_CHANNELS; c must not alias an input. */
int a2p_eval_gemm_f64(int32_t n, const double* a, int64_t a_rs, int64_t a_cs, const double* d, const double* b, int64_t b_rs,
                      int64_t b_cs, double* c, void* stream);
/* Symmetric eigensolver: cyclic Jacobi with round-robin ordering, one workgroup, n <= A2P_EVAL_MAX_CHANNELS.  a [n, n] (read as
 * 0.5 (a + a^T)) -> eigenvalues w [n] (unsorted) and, when q is not NULL, eigenvectors q [n, n] (column j belongs to w[j]:
 * a = q diag(w) q^T).  Stops when ||offdiag||_F <= 1e-15 ||a||_F; sweeps_host / off_host (host, may be NULL) receive the sweeps
 * used and that final norm.  Synchronises `stream`.  A2P_ERR_NOCONVERGE when the sweep cap (40) is hit, A2P_ERR_NONFINITE for a
 * non-finite input.  workspace: A2P_EVAL_EIGH_WS_DOUBLES(n) doubles of device memory. */
#define A2P_EVAL_EIGH_WS_DOUBLES(n) ((int64_t)((n) + ((n) & 1)) * ((n) + ((n) & 1)) + 2)
int a2p_eval_eigh(const double* a, int32_t n, double* w, double* q, double* workspace, int32_t* sweeps_host, double* off_host,
                  void* stream);

/* ---- capture dataset (reference data_loaders/data.py:223-253, tensors.py:71-86; audio2photoreal_amd/data/) ----------------
 * What Social.__getitem__ + social_collate build for `batch` chunks of the test split, from takes that stay resident on the
 * device in their stored dtypes.  Chunk b is the frames [start_of[b], start_of[b] + frames) of take take_of[b] (host arrays).
 *   inp       fp32 [batch, channels, 1, frames]   (motion - mean) / std in fp64, times the presence flag when face != 0
 *                                                 (data.py:251-252), rounded once to fp32
 *   keyframes fp32 [batch, ceil(frames / key_step), channels]   the same values at frames 0, key_step, 2 key_step, ...
 *   missing   fp32 [batch, frames, channels]      the presence flag (face != 0) or ones
 *   audio     fp32 [batch, frames * samples_per_frame, 2]   (a - audio_mean[c]) / audio_std in fp32; swap_channels != 0 reads
 *                                                 channel 1 - c (the reference's flip_person)
 * Every output value is added to +0.0f as collate_tensors' zeroed canvas does (tensors.py:23-28: -0.0 becomes +0.0).
 * Correctly rounded IEEE operations only: the outputs carry the reference's bits.  mean / std_dev: device fp64 [channels].
 * One launch on `stream`; no allocation, copy or synchronisation (the chunk table travels in the kernel arguments).  Audio
 * pointers must be 16-byte aligned and samples_per_frame even. */
#define A2P_DATASET_MAX_BATCH 64
typedef struct a2p_dataset_take {
  const void* motion;      /* device [frames, channels], fp64 (motion_f64 != 0) or fp32: takes of one call may differ */
  const uint8_t* present;  /* device [frames]: 0 on the missing face frames, 1 elsewhere; NULL: every frame present */
  const float* audio;      /* device [frames * samples_per_frame, 2] */
  int64_t frames;
  int32_t motion_f64;
  int32_t reserved;
} a2p_dataset_take;
int a2p_dataset_batch(const a2p_dataset_take* takes, int32_t n_takes, int32_t channels, int32_t face,
                      const int32_t* take_of, const int64_t* start_of, int32_t batch, int32_t frames, int32_t key_step,
                      int32_t samples_per_frame, const double* mean, const double* std_dev, float audio_mean0, float audio_mean1,
                      float audio_std, int32_t swap_channels, float* inp, float* keyframes, float* missing, float* audio,
                      void* stream);

/* ---- posed geometry (reference visualize/ca_body/utils/lbs.py; audio2photoreal_amd/skinning.py) -------------------------------
 * From un-normalised body poses to joint states, skinning matrices and posed vertices, fp32 like the reference, for all N frames
 * in one launch each.  Context-free; the skeleton tables are device arrays built and validated once by the caller.  No atomics
 * and a fixed summation order: a frame's result depends on neither N nor its index, and two runs give the same bits.
 *
 * a2p_skin_states: x = cat(pose [N, P_pos], scale [N or 1, P_scale]) (scale_per_frame = 0 shares row 0; P_scale = 0: no scale
 * parameters); the [7 J, P] parameter transform as compressed rows (row_ptr [7 J + 1], cols / vals ascending in the column) plus
 * offsets [7 J] gives (tx ty tz rx ry rz sc) per joint; local t = value + joint_offset [J, 3], q = pre_rotation [J, 4] (xyzw)
 * (x) fromXYZ(r) with half angles (-0.5, 0.5, 0.5), s = exp2(sc); the joints are solved level by level (order [J]: joints sorted
 * by depth, level_start [n_levels + 1]; parents [J] int32, -1 for a root; every parent sits in an earlier level).  Outputs, either
 * may be NULL: states [N, J, 8] (translation 3, quaternion xyzw 4, scale 1: solve_skeleton_state) and mats [N, J, 3, 4]
 * (states_to_matrix) against inv_bind [J, 8] = (rot(bind_q^-1, -bind_t) / bind_s, bind_q^-1, 1 / bind_s).
 *
 * a2p_skin_vertices: out [N, V, 3] = (sum over k < K of w[k][v] mats[n][idx[k][v]] [p, 1]) * (gx, gy, gz) with p = base [V, 3]
 * + unposed (NULL, [V, 3] when unposed_per_frame = 0, else [N, V, 3]).  idx (int32, in [0, J)) and w are stored [K, V]; unused
 * slots hold weight 0. */
#define A2P_SKIN_MAX_JOINTS 1024
#define A2P_SKIN_MAX_PARAMS 1024
#define A2P_SKIN_MAX_INFLUENCES 16
int a2p_skin_states(const float* pose, const float* scale, int32_t scale_per_frame, int64_t N, int32_t P_pos, int32_t P_scale,
                    int32_t J, const int32_t* row_ptr, const int32_t* cols, const float* vals, const float* offsets,
                    const float* joint_offset, const float* pre_rotation, const int32_t* parents, const int32_t* order,
                    const int32_t* level_start, int32_t n_levels, const float* inv_bind, float* states, float* mats, void* stream);
int a2p_skin_vertices(const float* mats, int64_t N, int32_t J, const float* base, const float* unposed, int32_t unposed_per_frame,
                      const int32_t* idx, const float* w, int32_t V, int32_t K, float gx, float gy, float gz, float* out,
                      void* stream);

/* ---- steering joints to 3D targets (audio2photoreal_amd/sample/steer.py, skinning.py; csrc/kernels_steer.h) -------------------
 * The skeleton solve of a2p_skin_states with a loss on joint positions and orientations, its gradient with respect to the pose
 * parameters (a backward pass through the solve) and a few steps of descent, per frame, in one launch.  a2p_steer describes the
 * skeleton, the constraints and the descent for both entry points:
 *   skeleton: a2p_skin_states' device tables, plus the children of every joint (child_ptr [J + 1], child_idx ascending inside a
 *     joint) and the P_pos pose columns of the parameter transform as compressed columns (col_ptr [P_pos + 1], rows ascending /
 *     cvals); scale [N or 1, P_scale] (scale_per_frame as a2p_skin_states) are constants; global_scaling multiplies a joint's
 *     translation into its position p.
 *   theta = mean + std z (mean / std fp32 [P_pos] on the device; either may be NULL: 0 / 1).
 *   constraints k < K <= A2P_STEER_MAX_CONSTRAINTS: joints / kinds / axes are HOST arrays (joint in [0, J), kind A2P_STEER_REACH
 *     or A2P_STEER_AIM, axes [K, 3]); targets fp32 [N, K, 3] and weights fp32 [N, K] (>= 0) are device arrays, frame n = b T + t
 *     in a step.  reach: w/2 |p - y|^2.  aim: w (1 - rot(q_j, axis) . d) with d = (y - p) / |y - p| held constant (the term
 *     and its gradient are 0 when y = p).  L = the sum over k.
 *   descent: g = std dL/dtheta; `iterations` times z <- z - min(alpha L / |g|^2, max_step / |g|inf) g.  L = 0, g = 0 and
 *     non-finite values leave z unchanged.  A frame whose weights are all zero is not touched.
 * No atomics and a fixed summation order: a frame's result depends on neither N nor its index, and two runs give the same bits.
 *
 * a2p_skin_steer: context-free.  z_in [N] rows of P_pos with row stride z_in_stride -> z_out (row stride z_out_stride; may be
 * z_in with the same stride), loss [N] and grad [N, P_pos] (L and g before the first iteration; either may be NULL).
 * iterations = 0 computes loss and grad only (z_out = z_in).
 *
 * a2p_sample_step_steer: a2p_sample_step of a pose context (nfeats == P_pos; N = B T) whose guided output -- u + scale (a - u), or
 * the combine of a2p_set_guidance -- is steered per frame before the clamp of clip_denoised and the DDIM / DDPM update.  The
 * steered rows replace both sequence blocks of the model output, and the unchanged step tail then returns them bit for bit; a
 * frame whose weights are all zero gets a2p_sample_step's bits.  steer->scale_per_frame must be 0. */
#define A2P_STEER_MAX_CONSTRAINTS 16
enum a2p_steer_kind { A2P_STEER_REACH = 0, A2P_STEER_AIM = 1 };
typedef struct a2p_steer {
  const int32_t* row_ptr; const int32_t* cols; const float* vals; const float* offsets;
  const float* joint_offset; const float* pre_rotation;
  const int32_t* parents; const int32_t* order; const int32_t* level_start;
  const int32_t* child_ptr; const int32_t* child_idx;
  const int32_t* col_ptr; const int32_t* rows; const float* cvals;
  const float* mean; const float* std; const float* scale;
  const int32_t* joints_host; const int32_t* kinds_host; const float* axes_host;
  const float* targets; const float* weights;
  float global_scaling[3];
  float alpha, max_step;
  int32_t P_pos, P_scale, J, n_levels, scale_per_frame, K, iterations;
} a2p_steer;
int a2p_skin_steer(const a2p_steer* steer, const float* z_in, int64_t z_in_stride, int64_t N, float* z_out, int64_t z_out_stride,
                   float* loss, float* grad, void* stream);
int a2p_sample_step_steer(a2p_ctx* ctx, int32_t sampler, const float* x, const int64_t* t_idx, const int64_t* timestep_map,
                          const float* tables, int32_t n_steps, const float* scale, const float* noise, float eta,
                          int32_t clip_denoised, const a2p_steer* steer, float* x_next, float* pred_xstart, void* stream);

/* ---- surface maps (reference visualize/ca_body/utils/geom.py; audio2photoreal_amd/surface.py) ---------------------------------
 * Normals, view cosine and UV maps of the posed mesh, fp32 like the reference, for all N frames in one launch each.  Context-free;
 * the topology tables are device arrays built and validated once by the caller (vi / vti [F, 3] int32 with entries in [0, V) /
 * [0, T), vt [T, 2]).  No float atomics and a fixed summation order: a frame's result depends on neither N nor its index, and two
 * runs give the same bits.  An output must not alias an input.
 *
 * a2p_surface_normals: verts [N, V, 3] -> normals [N, V, 3] (vert_normals) and view_cos [N, V] (compute_view_cos; camera [N, 3]
 * when camera_per_frame, else [1, 3]); either output may be NULL, view_cos needs the camera.  inc_ptr [V + 1] / inc_face: the
 * faces of vertex v, ascending in the face and then the corner (a face that lists v twice appears twice; an unused vertex has an
 * empty range and gets normal 0).  The face normals cross(p1 - p0, p2 - p0) are normalised (a length below 1e-5 counts as 1),
 * summed in table order and normalised by the same rule.
 *
 * a2p_surface_to_uv: values [N, V, C] -> out [N, C, H, H] (values_to_uv): b0 x[i0] + b1 x[i1] + b2 x[i2] where the texel's three
 * entries of index_image [H, H, 3] (int32, in [-1, V)) all differ from -1, else 0; bary_image [H, H, 3].  Every texel is written.
 *
 * a2p_surface_from_uv: values_uv [N, C, H', W'] -> out [N, V, C] (sample_uv as GeometryModule.from_uv calls it): the mean over
 * the 4 slots of v2uv [V, 4] (int32, in [0, T)) of the bilinear sample at vt[slot] (align_corners, zero padding).
 *
 * a2p_surface_uv_index: the one-time UV rasterisation at H x H: texel (row i, column j) has centre ((j + 0.5) / H, (i + 0.5) / H);
 * a face covers it when the centre is inside or on the boundary of its UV triangle; a zero-area triangle covers nothing; the
 * lowest covering face wins.  face_image [H, H] (-1: none), index_image [H, H, 3] = vi[face] (-1) and bary_image [H, H, 3] = the
 * reference's bary_coords of the centre (0).  All three images are required and written whole. */
#define A2P_SURFACE_MAX_UV 16384
#define A2P_SURFACE_MAX_CHANNELS 16
int a2p_surface_normals(const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const int32_t* inc_ptr,
                        const int32_t* inc_face, const float* camera, int32_t camera_per_frame, float* normals, float* view_cos,
                        void* stream);
int a2p_surface_to_uv(const float* values, int64_t N, int32_t V, int32_t C, const int32_t* index_image, const float* bary_image,
                      int32_t H, float* out, void* stream);
int a2p_surface_from_uv(const float* values_uv, int64_t N, int32_t C, int32_t Hs, int32_t Ws, const float* vt, int32_t T,
                        const int32_t* v2uv, int32_t V, float* out, void* stream);
int a2p_surface_uv_index(const float* vt, int32_t T, const int32_t* vti, const int32_t* vi, int32_t F, int32_t H,
                         int32_t* index_image, float* bary_image, int32_t* face_image, void* stream);

/* ---- rendered images (reference visualize/ca_body/utils/render.py RenderLayer; audio2photoreal_amd/render.py) -----------------
 * The posed mesh rasterised to images, fp32 like the reference, all N frames of a call in a fixed number of launches.  Context-
 * free; vi / vti [F, 3] int32 with entries in [0, V) / [0, T) and vt [T, 2] are device arrays validated once by the caller.  The
 * only atomic is a 64-bit integer minimum: a frame's result depends on neither N nor its index, and two runs give the same bits.
 * An output or scratch array must not alias an input.  N = 0 returns 0 without a launch.
 *
 * a2p_render_rasterize: verts [N, V, 3]; Rt [N, 3, 4] when rt_per_frame, else [1, 3, 4]; K [N, 3, 3] when k_per_frame, else [1,
 * 3, 3] (OpenCV: x right, y down, z forward).  p = R x + t, u = K00 (x / z) + K01 (y / z) + K02, v = K11 (y / z) + K12 (the skew
 * K01 is supported; the other entries are not read).  Pixel (row i, column j) has centre (j + 0.5, i + 0.5); a face covers it when
 * the centre is inside or on the boundary of the projected triangle (either winding; zero area covers nothing); a face with a
 * corner at z < near (near > 0) is dropped whole.  Depth is perspective-correct, 1 / z = sum of b_k / z_k over the screen
 * barycentrics b; the nearest face wins, the lowest face index among equal depth bits; a pixel whose depth is not a positive
 * finite number is not covered.  Scratch, contents undefined on return: proj [N, V, 3] float and key [N, H, W] 64-bit words.
 * Outputs, each may be NULL and the others are written whole: face [N, H, W] (-1: background), bary [N, H, W, 3] (perspective-
 * correct, b_k' = (b_k / z_k) / sum of b_j / z_j; 0) and depth [N, H, W] (0).
 *
 * a2p_render_interpolate: values [N, V, C] -> out [N, C, H, W] = b0 x[i0] + b1 x[i1] + b2 x[i2] with (i0, i1, i2) = vi[face]
 * and the pixel's bary; 0 where face is outside [0, F).
 *
 * a2p_render_texture: pixel uv = sum of b_k vt[vti[face][k]] (v <- 1 - v when flip_v), bilinear sample of tex ([N, C, Ht, Wt]
 * when tex_per_frame, else [1, C, Ht, Wt]) at x = u (Wt - 1), y = v (Ht - 1) clamped to the border, taps nw, ne, sw, se summed in
 * that order -> out [N, C, H, W]; 0 where face is outside [0, F). */
#define A2P_RENDER_MAX_SIZE 8192
#define A2P_RENDER_MAX_CHANNELS 16
int a2p_render_rasterize(const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const float* K, int32_t k_per_frame,
                         const float* Rt, int32_t rt_per_frame, int32_t H, int32_t W, float near, float* proj, uint64_t* key,
                         int32_t* face, float* bary, float* depth, void* stream);
int a2p_render_interpolate(const float* values, int64_t N, int32_t V, int32_t C, const int32_t* vi, int32_t F, const int32_t* face,
                           const float* bary, int32_t H, int32_t W, float* out, void* stream);
int a2p_render_texture(const int32_t* face, const float* bary, int64_t N, int32_t H, int32_t W, const float* vt, int32_t T,
                       const int32_t* vti, int32_t F, const float* tex, int32_t tex_per_frame, int32_t C, int32_t Ht, int32_t Wt,
                       int32_t flip_v, float* out, void* stream);

/* Anti-aliased images: S x S samples per pixel (1 <= S <= 4, S H and S W <= A2P_RENDER_MAX_SIZE).  Sample (a, b) of pixel (i, j) is
 * pixel (S i + a, S j + b) of the S H x S W image seen through K' = K with its first two rows times S in float32 (in the image's
 * own units its centre is (j + (b + 0.5) / S, i + (a + 0.5) / S)); its face is what a2p_render_rasterize gives at (S H, S W, K'),
 * its value what a2p_render_texture / a2p_render_interpolate give at its barycentrics.  Each call runs projection, key fill, cover
 * pass and one fused resolve: the samples of a pixel are summed a outer, b inner into fp32 accumulators from 0, n counts the
 * covered ones; alpha [N, 1, H, W] = (float)n / (float)(S S), mean = acc / (float)(S S) (premultiplied: an uncovered sample adds 0).
 * bg ([N, C, H, W] when bg_per_frame, else [1, C, H, W]; NULL: none): n == S S gives mean and bg is not read, n == 0 gives bg
 * itself, otherwise mean + (1 - alpha) bg; without bg, mean.  Every element of out [N, C, H, W] and alpha (and of depth [N, 1, H, W],
 * optional: the mean of the samples' depths, premultiplied like out) is written.  proj [N, V, 3] floats and key [N, S H, S W] 64-bit
 * words are scratch; no face index comes from the caller.  No float atomics: a frame's bits depend on neither N nor its index. */
#define A2P_RENDER_MAX_SUPERSAMPLE 4
int a2p_render_antialiased_texture(const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const float* vt, int32_t T,
                                   const int32_t* vti, const float* K, int32_t k_per_frame, const float* Rt, int32_t rt_per_frame,
                                   int32_t H, int32_t W, int32_t S, float near, const float* tex, int32_t tex_per_frame, int32_t C,
                                   int32_t Ht, int32_t Wt, int32_t flip_v, const float* bg, int32_t bg_per_frame, float* proj,
                                   uint64_t* key, float* out, float* alpha, void* stream);
int a2p_render_antialiased_values(const float* verts, int64_t N, int32_t V, const int32_t* vi, int32_t F, const float* K,
                                  int32_t k_per_frame, const float* Rt, int32_t rt_per_frame, int32_t H, int32_t W, int32_t S, float near,
                                  const float* values, int32_t C, const float* bg, int32_t bg_per_frame, float* proj, uint64_t* key,
                                  float* out, float* alpha, float* depth, void* stream);

/* Scenes of several bodies (audio2photoreal_amd/scene.py): P meshes, 1 <= P <= A2P_SCENE_MAX_BODIES, in one image with one shared
 * z-buffer per sample.  Body p: verts [N, V, 3]; vt [T, 2] and vti [F, 3] (its own face numbering, entries in [0, T)); tex [N, C, Ht,
 * Wt] when tex_per_frame, else [1, C, Ht, Wt] (C is the call's, the sizes are the body's); flip_v; placement NULL, or [N, 3, 4] when
 * placement_per_frame, else [1, 3, 4]: x_world = R x + t with M = [R | t].  faces [sum F, 3] is the merged face table the caller
 * built once: body p's vi with the sum of the earlier bodies' V added, bodies in order (entries in [0, sum V)).
 *
 * One launch projects every body into proj [N, sum V, 3] through K' = K with its first two rows times S in float32, as the
 * anti-aliased images above.  A body without a placement is projected exactly as a2p_render_rasterize projects it.  A placed vertex is
 * first moved, per coordinate r, by w_r = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3] in float32, every product and sum rounded
 * (no fused multiply-add), and w is projected in its place.  Key fill and cover pass then run on the merged mesh at (S H, S W): the
 * key is depth bits << 32 | global face index, so at exactly equal depth the earlier body wins, then the lower face.  One fused resolve
 * walks a pixel's samples a outer, b inner, finds each sample's body from its global face index and shades it from that body's vt,
 * vti, tex and flip_v by a2p_render_texture's expression, into fp32 accumulators from 0; n counts the covered samples, n_p those body
 * p wins.  alpha [N, 1, H, W] = (float)n / (float)(S S); out [N, C, H, W] = acc / (float)(S S) (premultiplied), over bg ([N, C, H, W]
 * when bg_per_frame, else [1, C, H, W]; NULL: none) by the rule above: n == S S does not read bg, n == 0 gives bg itself, otherwise
 * mean + (1 - alpha) bg; depth [N, 1, H, W] = the sum of the covered samples' camera-space depths / (float)(S S); body_alpha [N, P, H,
 * W] = (float)n_p / (float)(S S).  Every element of the four outputs is written; all four are required.  proj [N, sum V, 3] floats and
 * key [N, S H, S W] 64-bit words are scratch.  Limits: 3 sum V and 3 sum F < 2^31; the image and channel limits above; a face with a
 * corner at z < near is dropped whole (one near plane for all bodies).  No float atomics: a frame's bits depend on neither N nor its
 * index.  No scratch or output array may alias an input or another. */
#define A2P_SCENE_MAX_BODIES 4
typedef struct a2p_scene_body {
  const float* verts;
  const float* placement;
  const float* tex;
  const float* vt;
  const int32_t* vti;
  int32_t V, F, T, Ht, Wt, flip_v, placement_per_frame, tex_per_frame;
} a2p_scene_body;
int a2p_scene_render(const a2p_scene_body* bodies, int32_t P, const int32_t* faces, int64_t N, const float* K, int32_t k_per_frame,
                     const float* Rt, int32_t rt_per_frame, int32_t H, int32_t W, int32_t S, float near, int32_t C, const float* bg,
                     int32_t bg_per_frame, float* proj, uint64_t* key, float* out, float* alpha, float* depth, float* body_alpha,
                     void* stream);

/* ---- decoder layers (reference visualize/ca_body/nn/layers.py, nn/blocks.py, utils/seams.py; audio2photoreal_amd/decoder.py) --
 * The layer family of the body renderer's networks, fp32 like the reference, on the caller's stream.  Context-free: weights
 * (already folded, w = v g / ||v||), biases, masks and seam tables are device arrays the caller prepared once.  No atomics and a
 * fixed summation order: a frame's result depends on neither N nor its index, and two runs give the same bits.  An output must
 * not overlap an input.  N = 0 (planes = 0) returns 0 without a launch.
 *
 * a2p_conv2d_ub: direct convolution for few channels; NCHW, stride 1, zero padding k / 2, k = 1 or 3, groups >= 1 with at most
 * A2P_CONV_MAX_CHANNELS input and output channels per group.  Per output element, in this order:
 *   v = sum over ci ascending, then ky, kx row-major, of weight[oc][ci][ky][kx] x[n][g C_in/groups + ci][y + ky - k/2][x + kx - k/2]
 *   v = v + bias                    bias_mode TIED: bias [C_out]; UNTIED: bias [C_out, H, W]
 *   v = v >= 0 ? v : slope v        when act
 *   v = v + skip                    skip_mode TENSOR: skip [N, C_out, H, W]; CONV: skip_bias[oc] (0 when NULL) + sum over cs
 *                                   ascending of skip_weight[oc][cs] skip_src[n][g C_s/groups + cs][y][x] (a 1 x 1 convolution
 *                                   with the same `groups`; skip_weight [C_out, C_s / groups])
 *   out = v * mask[y][x]            when mask [H, W] is given
 * A source (x, skip_src) is [N, C, Hs, Ws] with frames frame_stride floats apart (>= C Hs Ws: a channel window of a larger
 * tensor is a source).  When (Hs, Ws) differs from (H, W) it is read through nn.UpsamplingBilinear2d((H, W)) -- bilinear,
 * align_corners = True, any ratio: src = dst (Hs - 1) / (H - 1) in float32, i0 = min((int)src, Hs - 1), i1 = min(i0 + 1, Hs - 1),
 * l = src - i0, value = (1 - ly) ((1 - lx) a00 + lx a01) + ly ((1 - lx) a10 + lx a11) -- and the upsampled tensor is never
 * written.  out [N, C_out, H, W] is written whole.
 *
 * a2p_seam_impaint: SeamSampler.impaint on value [planes, H, W] in place: value[p][dst[i]] = (value before the call)[p][src[i]]
 * for the P pairs of flat texel indices in [0, H W); dst holds a texel at most once.  scratch: planes * P floats, contents
 * undefined on return.
 *
 * a2p_seam_resample: SeamSampler.resample, out of place: out = (1 - w) tex + w s with s the grid_sample (bilinear, align_corners
 * = False, padding_mode border) of the plane at g = 2 (uv - 0.5); uvs [H, W, 2] (u along x), weights [H, W].  x = ((g + 1) W -
 * 1) / 2 clamped to [0, W - 1]; the taps nw, ne, sw, se are summed in that order. */
#define A2P_CONV_MAX_CHANNELS 4096
#define A2P_CONV_MAX_SIZE 16384
enum { A2P_CONV_BIAS_NONE = 0, A2P_CONV_BIAS_TIED = 1, A2P_CONV_BIAS_UNTIED = 2 };
enum { A2P_CONV_SKIP_NONE = 0, A2P_CONV_SKIP_TENSOR = 1, A2P_CONV_SKIP_CONV = 2 };
typedef struct a2p_conv_source {
  const float* data;
  int64_t frame_stride;
  int32_t C, H, W, reserved;
} a2p_conv_source;
typedef struct a2p_conv2d_desc {
  a2p_conv_source x;
  a2p_conv_source skip_src;
  const float* weight;
  const float* bias;
  const float* skip;
  const float* skip_weight;
  const float* skip_bias;
  const float* mask;
  float* out;
  int64_t N;
  int32_t C_out, H, W, k, groups, bias_mode, act, skip_mode;
  float slope;
  int32_t reserved;
} a2p_conv2d_desc;
int a2p_conv2d_ub(const a2p_conv2d_desc* desc, void* stream);
int a2p_seam_impaint(float* value, int64_t planes, int32_t H, int32_t W, const int32_t* dst, const int32_t* src, int32_t P,
                     float* scratch, void* stream);
int a2p_seam_resample(const float* tex, int64_t planes, int32_t H, int32_t W, const float* uvs, const float* weights, float* out,
                      void* stream);

/* ---- texture layers (reference visualize/ca_body/nn/unet.py, nn/shadow.py, models/mesh_vae_drivable.py forward_tex;
 * audio2photoreal_amd/texture.py) --
 * What turns the decoder's mean texture into the final one.  Like the decoder layers: fp32, NCHW, on the caller's stream,
 * context-free, weights already folded, no atomics and a fixed summation order (a frame's result depends on neither N nor its
 * index), the same limits A2P_CONV_MAX_CHANNELS per layer side and A2P_CONV_MAX_SIZE per plane side; an output must not overlap
 * an input; N = 0 (planes = 0) returns 0 without a launch.
 *
 * a2p_conv2d_down_ub: la.Conv2dWNUB(C_in, C_out, H, W, 4, 2, 1) and an optional LeakyReLU.  x is a source [N, C_in, Hs, Ws] as in
 * a2p_conv2d_ub (frame stride, channel windows), read directly; Hs, Ws >= 2, odd sizes allowed; weight [C_out, C_in, 4, 4]; out
 * [N, C_out, H, W] with H = (Hs - 2) / 2 + 1, W = (Ws - 2) / 2 + 1 (floor division).  Per output element, in this order:
 *   v = sum over ci ascending, then ky, kx row-major, of weight[co][ci][ky][kx] x[n][ci][2 y - 1 + ky][2 x - 1 + kx]  (0 outside)
 *   v = v + bias                    bias_mode as in a2p_conv2d_ub (TIED [C_out], UNTIED [C_out, H, W])
 *   v = v >= 0 ? v : slope v        when act = A2P_TEX_ACT_LRELU
 * skip must be NULL and act at most LRELU.
 *
 * a2p_conv_transpose2d_ub: la.ConvTranspose2dWNUB(C_in, C_out, 2 Hs, 2 Ws, 4, 2, 1) with the epilogues the reference puts behind
 * it.  weight [C_in, C_out, 4, 4] (PyTorch's transposed layout); x [N, C_in, Hs, Ws] with Hs, Ws in [1, A2P_CONV_MAX_SIZE / 2];
 * out [N, C_out, 2 Hs, 2 Ws].
 *   v = sum over ci ascending, then the valid taps with ky ascending, then kx ascending, of
 *       weight[ci][co][ky][kx] x[n][ci][(Y + 1 - ky) / 2][(X + 1 - kx) / 2]
 *       a tap is valid when Y + 1 - ky and X + 1 - kx are even; a source position outside the plane counts 0.  Even Y: ky = 1
 *       (row Y / 2) and ky = 3 (row Y / 2 - 1); odd Y: ky = 0 (row (Y + 1) / 2) and ky = 2 (row (Y - 1) / 2)
 *   v = v + bias
 *   v = v >= 0 ? v : slope v        act = A2P_TEX_ACT_LRELU
 *   v = 1 / (1 + expf(-(v + beta))) act = A2P_TEX_ACT_SIGMOID (accurate expf)
 *   v = v + skip                    when skip [N, C_out, 2 Hs, 2 Ws] is given
 *
 * a2p_resize_bilinear: F.interpolate(x, (H, W), mode = "bilinear", align_corners = False) of x [planes, Hs, Ws], any ratio, by
 * PyTorch's float32 rule: scale = Hs / H, src = max((dst + 0.5) scale - 0.5, 0), i0 = min((int)src, Hs - 1), i1 = i0 + (i0 < Hs -
 * 1), l1 = src - i0, l0 = 1 - l1, value = l0y (l0x a00 + l1x a01) + l1y (l0x a10 + l1x a11).
 *
 * a2p_texture_compose: the arithmetic of AutoEncoder.forward_tex between its seam steps, one launch at the output size:
 *   out[n][c][Y][X] = ((resize(t)[n][c][Y][X] + u[n][4 c + 2 (Y % 2) + (X % 2)][Y / 2][X / 2]) tex_std + tex_mean[c][Y][X])
 *                     * shadow[n or 0][0][Y][X]
 * t [N, C, Sh, Sw] read through the rule of a2p_resize_bilinear at exactly twice the size; u [N, 4 C, Sh, Sw] (the index is
 * nn.PixelShuffle(2)); tex_mean [C, 2 Sh, 2 Sw]; shadow [shadow_frames, 1, 2 Sh, 2 Sw] with shadow_frames 1 or N, or NULL for no
 * shadow (shadow_frames ignored).  Only out [N, C, 2 Sh, 2 Sw] is written. */
enum { A2P_TEX_ACT_NONE = 0, A2P_TEX_ACT_LRELU = 1, A2P_TEX_ACT_SIGMOID = 2 };
typedef struct a2p_tex_conv_desc {
  a2p_conv_source x;
  const float* weight;
  const float* bias;
  const float* skip;
  float* out;
  int64_t N;
  int32_t C_out, bias_mode, act;
  float slope, beta;
  int32_t reserved;
} a2p_tex_conv_desc;
int a2p_conv2d_down_ub(const a2p_tex_conv_desc* desc, void* stream);
int a2p_conv_transpose2d_ub(const a2p_tex_conv_desc* desc, void* stream);
int a2p_resize_bilinear(const float* x, int64_t planes, int32_t Hs, int32_t Ws, int32_t H, int32_t W, float* out, void* stream);
int a2p_texture_compose(const float* t, const float* u, const float* tex_mean, float tex_std, const float* shadow,
                        int32_t shadow_frames, int64_t N, int32_t C, int32_t Sh, int32_t Sw, float* out, void* stream);

/* ---- encode layers (reference visualize/ca_body/nn/layers.py LinearWN, nn/blocks.py ConvDownBlock, utils/lbs.py unskinning /
 * unpose, models/mesh_vae_drivable.py FaceEncoder; audio2photoreal_amd/encoder.py, skinning.py) --
 * What lies between the samplers' output and the renderer's embeddings.  Like the decoder and texture layers: fp32, on the
 * caller's stream, context-free, weights already folded, 64-bit offsets, no atomics and a fixed summation order (a frame's result
 * depends on neither N nor its index, and two runs give the same bits); an output must not overlap an input; N = 0 returns 0
 * without a launch.
 *
 * a2p_linear_f32: out[n][o] = act(sum over i of x[n][i] weight[o][i] + bias[o]) for x [N, I] with rows ldx >= I floats apart,
 * weight [O, I] dense, bias [O] or NULL, out [N, O] with rows ldo >= O floats apart; act 0 none, 1 LeakyReLU(slope).  Any I, O >= 1:
 * no padding or alignment beyond 4 bytes is asked of the caller.  The sum over i is cut into S = ceil(I / A2P_LINEAR_KSLICE) slices
 * [256 s, min(I, 256 s + 256)); S depends on I alone.  Per output element, in this order:
 *   a_s = 0;  a_s = fmaf(weight[o][i], x[n][i], a_s) for i ascending over slice s          one fused multiply-add per term
 *   v = a_0;  v = v + a_s for s = 1 .. S - 1 ascending
 *   v = v + bias[o]                 when bias is given
 *   v = v >= 0 ? v : slope v        when act = 1
 * S > 1 takes scratch, S N O floats (scratch_floats says how many it holds; contents undefined on return), and a second launch;
 * S = 1 takes none (scratch may be NULL).  Every weight is read from memory once per 64 rows of x.
 *
 * a2p_conv2d_down3_ub: the second launch of a ConvDownBlock, lrelu2(conv2(h)) + conv_resize(x); the first, h = lrelu1(conv1(x)), is
 * an a2p_conv2d_ub call.  h and x are sources [N, C_in, Hs, Ws] as in a2p_conv2d_ub (frame stride, channel windows) of one shape,
 * read directly; w2 [C_out, C_in, 3, 3]; b2 [C_out, H, W] (untied); wr [C_out, C_in]; br [C_out] or NULL (counts 0); out [N, C_out,
 * H, W] with H = (Hs - 1) / 2 + 1, W = (Ws - 1) / 2 + 1 (floor division; odd sizes allowed); groups = 1; the channel and size limits
 * of a2p_conv2d_ub.  Per output element, in this order:
 *   v = sum over ci ascending, then ky, kx row-major, of w2[co][ci][ky][kx] h[n][ci][2 y - 1 + ky][2 x - 1 + kx]   (0 outside)
 *   v = v + b2[co][y][x]
 *   v = v >= 0 ? v : slope v
 *   r = sum over ci ascending of wr[co][ci] x[n][ci][2 y][2 x];  v = v + (br[co] + r)
 * The 1 x 1 branch is never written to memory.
 *
 * a2p_unskin_vertices: LinearBlendSkinning.unskinning with the two lines of LBSModule.unpose; layouts and limits of
 * a2p_skin_vertices (mats [N, J, 3, 4]; idx / w [K, V]); verts [N, V, 3]; tmpl [V, 3]; out [N, V, 3].  Per frame and vertex:
 *   M = sum over k ascending of w[k][v] mats[n][idx[k][v]], entry by entry from 0;  A = M[:, 0:3], t = M[:, 3]
 *   d = verts[n][v] / (gx, gy, gz) - t                                                 a division, as the reference writes it
 *   out[n][v] = (adj(A) d) / det(A) - tmpl[v]       adj: cofactors as differences of two products; det = A00 C00 + A01 C01 + A02
 *                                                   C02 and every row of adj(A) d summed left to right
 * The reference inverts the 4 x 4 matrix with Tensor.inverse() (an LU); this is the closed form in fp32.  A zero or non-finite
 * determinant yields a non-finite output and is not checked here.
 *
 * a2p_face_tex_cond: raw [N, C, Hs, Ws], bias [C, Hs, Ws], mask [H, W] -> out [N, C, H, W]:
 *   out[n][c][y][x] = (resize(255 ((raw[n][c] + bias[c]) + 0.5))[y][x] / 255 - 0.5) mask[y][x]
 * with the taps, weights and order of a2p_resize_bilinear (align_corners = False, any ratio) and the arithmetic inside applied to
 * each tap; face_tex itself is never written. */
#define A2P_LINEAR_KSLICE 256
typedef struct a2p_down3_desc {
  a2p_conv_source h;
  a2p_conv_source x;
  const float* w2;
  const float* b2;
  const float* wr;
  const float* br;
  float* out;
  int64_t N;
  int32_t C_out;
  float slope;
} a2p_down3_desc;
int a2p_linear_f32(const float* x, int64_t ldx, const float* weight, const float* bias, int64_t N, int32_t I, int32_t O, int32_t act,
                   float slope, float* out, int64_t ldo, float* scratch, int64_t scratch_floats, void* stream);
int a2p_conv2d_down3_ub(const a2p_down3_desc* desc, void* stream);
int a2p_unskin_vertices(const float* mats, int64_t N, int32_t J, const float* verts, const float* tmpl, const int32_t* idx,
                        const float* w, int32_t V, int32_t K, float gx, float gy, float gz, float* out, void* stream);
int a2p_face_tex_cond(const float* raw, const float* bias, const float* mask, int64_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t H,
                      int32_t W, float* out, void* stream);

/* ---- video frames (reference visualize/render_codes.py BodyRenderer.render_full_video, which hands the frames to mediapy and
 * ffmpeg; audio2photoreal_amd/video.py) --
 * Baseline JPEG (ITU-T T.81, sequential DCT, Huffman) of uint8 RGB frames for a Motion-JPEG stream, in two stages.  Context-free,
 * on the caller's stream, 64-bit offsets, no float atomics; a frame's coefficients and bytes depend on that frame and the tables
 * alone, never on N or the frame's index; an output must not overlap an input; N = 0 launches no frame kernel.
 *
 * a2p_jpeg_coefficients: rgb [N, H, W, 3] uint8 with frames frame_stride and rows row_stride BYTES apart (row_stride >= 3 W: a
 * column window of a wider image is read in place) -> out int16 [N, mcu_rows, mcu_cols, blocks_per_mcu, 64], every block in zig-zag
 * order.  subsampling 420: MCU 16 x 16, blocks Y00 Y01 Y10 Y11 Cb Cr; 444: MCU 8 x 8, blocks Y Cb Cr; mcu_rows = ceil(H / MCU),
 * mcu_cols = ceil(W / MCU).  qtab: uint16 [2][64], luminance then chrominance, in natural order (index 8 v + u), every entry >= 1.
 * The arithmetic is fp32 with no intermediate rounding to integers:
 *   Y  = 0.299 R + 0.587 G + 0.114 B;  Cb = -0.168735892 R - 0.331264108 G + 0.5 B + 128;  Cr = 0.5 R - 0.418687589 G - 0.081312411 B + 128
 *   samples right of / below the image repeat its last column / row;  4:2:0 chroma = ((a + b) + (c + d)) / 4 over each 2 x 2 group
 *   f = sample - 128
 *   F(u, v) = 1/4 C(u) C(v) sum over x, y of f(x, y) cos((2 x + 1) u pi / 16) cos((2 y + 1) v pi / 16),  C(0) = 1 / sqrt 2, else 1:
 *             a row pass then a column pass of 8-point sums, each one product and seven fmaf with the index ascending
 *   q = rintf(F / Q[v][u])  (IEEE division, ties to even);  AC coefficients are clamped to +-1023
 * Sizes up to A2P_JPEG_MAX_SIZE, the format's limit.  The loads are 4 bytes wide where rgb, frame_stride and row_stride are
 * multiples of 4 and single bytes otherwise; the results are the same.
 *
 * a2p_jpeg_entropy: coef int16 in that layout (any values: a DC difference is clamped to +-2047, an AC coefficient to +-1023) ->
 * every frame's entropy-coded segment.  The restart interval is one MCU row (DRI = mcu_cols): the DC prediction of every component
 * starts at 0 in every interval, every interval is padded with 1-bits to a byte, and every interval but a frame's last is followed
 * by RSTm (0xFF, 0xD0 + m), m = the row's index mod 8.  DC: the category's code, then the amplitude bits; AC: (run, size) codes, ZRL
 * for runs of 16, EOB when the tail is zero (none when coefficient 63 is not); 0x00 follows every 0xFF data byte.  huff: uint32
 * [A2P_JPEG_HUFF_WORDS]: DC luminance [16] and chrominance [16] by category, AC luminance [256] and chrominance [256] by symbol,
 * each (length << 16) | code, length <= 16.  A block codes to at most A2P_JPEG_BLOCK_BITS bits, which is what the kernel reserves.
 * The call has two forms, used in this order with the same interval and offsets arrays:
 *   out = NULL   sizes: interval int64 [N, mcu_rows] gets the offset of every interval inside its frame's segment and offsets int64
 *                [N + 1] the start of every frame in a packed stream, offsets[n + 1] - offsets[n] = head_bytes + segment + tail_bytes;
 *                offsets[N] is the stream's length
 *   out given    writes: per frame head (head_bytes, copied from `head`; left untouched when head is NULL), the segment, tail
 *                likewise, at out + offsets[n].  No byte at or beyond out_bytes is written: an out_bytes below offsets[N] truncates
 *                the stream and is the caller's error.
 * Nothing is truncated inside the kernels: the bytes are counted before they are written. */
#define A2P_JPEG_MAX_SIZE 65535
#define A2P_JPEG_BLOCK_BITS 1665
#define A2P_JPEG_HUFF_WORDS 544
int a2p_jpeg_coefficients(const uint8_t* rgb, int64_t N, int32_t H, int32_t W, int64_t frame_stride, int64_t row_stride,
                          int32_t subsampling, const uint16_t* qtab, int16_t* out, void* stream);
int a2p_jpeg_entropy(const int16_t* coef, int64_t N, int32_t mcu_rows, int32_t mcu_cols, int32_t blocks_per_mcu, const uint32_t* huff,
                     const uint8_t* head, int32_t head_bytes, const uint8_t* tail, int32_t tail_bytes, int64_t* interval,
                     int64_t* offsets, uint8_t* out, int64_t out_bytes, void* stream);

/* ---- reading video frames (audio2photoreal_amd/video.py decode_jpeg_frames, MJPEGReader) --
 * Baseline sequential, 8-bit, Huffman-coded JPEG back to uint8 RGB, the mirror of the two stages above: an integer stage (restart
 * scan, entropy decoding; exact) and an arithmetic stage (fp32).  Context-free, on the caller's stream, 64-bit offsets, integer
 * atomics only (a minimum); a frame's result depends on that frame and the tables alone; an output must not overlap an input; N = 0
 * launches nothing.  The host parses the marker segments (video.py parse_jpeg_header); the GPU sees entropy-coded bytes only and
 * trusts none of them: every byte index is compared with its interval's end before the byte is read, every loop is bounded by the
 * geometry, and nothing is written outside the frame's own ranges, coefficients and status.
 *
 * Read: one component (an MCU is one block), or three with luminance sampled 1 x 1 (4:4:4, blocks Y Cb Cr), 2 x 1 (4:2:2, Y0 Y1 Cb
 * Cr) or 2 x 2 (4:2:0, Y00 Y01 Y10 Y11 Cb Cr) over 1 x 1 chrominance; any Huffman tables with codes up to 16 bits; any restart
 * interval.  Not read, and rejected by the host before any launch: progressive, extended and arithmetic-coded frames, 12-bit
 * samples, 16-bit quantisation tables, four components, other sampling factors.
 *
 * status: int32 per frame, 0 or (interval << 4) | cause of the first failing interval, cause one of A2P_JPEG_ERR_*.
 *
 * a2p_jpeg_restarts: data uint8 [data_bytes], the entropy-coded segments of N frames; segments int64 [N][2], begin and end of every
 * frame's segment in data (clamped to [0, data_bytes]) -> ranges int64 [N][intervals + 1]: ranges[k], k < intervals, is where
 * interval k starts, ranges[intervals] the segment's end; interval k ends 2 bytes (its RSTm) before ranges[k + 1], the last one at
 * the end.  intervals = ceil(mcus / Ri), 1 without DRI.  A frame passes when it holds exactly intervals - 1 markers, RST0 .. RST7
 * cyclically, and no other: 0xFF is followed by 0x00 or the RSTm due.  One workgroup per frame scans chunks of 4096 bytes: count,
 * prefix sum within the workgroup, write positions.
 *
 * a2p_jpeg_decode_entropy: those ranges -> coef int16 [N, mcu_rows, mcu_cols, blocks_per_mcu, 64] in scan order, the layout of
 * a2p_jpeg_coefficients (blocks_per_mcu 1, 3, 4 or 6); coef and status are zeroed on the stream first and only non-zero
 * coefficients are stored.  One lane per restart interval: byte unstuffing, Huffman decoding from tables in LDS, amplitude
 * extension, DC prediction from 0 in every interval.  restart_interval = 0 (no DRI) is ONE interval and therefore one lane per
 * frame: slow and correct.  restart_status: the status of a2p_jpeg_restarts or NULL; frames it marks are left zero.  tables: int32
 * [A2P_JPEG_TABLES][A2P_JPEG_TABLE_WORDS], DC 0, DC 1, AC 0, AC 1, each maxcode[16] (largest code of length l + 1, -1 for none),
 * offset[16] (index of that length's first symbol minus its first code), then the 256 symbols as bytes.  selectors: bit c the DC
 * table of component c, bit 4 + c its AC table.  A DC category above 11 or an AC size above 10 is not 8-bit baseline and stops the
 * lane, as do a code in no table, a run past coefficient 63, an interval that ends inside a code and a byte left over.
 *
 * a2p_jpeg_pixels: coef in that layout, qtab uint16 [components][64] in scan order (as DQT stores them, one per component in scan
 * order) -> out uint8 [N, H, W, 3] with frames frame_stride and rows row_stride BYTES apart (row_stride >= 3 W: a clip decodes
 * straight into a column window of a wider image; no byte outside the window is written).  fp32, one product and seven fmaf per
 * 8-point sum with the index ascending:
 *   F = coef Q;  t(y, u) = sum over v of F(v, u) c(v, y), then s(y, x) = sum over u of t(y, u) c(u, x),  c(u, x) = C(u) / 2 cos((2 x + 1) u pi / 16)
 *   sample = clamp(s + 128, 0, 255)  (T.81 A.3.1);  a chroma sample serves its whole luma_h x luma_v group (replication, the inverse
 *   of the encoder's box mean; libjpeg's triangle "fancy" upsampling is deliberately not reproduced)
 *   R = Y + 1.402 Cr';  G = Y - 0.344136286 Cb' - 0.714136286 Cr';  B = Y + 1.772 Cb'  (Cb' = Cb - 128, Cr' = Cr - 128; G adds the Cb
 *   term first);  rintf, clamp to [0, 255], crop to H x W.  One component goes to all three channels. */
#define A2P_JPEG_TABLES 4
#define A2P_JPEG_TABLE_WORDS 96
#define A2P_JPEG_ERR_RST_COUNT 1
#define A2P_JPEG_ERR_RST_ORDER 2
#define A2P_JPEG_ERR_MARKER 3
#define A2P_JPEG_ERR_NO_CODE 4
#define A2P_JPEG_ERR_RUN 5
#define A2P_JPEG_ERR_ENDS_IN_CODE 6
#define A2P_JPEG_ERR_AMPLITUDE 7
#define A2P_JPEG_ERR_TRAILING 8
int a2p_jpeg_restarts(const uint8_t* data, int64_t data_bytes, const int64_t* segments, int64_t N, int64_t intervals, int64_t* ranges,
                      int32_t* status, void* stream);
int a2p_jpeg_decode_entropy(const uint8_t* data, int64_t data_bytes, const int64_t* ranges, const int32_t* restart_status, int64_t N,
                            int32_t mcu_rows, int32_t mcu_cols, int32_t blocks_per_mcu, int32_t restart_interval, const int32_t* tables,
                            int32_t selectors, int16_t* coef, int32_t* status, void* stream);
int a2p_jpeg_pixels(const int16_t* coef, int64_t N, int32_t H, int32_t W, int32_t components, int32_t luma_h, int32_t luma_v,
                    const uint16_t* qtab, uint8_t* out, int64_t frame_stride, int64_t row_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* A2P_HIP_H */
