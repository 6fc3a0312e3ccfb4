/*
 * dmx.h — C ABI of libdmx.so, the MI355X (gfx950) native CFG denoising loop.
 *
 * The reference (S-Taichiii/diffusion-model) is pure Python and has no FFI; its
 * drop-in boundary is the duck-typed Python surface:
 *   Diffuser.denoise_cond / sample_latent_cond   (reference diff.py:127-162, 174-369)
 *   UnetCondWithGeomHead.forward                  (reference models/unet_cond_geom.py:79-100)
 *   VAE.decode                                    (reference models/vae.py:64-69)
 * Those Python classes are re-implemented in diffusion-model_amd/ and call the
 * entry points below through ctypes (diffusion-model_amd/dmx/_lib.py).  Each entry
 * point cites the reference call it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, a DMX_E* code otherwise; the message is
 *     available from dmx_last_error() (thread-local).  No C++ exception crosses
 *     this boundary.
 *   - tensors are caller-owned DEVICE pointers (contiguous, fp32 NCHW for x/eps/
 *     images, int64 for t/y, fp32 (n,12) for vals/mask); weights and workspace are
 *     owned by the dmx objects.
 *   - `stream` is a hipStream_t (void* here so that the header needs no HIP).
 *     All work is enqueued on it; calls on one model must be serialised by the
 *     caller.
 */
#ifndef DMX_H_
#define DMX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMX_OK 0
#define DMX_E_ARG 1      /* invalid argument / shape (reference: ValueError / AssertionError) */
#define DMX_E_STATE 2    /* object not ready (e.g. weights missing) */
#define DMX_E_HIP 3      /* HIP runtime failure */
#define DMX_E_INTERNAL 4

/* model kinds */
#define DMX_UNET_COND_GEOM 1 /* models/unet_cond_geom.py:26 UnetCondWithGeomHead */
#define DMX_UNET_COND 2      /* models/unet_cond.py:102    UnetCond               */
#define DMX_UNET 3           /* models/unet.py:101          Unet (unconditional)  */
#define DMX_VAE 4            /* models/vae.py:6             VAE                   */

typedef struct dmx_ctx dmx_ctx;
typedef struct dmx_model dmx_model;

int dmx_abi_version(void);
const char* dmx_last_error(void);

/* Context: one per device per process. */
int dmx_create(int device, dmx_ctx** out);
int dmx_destroy(dmx_ctx* ctx);

/* Sinusoidal time table pos[t-1][0..255] for t = 1..tmax (host fp32, computed by the
 * caller with the reference's own formula, models/unet_cond.py:155-161), copied to
 * the device. */
int dmx_set_time_table(dmx_ctx* ctx, const float* host_table, int tmax);

/* ---- weights (replaces Utils.loadModel -> load_state_dict, utils.py:68-73) ---------
 * Keys are the reference state_dict names; listing them needs no GPU. */
int dmx_model_num_keys(int kind, int in_ch, int remove_deep_conv);
int dmx_model_key(int kind, int in_ch, int remove_deep_conv, int index, char* name_out, int name_cap,
                  int64_t* shape_out /* [4] */, int* ndim_out);

int dmx_model_create(dmx_ctx* ctx, int kind, int in_ch, int remove_deep_conv, dmx_model** out);

/* Constructor arguments of the reference networks that change the checkpoint layout or
 * the arithmetic (UnetCond / UnetCondWithGeomHead / VAE __init__, reference
 * models/unet_cond.py:113, models/unet_cond_geom.py:31-49, models/vae.py:11).
 * dmx_model_create(..) is dmx_model_create_cfg with the reference defaults
 * (num_classes 3, geom_dim 12, geom_hidden 256, scale_factor 0.18215). */
typedef struct dmx_model_config {
  int kind;             /* DMX_UNET_COND_GEOM .. DMX_VAE */
  int in_ch;            /* U-Net latent channels, 1..4 */
  int remove_deep_conv; /* models/unet_cond.py:139-145 */
  int num_classes;      /* class_emb has num_classes + 1 rows (models/unet_cond.py:121) */
  int geom_dim;         /* GeomHead output width (models/unet_cond_geom.py:38) */
  int geom_hidden;      /* GeomHead hidden width (models/unet_cond_geom.py:39) */
  float scale_factor;   /* VAE latent scale (models/vae.py:11,59,66) */
} dmx_model_config;
int dmx_model_create_cfg(dmx_ctx* ctx, const dmx_model_config* cfg, dmx_model** out);
int dmx_model_cfg_num_keys(const dmx_model_config* cfg);
int dmx_model_cfg_key(const dmx_model_config* cfg, int index, char* name_out, int name_cap,
                      int64_t* shape_out /* [4] */, int* ndim_out);
int dmx_model_destroy(dmx_model* m);
/* Register one reference-layout tensor (device pointer, fp32 contiguous).  The pointer is
 * read by dmx_model_finalize and again by dmx_model_refresh and the training entry points, so
 * a caller using those keeps the tensor alive (and at the same address) for the model's life. */
int dmx_model_set_tensor(dmx_model* m, const char* name, const float* dev_ptr, const int64_t* shape, int ndim);
/* Repack every registered tensor into the model's kernel layouts (device-side). */
int dmx_model_finalize(dmx_model* m, void* stream);
/* The registered tensors changed in place (optimizer.step, load_state_dict's copy_): repeat
 * every repack on `stream` (no host sync); the split-precision planes are re-derived before the
 * next mode-1/2 launch.  Replaces re-running Utils.loadModel after each update (utils.py:68-73). */
int dmx_model_refresh(dmx_model* m, void* stream);
/* GEMM arithmetic: 0 = fp32 MFMA (exact fp32 products), 1 (default) = fp32 operands split
 * into fp16 hi+lo on the fp16 matrix cores (3 MFMAs, fp32 accumulate, ~1e-7 relative),
 * 2 = fp16 operands (BASELINE config 4: one MFMA, fp32 accumulate, fp32 norms/softmax/scheduler). */
int dmx_model_set_precision(dmx_model* m, int prec);
int dmx_model_get_precision(const dmx_model* m);
/* What the network's output means.  DMX_PRED_EPS (the default): the noise eps.  DMX_PRED_V: the
 * velocity v = sqrt(ab_t) noise - sqrt(1 - ab_t) x0 (Salimans & Ho 2022).  A v-model's step mixes in
 * output space (CFG, composition, perturbed branch, CFG rescale, geometry guidance) and then converts
 * once per element, immediately before the rule's update:
 *   eps = p_o[t - 1] * out + p_x[t - 1] * x_net       p_o = sqrt(ab), p_x = sqrt(1 - ab), [T] fp32
 * two products and a sum, one IEEE rounding each, never contracted; t is the row's network timestep
 * (clamped to [1, T] for the table read) and x_net the latent the network was evaluated at.  p_o /
 * p_x are device pointers tabulated by the caller; the model keeps device copies (the call waits for
 * `stream`).  Every dmx_step* / dmx_sample_loop* entry honours the setting; a step or loop whose
 * schedule names a timestep above T is DMX_E_ARG before anything is launched (the strided rules'
 * t_map is read back for that: one small device-to-host copy per call, in v-mode only).  A change of
 * kind or tables drops every captured graph and the cached deep feature.  DMX_E_ARG: an unknown kind,
 * DMX_PRED_V with a NULL table, or T < 1; DMX_PRED_EPS reads neither table nor T. */
#define DMX_PRED_EPS 0
#define DMX_PRED_V 1
int dmx_model_set_prediction(dmx_model* m, int kind, const float* p_o, const float* p_x, int T, void* stream);
int dmx_model_get_prediction(const dmx_model* m);
/* The conversion alone, for a foreign v-model: eps_out = p_o[t_n - 1] * out + p_x[t_n - 1] * x with
 * the arithmetic above, t (n,) int64 read at n * t_stride (0: one value for all) and clamped to
 * [1, T]; out, x, eps_out NCHW (n,c,h,w), any c*h*w; eps_out may alias out (not x). */
int dmx_pred_to_eps(const float* out, const float* x, const int64_t* t, int t_stride, const float* p_o,
                    const float* p_x, int T, int n, int c, int h, int w, float* eps_out, void* stream);
/* The x0-form of a v-model, for schedules whose last step is pure noise (ab_T = 0, "zero terminal SNR",
 * Lin et al. 2023), where the eps-form updates divide by sqrt(ab_T) = 0.  The mixed output is converted
 * to both x0 and eps, with x_net and t as above,
 *   x0  = p_o[t - 1] * x_net - p_x[t - 1] * out        eps = p_o[t - 1] * out + p_x[t - 1] * x_net
 * and the rules update from them without a division (one IEEE rounding per operation, never contracted):
 *   DDPM   x' = (d_s[t - 1] * x0 + d_d[t - 1] * eps) + nz * sd[t - 1]           nz = 0 at t == 1
 *   DDIM   x' = (k_s * x0 + k_d * eps) + k_n * nz
 *   DPM    y = k_x * x + k_c * x0;  x' = k_p != 0 ? y + k_p * hist : y;  hist <- x0
 * d_s = sqrt(ab_prev), d_d = (1 - ab_prev) sqrt(a_t) / sqrt(1 - ab_t) with ab_prev = 1 at t = 1: the DDPM
 * posterior mean on (x0, eps), [T] fp32 by network timestep like p_o / p_x; the step's c1 / c2 are not
 * read.  The strided rules read the k_s / k_d / k_n and k_x / k_c / k_p of their schedules and never
 * k_e / k_a.  Inversion has neither an x0 nor a division and converts as DMX_PRED_V does.  The range
 * flag is raised on x0, and on eps where the rule reads it.  Same contract as dmx_model_set_prediction:
 * device copies are kept, a repeated identical call is recognised, a change drops every captured graph
 * and the cached deep feature, a schedule that names a timestep above T is DMX_E_ARG before any launch;
 * dmx_model_get_prediction then returns DMX_PRED_V_X0, and dmx_model_set_prediction with DMX_PRED_EPS or
 * DMX_PRED_V leaves the x0-form (DMX_PRED_V_X0 is not a kind of that entry).  DMX_E_ARG: a NULL table or
 * T < 1. */
#define DMX_PRED_V_X0 2
int dmx_model_set_prediction_x0(dmx_model* m, const float* p_o, const float* p_x, const float* d_s,
                                const float* d_d, int T, void* stream);
/* The x0-form's conversion alone, both halves in one pass: dmx_pred_to_eps's operands and rules;
 * eps_out may alias out; neither output may alias x, nor each other, and x0_out may not alias out. */
int dmx_pred_split(const float* out, const float* x, const int64_t* t, int t_stride, const float* p_o,
                   const float* p_x, int T, int n, int c, int h, int w, float* x0_out, float* eps_out,
                   void* stream);
/* Range guard of the split-precision modes (1, 2): an operand beyond the f16 range turns a
 * network output (eps / decoded pixel / encoder head) non-finite, and the output kernels then
 * raise a sticky per-model flag.  Reads it (synchronising `stream`), optionally clearing it;
 * the Python samplers check it at chunk boundaries and recompute the chunk in mode 0. */
int dmx_model_range_check(dmx_model* m, int reset, int* flagged, void* stream);

/* ---- U-Net forward (replaces model(x, t, y, cond_vals, cond_mask), diff.py:149-150) --
 * x: (n,in_ch,h,w); t: (n,) int64 in [1, tmax]; y: (n,) int64 or NULL (DMX_UNET);
 * vals/mask: (n,12) or NULL; eps: (n,in_ch,h,w); geom: (n,12) or NULL. */
int dmx_unet_forward(dmx_model* m, const float* x, const int64_t* t, const int64_t* y, const float* vals,
                     const float* mask, float* eps, float* geom, int n, int h, int w, void* stream);

/* ---- one denoising step (replaces Diffuser.denoise_cond, diff.py:127-162, with the two
 * model calls batched as one 2n-sample forward, and Diffuser.denoise, diff.py:32-56) ----- */
typedef struct dmx_step_args {
  const float* x_in;        /* (n,C,h,w) */
  float* x_out;             /* (n,C,h,w); may alias x_in */
  const int64_t* t;         /* device; t_stride 0 => one value for every sample */
  int t_stride;
  const int64_t* y;         /* (n,) class ids, NULL for DMX_UNET */
  int64_t null_label;       /* diff.py:148 */
  const float* vals;        /* (n,12) or NULL */
  const float* mask;        /* (n,12) or NULL */
  float guidance;           /* > 0 => CFG (diff.py:147); DMX_UNET ignores it */
  const float* c1;          /* device tables [T]: (1-a)/sqrt(1-ab), sqrt(a), posterior std */
  const float* c2;
  const float* sd;
  int T;
  const float* noise;       /* (n,C,h,w) device noise, or NULL => on-device Philox */
  uint64_t seed;            /* Philox key (noise == NULL) */
  int64_t sample_offset;    /* global index of sample 0 (shard-invariant noise) */
  int n, h, w;
} dmx_step_args;

int dmx_step(dmx_model* m, const dmx_step_args* a, void* stream);

/* Run `steps` consecutive steps in place (x_in == x_out required), t taken from the
 * device scalar a->t (t_stride 0) and decremented on the device after each step; the
 * step is captured once into a hipGraph when use_graph != 0.  Noise must be NULL
 * (Philox).  This is the diff.py:332-344 loop without host round trips. */
int dmx_sample_loop(dmx_model* m, const dmx_step_args* a, int steps, int use_graph, void* stream);

/* Standalone K1 update (diff.py:151,158-162) for duck-typed foreign models:
 * eps = eu + g*(ec-eu) (ec NULL => eps = eu); x' = (x - c1*eps)/c2 + noise*sd. */
int dmx_ddpm_update(const float* x, float* x_out, const float* eu, const float* ec, float guidance,
                    const int64_t* t, int t_stride, const float* c1, const float* c2, const float* sd, int T,
                    const float* noise, uint64_t seed, int64_t sample_offset, int n, int c, int h, int w,
                    void* stream);

/* ---- strided (few-step) sampling: DDIM steps over a sub-sequence of the T timesteps -------
 * (Song et al. 2021; no reference counterpart — the reference samplers walk all T steps.)
 * A schedule of S positions: position p in [1, S] stands for the network timestep
 * t = t_map[p-1] (ascending, t_map[S-1] = T) and its step goes to s = t_map[p-2] (s = 0, with
 * alpha_bar 1, below position 1).  Row p-1 of the five fp32 tables holds
 *   k_e = sqrt(1-ab[t]), k_a = sqrt(ab[t]), k_s = sqrt(ab[s]), k_n = sigma(eta), k_d = sqrt(1-ab[s]-sigma^2)
 * and the update is  eps = eu + g*(ec-eu);  x0 = (x - k_e*eps)/k_a;  x' = k_s*x0 + k_d*eps + k_n*noise,
 * one IEEE rounding per operation in that order.  Noise is neither read nor drawn where k_n == 0;
 * Philox noise is keyed by (seed, t, global sample index) — the timestep, not the position.
 * All seven members are device pointers / counts owned by the caller. */
typedef struct dmx_ddim_sched {
  const int64_t* t_map; /* [S] int64 */
  const float* k_e;     /* [S] each */
  const float* k_a;
  const float* k_s;
  const float* k_d;
  const float* k_n;
  int S;
} dmx_ddim_sched;

/* dmx_step / dmx_sample_loop in the strided form: a->t holds POSITIONS in [1, S] (the loop
 * decrements the position scalar); a->c1, c2, sd and T are ignored and may be NULL / 0.
 * Everything else is as in the DDPM calls.  A captured graph belongs to one schedule (pointers
 * and S): another schedule, or the DDPM loop, on the same model captures anew. */
int dmx_step_ddim(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* sched, void* stream);
int dmx_sample_loop_ddim(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* sched, int steps,
                         int use_graph, void* stream);
/* Standalone strided update for duck-typed foreign models (ec NULL => eps = eu); pos: device
 * int64 positions, pos_stride 0 => one value for every sample. */
int dmx_ddim_update(const float* x, float* x_out, const float* eu, const float* ec, float guidance,
                    const int64_t* pos, int pos_stride, const dmx_ddim_sched* sched, const float* noise,
                    uint64_t seed, int64_t sample_offset, int n, int c, int h, int w, void* stream);

/* ---- DPM-Solver++(2M) over a schedule of S positions (Lu et al. 2022, Alg. 2: second-order
 * multistep, data prediction; no reference counterpart).  Positions, t_map, k_e and k_a are as in
 * dmx_ddim_sched.  With t = t_map[p-1], s = t_map[p-2] (0 below position 1), u = t_map[p] and
 * lam = log(alpha/sigma), row p-1 of the other fp32 tables holds
 *   k_x = sigma_s/sigma_t,  m = alpha_s - k_x*alpha_t,  r = (lam_t - lam_u)/(lam_s - lam_t),
 *   k_c = m*(1 + 1/(2r)), k_p = -m/(2r)   (first-order rows p = S and p = 1: k_c = m, k_p = 0)
 * and the update is  eps = eu + g*(ec-eu);  x0 = (x - k_e*eps)/k_a;  y = k_x*x + k_c*x0;
 * x' = k_p != 0 ? y + k_p*hist : y;  hist <- x0, one IEEE rounding per operation in that order.
 * hist has x's shape (n,C,h,w), must not alias x, is read only where k_p != 0 and is always
 * written: position S may start from an uninitialised buffer, and a caller entering below
 * position S must supply the x0 of position p + 1.  No noise is read or drawn at any position.
 * All members are device pointers / counts owned by the caller. */
typedef struct dmx_dpm_sched {
  const int64_t* t_map; /* [S] int64 */
  const float* k_e;     /* [S] each */
  const float* k_a;
  const float* k_x;
  const float* k_c;
  const float* k_p;
  float* hist; /* (n,C,h,w), read + written */
  int S;
} dmx_dpm_sched;

/* dmx_step / dmx_sample_loop with the DPM-Solver++(2M) update: a->t holds POSITIONS in [1, S],
 * a->noise must be NULL and a->c1, c2, sd, T and seed are not read.  A captured graph belongs to
 * one schedule (table pointers, hist and S): another schedule or history buffer, a DDIM loop or
 * the DDPM loop on the same model captures anew. */
int dmx_step_dpm(dmx_model* m, const dmx_step_args* a, const dmx_dpm_sched* sched, void* stream);
int dmx_sample_loop_dpm(dmx_model* m, const dmx_step_args* a, const dmx_dpm_sched* sched, int steps,
                        int use_graph, void* stream);
/* Standalone update for duck-typed foreign models (ec NULL => eps = eu); pos: device int64
 * positions, pos_stride 0 => one value for every sample.  x_out may alias x. */
int dmx_dpm_update(const float* x, float* x_out, const float* eu, const float* ec, float guidance,
                   const int64_t* pos, int pos_stride, const dmx_dpm_sched* sched, int n, int c, int h, int w,
                   void* stream);

/* ---- DDIM inversion: the probability-flow ODE walked upwards, from a latent z0 to the noisy latent
 * that the DDIM sampler (eta = 0) maps back to z0 (Song et al. 2021, eq. 12 with sigma = 0 solved for
 * the noisier latent; fixed-point refinement as in Pan et al. 2023, "Effective real image editing with
 * accelerated iterative diffusion inversion"; no reference counterpart).  With tau the ascending
 * timesteps of a DDIM schedule, position p = 1..p0 goes from s = tau_{p-1} (tau_0 = 0, alpha_bar 1) up
 * to t = tau_p in R + 1 rows k = 0..R, each computing
 *   eps = eu + g*(ec-eu) at (x, t_eval);   y = i_x*src + i_e*eps;   x <- y;   adv != 0: src <- y
 * one IEEE rounding per operation in that order, with
 *   i_x = sqrt(ab[t]/ab[s]),  i_e = sqrt(1-ab[t]) - i_x*sqrt(1-ab[s]),
 *   t_eval = s for k = 0 (tau_1 at p = 1: there is no timestep 0), t for k >= 1,  adv = (k == R).
 * src is the latent at the start of the position: row 0 is the plain DDIM inversion step, rows k >= 1
 * iterate y <- F(src, eps(y, t)), whose fixed point is the exact preimage of the DDIM step t -> s.  The
 * S = p0*(R+1) rows are stored in COUNTDOWN order — the counter c runs S..1 and reads row c - 1; the
 * row of (p, k) is c = S - ((p-1)*(R+1) + k) — so a->t counts down as in every other loop and t_map is
 * the t_eval column.  A caller starts with x == src == z0 (two buffers).  src has x's shape (n,C,h,w),
 * must not alias x, and each of its elements is read and written by the same lane.  No noise is read or
 * drawn.  All members are device pointers / counts owned by the caller. */
typedef struct dmx_invert_sched {
  const int64_t* t_map; /* [S] int64: t_eval per row */
  const float* i_x;     /* [S] each */
  const float* i_e;
  const int* adv;       /* [S] int32 */
  float* src;           /* (n,C,h,w), read + written */
  int S;                /* rows */
} dmx_invert_sched;

/* dmx_step / dmx_sample_loop with the inversion update: a->t holds COUNTDOWN positions in [1, S],
 * a->noise must be NULL and a->c1, c2, sd, T and seed are not read.  CFG, the one-forward step for
 * guidance 0, t_stride and ragged batches are those of the DDIM step.  There is no known region,
 * rescale, composition, geometry or perturbed-attention guidance.  A captured graph belongs to one
 * schedule (table pointers, src and S): another schedule or src buffer, or a DDIM, DPM or DDPM loop
 * on the same model captures anew. */
int dmx_step_invert(dmx_model* m, const dmx_step_args* a, const dmx_invert_sched* sched, void* stream);
int dmx_sample_loop_invert(dmx_model* m, const dmx_step_args* a, const dmx_invert_sched* sched, int steps,
                           int use_graph, void* stream);
/* Standalone update for duck-typed foreign models (ec NULL => eps = eu), any c >= 1; pos: device int64
 * countdown positions, pos_stride 0 => one value for every sample.  x_src is the source latent the update
 * reads (sched->src in a loop), sched->src receives y where adv != 0; x_out may alias
 * the x the prediction was made on, never x_src or sched->src. */
int dmx_invert_update(const float* x_src, float* x_out, const float* eu, const float* ec, float guidance,
                      const int64_t* pos, int pos_stride, const dmx_invert_sched* sched, int n, int c, int h, int w,
                      void* stream);

/* ---- Known-region sampling: img2img starts and masked inpainting (no reference counterpart).
 * z0 is a known latent and e0 one fixed Gaussian draw, both (n,C,h,w); mask is (n,h,w) in [0,1],
 * broadcast over channels, 1 = regenerate, 0 = keep.  Positions p in [1, S] and tau are those of
 * the loop the blend follows (dmx_ddim_sched / dmx_dpm_sched; the DDPM loop: tau = 1..T, S = T).
 * Row p-1 of the fp32 tables holds q_a = sqrt(ab[s]), q_e = sqrt(1 - ab[s]) for s = tau_{p-1}
 * (tau_0 = 0, ab[0] = 1: row 0 is exactly (1, 0)).  After the step at position p has produced xg,
 *   kn = q_a*z0 + q_e*e0;   x' = m == 0 ? kn : m == 1 ? xg : m*xg + (1-m)*kn
 * one IEEE rounding per operation.  The two ends of the mask are selects: a non-finite xg where
 * m != 0 cannot reach an element with m == 0, and those elements follow the forward trajectory of
 * z0 under e0 down to z0 itself at p = 1.  Nothing is drawn.  All members are device pointers /
 * counts owned by the caller and none may alias the x the blend writes. */
typedef struct dmx_known_sched {
  const float* z0;   /* (n,C,h,w) */
  const float* e0;   /* (n,C,h,w) */
  const float* mask; /* (n,h,w); NULL in dmx_known_blend: every element kept */
  const float* q_a;  /* [S] each */
  const float* q_e;
  int S;
} dmx_known_sched;

/* The blend alone (duck-typed foreign models, and the start latent).  pos: device int64 positions,
 * clamped to [1, S]; pos_stride 0 => one value for every sample.  x_out may alias x.
 * known->mask NULL: x_out = kn and x is not read (may be NULL) — with pos = p0 + 1 this is the
 * start latent sqrt(ab[tau_p0])*z0 + sqrt(1-ab[tau_p0])*e0 of a loop entering at p0 < S. */
int dmx_known_blend(const float* x, float* x_out, const int64_t* pos, int pos_stride,
                    const dmx_known_sched* known, int n, int c, int h, int w, void* stream);
/* dmx_step* / dmx_sample_loop* with the blend launched after the step's tail, reading the position
 * the tail read and rewriting a->x_out in place.  At most one of ddim / dpm is non-NULL; both NULL:
 * the DDPM step.  known->S must equal the schedule's S (a->T for DDPM) and known->mask must be
 * given.  A captured graph belongs to one dmx_known_sched as it belongs to one schedule: the
 * plain loops never replay a known-region graph, nor the reverse. */
int dmx_step_known(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim, const dmx_dpm_sched* dpm,
                   const dmx_known_sched* known, void* stream);
int dmx_sample_loop_known(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim,
                          const dmx_dpm_sched* dpm, const dmx_known_sched* known, int steps, int use_graph,
                          void* stream);

/* ---- Guidance controls of a CFG step beyond its scale (no reference counterpart).
 * rescale = phi in [0, 1] (Lin et al. 2023, "Common diffusion noise schedules and sample steps are
 * flawed", §3.4): with eu / ec the unconditional / conditional predictions and
 * eg = eu + g*(ec-eu) the guided one (one IEEE rounding per operation, as in every step), each
 * sample n is scaled over its C*h*w elements by
 *   r[n] = 1 + phi*(std(ec[n]) / std(eg[n]) - 1);   eps = eg * r[n]
 * before the DDPM / DDIM / DPM update.  The moments are accumulated in double in a fixed order
 * from the fp32 values (per-block mean and centred sum of squares, combined in block order about
 * the sample mean), r is formed in double and rounded to fp32 once, and r[n] = 1 where std(eg[n]) is not a
 * positive finite number.  A sample's result does not depend on the batch it sits in.  A
 * non-finite eg raises the range flag as in the plain step.  phi = 0 is the plain step.
 * (The guidance interval of the samplers needs no ABI: a step outside it is the plain step with
 * guidance 0 and y given, one conditional forward.) */
typedef struct dmx_guidance {
  float rescale;
} dmx_guidance;

/* dmx_step* / dmx_sample_loop* with the guidance controls: at most one of ddim / dpm is non-NULL
 * (both NULL: the DDPM step), known may be NULL (no blend), guidance must be given.  With
 * rescale > 0 the step must be a CFG step (a->guidance > 0, a->y given, a conditional model); its
 * single tail launch becomes three (head + CFG mix + block moments; ratio + scale; update), whose
 * workspace is part of the model's planned arena.  With rescale == 0 both calls are exactly the
 * plain / known-region calls and share their graphs. */
int dmx_step_guided(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim, const dmx_dpm_sched* dpm,
                    const dmx_known_sched* known, const dmx_guidance* guidance, void* stream);
int dmx_sample_loop_guided(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim,
                           const dmx_dpm_sched* dpm, const dmx_known_sched* known, const dmx_guidance* guidance,
                           int steps, int use_graph, void* stream);
/* The CFG mix and rescale alone, for duck-typed foreign models (no model, no arena): eu, ec, eps_out
 * (n,c,h,w) with any c, h, w >= 1; ratio_out (n,) receives r or is NULL; eps_out may alias eu or ec.
 * One block per sample: mean, then centred squares, then the scaling, each reduction in a fixed
 * order in double.  Feed eps_out to dmx_*_update with ec = NULL. */
int dmx_cfg_rescale(const float* eu, const float* ec, float guidance, float rescale, float* eps_out,
                    float* ratio_out, int n, int c, int h, int w, void* stream);

/* ---- Composed guidance: K weighted condition branches over a chosen base branch (Liu et al. 2022,
 * "Compositional visual generation with composable diffusion models"; no reference counterpart).
 * Branch 0 is the base, branches 1..K the conditions, 1 <= K <= DMX_COMPOSE_MAX.  Branch k of sample
 * i has the label y[k][i], the numeric row vals[k][i][:] and the mask row mask[k][i][:] (width 12);
 * the step runs one (K+1)*n-sample forward whose row k*n + i is branch k of sample i (x and t are
 * shared by the branches, and so is the part of the network before the first embedding add).  With
 * e_k the prediction of branch k and w_k[i] = weight[k-1][i] (finite fp32; zero and negative legal)
 *   d_k = e_k - e_0;  s = w_1*d_1;  s = s + w_k*d_k (k = 2..K);  eps = e_0 + s
 * one IEEE rounding per operation in that order, then the DDPM / DDIM / DPM update and, if asked
 * for, the known-region blend, both as in every step.  K = 1 with a constant weight g, base label
 * null_label and the call's vals / mask is bit for bit the plain CFG step; a weight per sample is
 * a per-sample guidance scale; a base row (null label, vals = mask = 0) is the input the model's
 * joint condition dropout trained as unconditional; any other base row is a negative condition.
 * A non-finite eps raises the range flag.  All members are device pointers owned by the caller;
 * none may alias the x the step writes. */
#define DMX_COMPOSE_MAX 4
typedef struct dmx_compose {
  int K;               /* 1 .. DMX_COMPOSE_MAX */
  const int64_t* y;    /* [(K+1)][n], row 0 = base branch */
  const float* vals;   /* [(K+1)][n][12], or NULL together with mask */
  const float* mask;
  const float* weight; /* [K][n] */
} dmx_compose;

/* The general step and loop entries: at most one of ddim / dpm is non-NULL (both NULL: the DDPM
 * step); known, guidance and compose may each be NULL.  With compose == NULL they are
 * dmx_step_guided / dmx_sample_loop_guided (which forward here), guidance == NULL standing for
 * rescale 0.  With compose given the model must be conditional, a->n <= 65535, guidance must be
 * NULL or have rescale == 0, and a->y, a->vals, a->mask, a->guidance and a->null_label are not
 * read.  A composed loop's graphs belong to its dmx_compose (K and the four pointers) as they
 * belong to a schedule: plain loops never replay them, nor the reverse. */
int dmx_step_composed(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim, const dmx_dpm_sched* dpm,
                      const dmx_known_sched* known, const dmx_guidance* guidance, const dmx_compose* compose,
                      void* stream);
int dmx_sample_loop_composed(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim,
                             const dmx_dpm_sched* dpm, const dmx_known_sched* known, const dmx_guidance* guidance,
                             const dmx_compose* compose, int steps, int use_graph, void* stream);
/* The mix alone, for duck-typed foreign models (no model, no arena): e [(K+1)][n][c][h][w] (NCHW per
 * branch, branch-major), weight [K][n], eps_out (n,c,h,w) with any c, h, w >= 1; eps_out may alias a
 * branch of e.  Feed eps_out to dmx_*_update with ec = NULL. */
int dmx_compose_eps(const float* e, const float* weight, int K, int n, int c, int h, int w, float* eps_out,
                    void* stream);

/* ---- Geometry guidance: classifier guidance by the GeomHead's input gradient (Dhariwal & Nichol
 * 2021, §4.1, DDIM form; no reference counterpart).  DMX_UNET_COND_GEOM regresses the geom_dim
 * geometry values from the noisy latent at every timestep; with geom = its output on the step's
 * conditional input (a->y, a->vals, a->mask) and the target the step's own a->vals / a->mask,
 *   L_n = sum_j m_nj (geom_nj - v_nj)^2 / max(sum_j m_nj, 1e-6)
 *   eps' = eps + (scale[n] * sig[p-1]) * dL_n/dx
 * where eps is the CFG-guided prediction, p the step's position and sig[p-1] = sqrt(1 - ab[t]) of
 * its timestep (per position, as the schedule's tables; the DDPM step: per timestep, S = T).  One
 * IEEE rounding per operation: the scale product, its product with the gradient, the sum.  Where
 * scale[n] == 0 or the gradient element is exactly zero, eps' has eps's bits; a row whose mask is
 * all zero has an exactly zero gradient.  A non-finite eps' raises the range flag.  Both tables are
 * device pointers owned by the caller. */
typedef struct dmx_geom_guide {
  const float* scale; /* (n,) device */
  const float* sig;   /* per position */
  int S;
} dmx_geom_guide;

/* dmx_step* / dmx_sample_loop* with geometry guidance: at most one of ddim / dpm is non-NULL (both
 * NULL: the DDPM step), known may be NULL, geom must be given with S equal to the schedule's
 * (a->T for DDPM).  The model must be DMX_UNET_COND_GEOM and the step a CFG step with a condition
 * (a->guidance > 0, a->y, a->vals and a->mask given); there is no rescale and no composition.
 * Every step runs the 2n CFG forward, the taped training forward of the n conditional rows (fp32
 * semantics, as dmx_train_forward; it reads the step's position scalar), the loss seed, the
 * data-only backward to x (dmx_train_backward_input's launches), the mix and the rule's update on
 * the mixed prediction, then the blend if asked for; all of it inside the model's planned arena,
 * so the loop is captured like every other.  The model's training tape is replaced: a
 * dmx_train_backward still pending on an earlier dmx_train_forward is refused as stale. */
int dmx_step_geom(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim, const dmx_dpm_sched* dpm,
                  const dmx_known_sched* known, const dmx_geom_guide* geom, void* stream);
int dmx_sample_loop_geom(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim, const dmx_dpm_sched* dpm,
                         const dmx_known_sched* known, const dmx_geom_guide* geom, int steps, int use_graph,
                         void* stream);
/* The mix alone, for duck-typed foreign models (no model, no arena): eps, grad, eps_out (n,c,h,w)
 * with any c, h, w >= 1; scale (n,); sig [S]; pos: device int64 positions clamped to [1, S],
 * pos_stride 0 => one value for every sample.  eps_out may alias eps.  Feed eps_out to
 * dmx_*_update with ec = NULL. */
int dmx_geom_mix(const float* eps, const float* grad, const float* scale, const float* sig, int S,
                 const int64_t* pos, int pos_stride, float* eps_out, int n, int c, int h, int w, void* stream);
/* The loss and its seed alone: geom, vals, mask, seed_out (n,gd); loss_out (n,) or NULL.
 * seed_out[n][j] = dL_n/dgeom_nj = 2 m_nj (geom_nj - v_nj) / max(sum_j m_nj, 1e-6) — what
 * dmx_train_backward_input takes as d_geom. */
int dmx_geom_seed(const float* geom, const float* vals, const float* mask, int n, int gd, float* loss_out,
                  float* seed_out, void* stream);

/* ---- Perturbed-attention guidance: an identity-attention branch in a composed step (Ahn et al. 2024,
 * "Self-rectifying diffusion sampling with perturbed-attention guidance"; no reference counterpart).
 * In a perturbed branch the self-attention of the chosen blocks is replaced by the identity: the
 * softmax matrix is I, so a token's attention output is its own value vector (the V third of the
 * in_proj output, bias included); out_proj, the residual and the feed-forward run as always.  Bit i
 * of `blocks` stands for the block sa(i+1), i = 0..5 (sa1..sa3 the down path, sa4..sa6 the up path);
 * it must be non-zero and below 64.  Bit k of `branches` marks branch k of the composition (0 = the
 * base) as perturbed; the set bits must form a non-empty run k0..K, the trailing branches, so that
 * the perturbed rows [k0*n, (K+1)*n) of the branch-major forward are one range.  The mix is the
 * composition's, unchanged: with branch K the main condition's rows again, perturbed, weight -s on
 * it and g + s on the main branch, eps = e_u + g (e_c - e_u) + s (e_c - e_p).  Rows of unperturbed
 * branches keep the bits they have without the struct; a perturbed row skips the attention core of
 * the chosen blocks (an exact fp32 copy in every precision mode). */
typedef struct dmx_perturb {
  uint32_t blocks;   /* bit i: sa(i+1); 1 .. 63 */
  uint32_t branches; /* bit k: branch k; a trailing run of 0 .. K */
} dmx_perturb;

/* The general step and loop entries: every part of dmx_step_composed / dmx_sample_loop_composed
 * (which forward here with perturb == NULL) plus perturb, which may be NULL.  With perturb given
 * compose must be given, and there is no rescale (as in every composed step) and no geometry
 * guidance.  A perturbed loop's graphs belong to its dmx_perturb as they belong to its
 * composition: composed loops never replay them, nor the reverse. */
int dmx_step_perturbed(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim, const dmx_dpm_sched* dpm,
                       const dmx_known_sched* known, const dmx_guidance* guidance, const dmx_compose* compose,
                       const dmx_perturb* perturb, void* stream);
int dmx_sample_loop_perturbed(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim,
                              const dmx_dpm_sched* dpm, const dmx_known_sched* known, const dmx_guidance* guidance,
                              const dmx_compose* compose, const dmx_perturb* perturb, int steps, int use_graph,
                              void* stream);
/* dmx_unet_forward with the samples [row0, row1) perturbed in the blocks of `blocks` (0 <= row0 <
 * row1 <= n, blocks in 1..63): the other samples' outputs have the bits dmx_unet_forward gives them. */
int dmx_unet_forward_perturbed(dmx_model* m, const float* x, const int64_t* t, const int64_t* y, const float* vals,
                               const float* mask, float* eps, float* geom, int n, int h, int w, uint32_t blocks,
                               int row0, int row1, void* stream);
/* The identity core alone: qkv (n,L,3C) = q | k | v -> out (n,L,C) = v, an exact fp32 copy.
 * C in {64, 128, 256}; n, L >= 1; n*L*C < 2^41. */
int dmx_attn_identity(const float* qkv, float* out, int n, int L, int C, void* stream);

/* ---- Feature caching: reuse the deep U-Net feature between steps (DeepCache, Ma et al. 2024; no
 * reference counterpart).  The deep feature D is the output of sa5 — up3's upsampled input,
 * (rows, h/2, w/2, 64) fp32 in the engine's layout, rows = 2n in a CFG step (null half first) and n in
 * an unguided one.  Step k of a call (k = 0 in the one-step entry) is a REFRESH step iff
 * (phase + k) % interval == 0: the plain step, bit for bit, which also leaves D in a buffer the model
 * owns (outside its workspace, allocated on first use; sa5's last launch writes there, so a refresh
 * step launches what the plain step launches).  Every other step is a REUSE step: the embedding, inc
 * (once for the n shared rows under CFG batching), then up3 and sa6 on the stored D, the head and the
 * same tail — nothing between inc and up3 is launched.  An approximation: the stored D belongs to an
 * earlier x and t.  NULL or interval <= 1 is the plain call and shares its graphs. */
typedef struct dmx_cache {
  int interval; /* N: a refresh every N-th step; <= 1: no caching */
  int phase;    /* >= 0: the call's first step stands at this offset of the cycle */
} dmx_cache;

/* dmx_step_guided / dmx_sample_loop_guided with the cache request: at most one of ddim / dpm is
 * non-NULL (both NULL: the DDPM step), known and guidance may be NULL.  A cached step takes no
 * composition, perturbed-attention guidance, geometry guidance or inversion (these entries have no
 * such argument; the rule is DMX_E_ARG wherever the parts could meet).  The model records what D
 * belongs to — rows, n, h, w, the precision mode and the generation of the weights (finalize /
 * dmx_model_refresh start a new one) — and a reuse step without a matching D is DMX_E_STATE, naming
 * the part that differs, before anything is launched.  A cached loop keeps two captured graphs, one
 * per step kind, each a one-step graph, and replays them in the pattern; dmx_model_graph_captures
 * counts each.  Reallocating the D buffer (more rows, a larger map) drops every captured graph. */
int dmx_step_cached(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim, const dmx_dpm_sched* dpm,
                    const dmx_known_sched* known, const dmx_guidance* guidance, const dmx_cache* cache,
                    void* stream);
int dmx_sample_loop_cached(dmx_model* m, const dmx_step_args* a, const dmx_ddim_sched* ddim,
                           const dmx_dpm_sched* dpm, const dmx_known_sched* known, const dmx_guidance* guidance,
                           const dmx_cache* cache, int steps, int use_graph, void* stream);
/* Diagnostic: what the D buffer holds.  shape_out[4] receives (rows, h/2, w/2, 64) — all zero when no
 * valid D is stored; dst (NULL: shape only) receives the rows*(h/2)*(w/2)*64 floats in that layout,
 * copied on `stream`, which is synchronised. */
int dmx_model_cached_features(dmx_model* m, int64_t* shape_out, float* dst, void* stream);

/* Captured sample-loop graphs.  A model keeps the graph pairs (1-step and 8-step) of the last 4
 * distinct loops (distinct dmx_step_args / schedule / inversion / known region / guidance / composition / perturbation / geometry guidance / time-table
 * generation) and evicts the least recently used, so a sampler that alternates unguided, guided
 * and rescaled segments captures each kind once.  All pairs replay on the caller's stream, one
 * after another, inside the model's one workspace; whatever reallocates or invalidates it (a
 * larger batch, dmx_model_set_precision to another mode, dmx_model_refresh) drops every pair.
 * A feature-cached loop (dmx_sample_loop_cached, interval > 1) takes two of the slots, one per step
 * kind, each holding a one-step graph only and each counted as one capture.
 * Returns the number of pairs captured since the model was created (-1: NULL model). */
int64_t dmx_model_graph_captures(const dmx_model* m);

/* ---- VAE decode (replaces VAE.decode, vae.py:64-69, plus Diffuser.reverse_to_img's
 * x*255 -> clamp -> uint8, diff.py:58-62) ---------------------------------------------
 * z: (n,4,h,w); img: (n,3,8h,8w) fp32 or NULL; u8: (n,8h,8w,3) uint8 (HWC) or NULL. */
int dmx_vae_decode(dmx_model* m, const float* z, float* img, uint8_t* u8, int n, int h, int w, void* stream);

/* ---- latent-channel frames (replaces generate_steps.py:47-64 save_latent_channels_by_dir's
 * per-channel min-max -> *255 -> uint8 before the PNG write) ---------------------------------
 * z: (n,c,h,w) fp32 device; out: (n,c,h,w) uint8 device, byte-identical to the reference's. */
int dmx_latent_frames_u8(const float* z, uint8_t* out, int n, int c, int h, int w, void* stream);

/* ---- generated-image metrics (replaces eval_iou_noise.py:77-94 binarisation and 162-272
 * distance transform / compute_metrics) ------------------------------
 * gt, pred: (n,h,w) uint8 device — masks (0 / nonzero; gray = 0) or grayscale images binarised
 * here (gray = 1: foreground = v < threshold if invert else v >= threshold); h, w <= 16384.
 * workspace: n*h*w int32 device scratch; out: (n,9) float64 device =
 * {iou, gt_iou, far_noise_ratio, gauss_recall, inter, union, gt_area, pred_area, fp}. */
int dmx_eval_metrics(const uint8_t* gt, const uint8_t* pred, int n, int h, int w, int gray, int threshold, int invert,
                     double sigma, int* workspace, double* out, void* stream);

/* ---- VAE encode (replaces VAE.encode, vae.py:51-62) -------------
 * x: (n,3,h,w) fp32, h and w multiples of 8; eps: (n,4,h/8,w/8) = the reference's
 * torch.randn_like(std) draw (caller-drawn, so the global RNG stream matches);
 * z: (n,4,h/8,w/8) = (mu + eps * exp(0.5 logvar)) * 0.18215; kl: (n,) per-sample KL term
 * (VAE.encode's returned kl is kl.mean()). */
int dmx_vae_encode(dmx_model* m, const float* x, const float* eps, float* z, float* kl, int n, int h, int w,
                   void* stream);

/* ---- training step (replaces the forward + loss.backward() of UnetCondWithGeomHead / UnetCond
 * in train_latent_cond.py:148-162) ------------------------------------
 * dmx_train_forward: model(x, t, y, cond_vals, cond_mask) with fp32 semantics (x3 split GEMMs with
 * device-side scales whatever the model's precision), recording the activations the backward needs in a tape owned by the
 * model; x: (n,in_ch,h,w); t, y: (n,) int64 (t in [1, tmax], y in [0, num_classes]);
 * vals/mask: (n,12) or NULL; eps: (n,in_ch,h,w) out; geom: (n,geom_dim) out or NULL.
 * *tape_id identifies the tape (one per model: a later forward replaces it).
 * dmx_train_backward: d_eps (n,in_ch,h,w) = dLoss/deps, d_geom (n,geom_dim) = dLoss/dgeom
 * (either may be NULL = zero); writes dLoss/dparam for every state_dict key into grads[i]
 * (one device pointer per key in dmx_model_cfg_key order, each of that key's shape; keys whose
 * branch did not run — cond_mlp without vals — receive zeros).  The gradient for x is
 * dmx_train_backward_input's.
 * dmx_train_backward_input: the same tape rules and cotangents; writes d_x (n,in_ch,h,w) = the
 * vector-Jacobian product with respect to the taped forward's x and nothing else — no parameter
 * gradient is computed and no gradient buffer is needed (the weight-gradient GEMMs, bias and
 * affine sums and the whole embedding backward are not launched).  It leaves the tape as it found
 * it: a dmx_train_backward on the same tape afterwards gives the bits it gives without. */
int dmx_train_forward(dmx_model* m, const float* x, const int64_t* t, const int64_t* y, const float* vals,
                      const float* mask, int n, int h, int w, float* eps, float* geom, int64_t* tape_id,
                      void* stream);
int dmx_train_backward(dmx_model* m, int64_t tape_id, const float* d_eps, const float* d_geom, float* const* grads,
                       int n_grads, void* stream);
int dmx_train_backward_input(dmx_model* m, int64_t tape_id, const float* d_eps, const float* d_geom, float* d_x,
                             void* stream);

/* ---- VAE training step (replaces the forward + loss.backward() of VAE.forward in train_vae.py,
 * models/vae.py:51-76; widths 3 / 4 / 64, image sides multiples of 8) -------------------------------
 * dmx_vae_train_forward: what dmx_vae_encode followed by dmx_vae_decode computes, with fp32 semantics
 * (x3 split GEMMs with device-side weight scales whatever the model's precision, as
 * dmx_train_forward), recording a tape owned by the model (raw conv outputs, GroupNorm(8) statistics
 * per (sample, group), activations, mu, logvar, the sigmoid output; one tape per model: a later forward
 * replaces it).  x: (n,3,h,w); eps: (n,4,h/8,w/8) = the caller's randn draw; x_recon: (n,3,h,w) out;
 * z: (n,4,h/8,w/8) out; kl: (n,) per-sample KL out.  n * h * w < 2^24.
 * dmx_vae_train_backward: d_recon (n,3,h,w), d_z (n,4,h/8,w/8), d_kl (n,) — the cotangents of the
 * three outputs, any of them NULL = zero; writes dLoss/dparam for every state_dict key into grads[i]
 * (dmx_model_cfg_key order).  No gradient for x.  Every reduction runs in a fixed order: the same
 * step twice gives bit-identical gradients. */
int dmx_vae_train_forward(dmx_model* m, const float* x, const float* eps, int n, int h, int w, float* x_recon, float* z,
                          float* kl, int64_t* tape_id, void* stream);
int dmx_vae_train_backward(dmx_model* m, int64_t tape_id, const float* d_recon, const float* d_z, const float* d_kl,
                           float* const* grads, int n_grads, void* stream);

/* ---- measurement: one eager step with a HIP event pair around every launch -----------
 * Fills up to `cap` records (kernel name as rocprofv3 shows it, layer label, algorithmic
 * FLOPs and HBM bytes of that launch, and its event-timed duration in ms). */
typedef struct dmx_kernel_record {
  char kernel[96];
  char layer[48];
  double flops;
  double bytes;
  float ms;
} dmx_kernel_record;

int dmx_step_profile(dmx_model* m, const dmx_step_args* a, dmx_kernel_record* recs, int cap, int* n_out,
                     void* stream);

/* ---- debugging: with taps enabled, dmx_unet_forward records every block output
 * (NHWC, inside the workspace) so they can be copied out and compared layer by layer. */
int dmx_debug_enable(dmx_model* m, int on);
int dmx_debug_num_taps(const dmx_model* m);
int dmx_debug_tap(dmx_model* m, int i, char* name_out, int cap, int64_t* count_out, float* dst, void* stream);

/* ---- multi-head attention core backward (the adjoint of nn.MultiheadAttention's softmax(Q K^T /
 * sqrt(D)) V core, models/unet_cond.py:36,49, 4 heads; used by dmx_train_backward, exported for its
 * test): qkv (n,L,3C) = q | k | v (head h at columns h*C/4), o = the core's output (n,L,C), dout =
 * dLoss/do (n,L,C); writes dLoss/dqkv (n,L,3C).  C/4 in {16, 32, 64}; all device fp32. */
int dmx_attn_core_backward(const float* qkv, const float* o, const float* dout, float* dqkv, int n, int L, int C,
                           void* stream);

/* ---- timing diagnostic (libraries built with -DDMX_DIAG=1 only; regular builds return 0): the
 * per-block s_memtime stamps of the Winograd conv launches ({start, after prologue, after chunk loop,
 * end, hardware id} x 2048 blocks x 32 launch slots, uint64) copied to host memory; returns the count
 * copied or -1; host == NULL resets the table and the launch counter.  tools/wino_stamps.py reads them. */
int dmx_diag_wino_stamps(unsigned long long* host, int cap);

/* Bytes of device workspace currently held by a model (diagnostics): the inference workspace plus,
 * once a training step ran, the tape and the backward workspace. */
int64_t dmx_model_workspace_bytes(const dmx_model* m);

/* ---- optimizer step (replaces torch.optim.Adam's step of train_latent_cond.py:99,163 and train_vae.py):
 * fused multi-tensor Adam / AdamW with global-norm gradient clipping and an exponential moving average
 * of the weights, over any list of contiguous fp32 device tensors.  Independent of dmx_model.
 *
 * The tensor list is cut once into chunks of at most DMX_OPTIM_CHUNK elements (one kernel block per
 * chunk).  Every step the caller passes one row per tensor: the pointers (gradient pointers change every
 * step) and that tensor's own coefficients, all computed on the host in double and rounded once:
 *   step_size = lr / (1 - beta1^step), inv_sqrt_bc2 = 1 / sqrt(1 - beta2^step), lr_wd = lr * weight_decay,
 *   wd = weight_decay (coupled decay; 0 in a decoupled row), omb1 = 1 - beta1, omb2 = 1 - beta2.
 * A row with g == NULL is skipped (torch: .grad is None).  Per element, in fp32, torch/optim/adam.py's
 * single-tensor rule:
 *   g' = coef g (+ wd p);  decoupled: p -= lr_wd p;  m += (g' - m) omb1;  v = beta2 v + omb2 g' g';
 *   p -= step_size m / (sqrt(v) inv_sqrt_bc2 + eps);  ema != NULL: ema = d ema + (1 - d) p.
 * The gradient buffers are only read. */
#define DMX_OPTIM_CHUNK 4096
#define DMX_OPTIM_ALIGNED 1u   /* set by dmx_optim_set_step: p, g, m, v, ema all 16-byte aligned */
#define DMX_OPTIM_DECOUPLED 2u /* AdamW: the decay multiplies p and does not enter the gradient */

typedef struct dmx_optim dmx_optim;

typedef struct dmx_optim_chunk {
  int64_t offset; /* first element, a multiple of DMX_OPTIM_CHUNK */
  int32_t tensor;
  int32_t len;    /* 1 .. DMX_OPTIM_CHUNK */
} dmx_optim_chunk;

typedef struct dmx_optim_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* ema;
  float step_size, inv_sqrt_bc2, lr_wd, eps;
  float wd, omb1, beta2, omb2;
  uint32_t flags;
  uint32_t reserved;
} dmx_optim_tensor;

/* The chunk table of n tensors with numel[i] elements (host only, no device needed): writes up to cap
 * chunks to out (NULL: count only) and returns the number of chunks, or -1. */
int64_t dmx_optim_chunks(int n, const int64_t* numel, dmx_optim_chunk* out, int64_t cap);

int dmx_optim_create(int device, int n, const int64_t* numel, dmx_optim** out);
int dmx_optim_destroy(dmx_optim* o);

/* The rows of the next step: copied into pinned host memory and uploaded with one asynchronous copy on
 * `stream`.  The staging buffers form a ring; one is rewritten only after the step that read it has
 * finished on the device (an event recorded behind that step), so the host waits only when it runs a
 * whole ring of steps ahead of the device. */
int dmx_optim_set_step(dmx_optim* o, const dmx_optim_tensor* rows, int n, void* stream);

/* One step over the rows last set, enqueued on `stream`; no host synchronisation.  max_norm > 0 with
 * norm_out (device, 2 floats) clips by the global gradient norm: norm_out[0] = the norm before clipping,
 * norm_out[1] = coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_'s rule); sums in
 * a fixed order, no atomics.  ema_d / ema_omd = d and 1 - d of the weight average (read where a row's ema
 * is set).  A set of rows is consumed by one step. */
int dmx_optim_step(dmx_optim* o, float max_norm, float ema_d, float ema_omd, float* norm_out, void* stream);

/* ---- training objective (replaces the torch ops around the network in train_latent_cond.py:136-159:
 * the timestep draw, diff.py:18-30 add_noise, the CFG dropout of label / values / mask, F.mse_loss,
 * masked_geom_mse and the autograd walk back to dLoss/deps, dLoss/dgeom).  Stateless: device pointers
 * and a stream, no model handle, so the pieces also serve a foreign model.  All tensors contiguous.
 *
 * dmx_train_noise, per sample n of B and element i of its C*h*w:
 *   z_noisy = sa[t_n - 1] * z + s1[t_n - 1] * noise       (sa = sqrt(ab), s1 = sqrt(1 - ab), [T] fp32,
 *                                                           tabulated by the caller)
 * two products and a sum, one IEEE rounding each, never contracted: given t and noise the result has
 * the bits of torch's expression.  y_used[n] = drop_n ? null_label : y[n]; vals_used / mask_used =
 * the rows of vals / mask, exactly zero where drop_n (kept rows bit for bit).
 * t, noise and drop are each read, or, where its bit of `draw` is set (DMX_DRAWS_T, DMX_DRAWS_NOISE,
 * DMX_DRAWS_DROP), written.  Read: drop == NULL drops nothing; a t outside [1, T] is clamped for the
 * table reads (the caller checks its range).  Written: drawn by Philox4x32-10 under `seed`, with
 * g = sample_offset + n the row's index in the global batch and Q = ceil(C*h*w / 4):
 *   noise[n][4q .. 4q+3] = the four normals of counter (DMX_DRAW_NOISE, g * Q + q)
 *   t_n    = 1 + floor(word0(DMX_DRAW_T, g) * T / 2^32)        (multiply-high; bias <= T / 2^32)
 *   drop_n = (word0(DMX_DRAW_DROP, g) >> 8) * 2^-24 < cfg_drop_prob   (0 drops none, 1 drops all)
 * so a rank that holds rows [k, k + B) of a global batch draws exactly those rows' values.
 * y, vals, mask may be NULL (then y_used / vals_used / mask_used are not written); gd = row width. */
#define DMX_DRAW_NOISE 0x8000000000000001ull
#define DMX_DRAW_T 0x8000000000000002ull
#define DMX_DRAW_DROP 0x8000000000000003ull
#define DMX_DRAWS_T 1
#define DMX_DRAWS_NOISE 2
#define DMX_DRAWS_DROP 4

typedef struct dmx_noise_args {
  const float* z;      /* (B,C,h,w) */
  const float* sa;     /* [T], index t - 1 */
  const float* s1;
  int T;
  int draw;            /* DMX_DRAWS_* bits */
  int64_t* t;          /* (B,) */
  float* noise;        /* (B,C,h,w) */
  uint8_t* drop;       /* (B,) 0 / 1 */
  uint64_t seed;
  int64_t sample_offset;
  float cfg_drop_prob; /* in [0, 1]; read when drop is drawn */
  int gd;
  const int64_t* y;    /* (B,) or NULL */
  int64_t null_label;
  const float* vals;   /* (B,gd) or NULL together with mask */
  const float* mask;
  float* z_noisy;      /* (B,C,h,w) */
  int64_t* y_used;
  float* vals_used;
  float* mask_used;
  int B, C, h, w;
} dmx_noise_args;

int dmx_train_noise(const dmx_noise_args* a, void* stream);
/* dmx_train_noise plus the v-prediction target of the same draws, in the same launch:
 *   target = sa[t_n - 1] * noise - s1[t_n - 1] * z          ((B,C,h,w); two products and a difference,
 *                                                             one rounding each, never contracted)
 * Every other output has dmx_train_noise's bits.  dmx_objective_loss / dmx_objective_seed then take
 * `target` where they take `noise`. */
int dmx_train_noise_target(const dmx_noise_args* a, float* target, void* stream);

/* dmx_objective_loss: with N = C*h*w, w_n = weight[t_n - 1] (weight == NULL: 1), g / v / m the rows of
 * geom / vals / mask (geom == NULL: no geometry term, gd not read)
 *   per_sample[n] = w_n * sum_i (eps - noise)^2 / N         noise_loss = sum_n per_sample[n] / B
 *   geom_loss = sum m (g - v)^2 / max(denom, 1e-6)          denom = *denom if given, else sum m
 *   loss = noise_loss + geom_lambda * geom_loss
 * Differences, squares and the mask product are fp32 with one rounding each; every sum is double in a
 * fixed order (one block per sample, then the B partials in index order in one block), each result
 * rounded to fp32 once: the same bits from run to run, no atomics.  out[0..3] = loss, noise_loss,
 * geom_loss, max(denom, 1e-6).  part: B * 3 doubles of scratch.
 * dmx_objective_seed: the gradient of `loss` scaled by the upstream scalar *up (a device pointer:
 * no host synchronisation), reading out[3] of the dmx_objective_loss call on the same arguments
 *   d_eps[n][i]  = (up * 2 w_n / (B N)) * (eps - noise)
 *   d_geom[n][j] = (up * geom_lambda * 2 / max(denom, 1e-6)) * (m * (g - v))      (d_geom NULL: skipped)
 * each coefficient formed in double and rounded once.  Both feed dmx_train_backward. */
typedef struct dmx_objective_args {
  const float* eps;    /* (B,C,h,w) */
  const float* noise;
  const int64_t* t;    /* (B,), read where weight is given */
  const float* weight; /* [T], index t - 1, or NULL */
  int T;
  const float* geom;   /* (B,gd) or NULL */
  const float* vals;
  const float* mask;
  int gd;
  const float* denom;  /* one device float or NULL */
  float geom_lambda;   /* finite, >= 0 */
  double* part;
  float* per_sample;   /* (B,) */
  float* out;          /* [4] */
  int B, C, h, w;
} dmx_objective_args;

int dmx_objective_loss(const dmx_objective_args* a, void* stream);
int dmx_objective_seed(const dmx_objective_args* a, const float* up, float* d_eps, float* d_geom, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMX_H_ */
