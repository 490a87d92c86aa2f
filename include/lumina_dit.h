/*
 * lumina_dit.h -- C ABI of the MI355X (gfx950) Next-DiT / Flag-DiT denoising engine.
 *
 * The reference (Alpha-VLLM/Lumina-T2X) has NO plugin / FFI interface: the hot path sits behind two
 * Python conventions:
 *   1. the model-callable protocol  model_fn(x[B,C,H,W], t[B], **kw) -> [B,C,H,W]
 *      (lumina_next_t2i/transport/transport.py:192-195, integrators.py:104-116), concretely
 *      NextDiT.forward_with_cfg (lumina_next_t2i/models/model.py:866-913) and
 *      NextDiT.forward (model.py:836-864);
 *   2. module construction + state_dict key contract (lumina_next_t2i/sample.py:125-142).
 * This header is what a ctypes / cffi / pybind stub on the reference side would bind to replace the
 * body of those two methods and of transport/integrators.py:ode.sample (integrators.py:104-116).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; lt_last_error() gives the message
 *     (thread-local, valid until the next call on the same thread).  No C++ exception crosses the ABI.
 *   - all pointers named *_dev are DEVICE pointers owned by the caller (PyTorch in our host code);
 *     the engine never frees or retains them beyond the call, except where stated.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  No call synchronises the
 *     stream or the device; nothing inside the denoising loop reads device data on the host.
 *   - dtype codes: LT_F32 = 0, LT_BF16 = 1, LT_F16 = 2 (f16 only accepted for weights upload).
 */
#ifndef LUMINA_DIT_H
#define LUMINA_DIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_F32 0
#define LT_BF16 1
#define LT_F16 2

/* model variants (which reference class the engine reproduces) */
#define LT_VARIANT_NEXT_T2I 0      /* lumina_next_t2i/models/model.py:665 NextDiT              */
#define LT_VARIANT_NEXT_IMAGENET 1 /* Next-DiT-ImageNet/models/models.py:836 DiT_Llama         */
#define LT_VARIANT_FLAG_T2I 2      /* lumina_t2i/models/model.py:661 DiT_Llama (Flag-DiT)      */
#define LT_VARIANT_NEXT_MOE 3      /* Next-DiT-MoE/models/models2.py:850 DiT_Llama (time+space MoE) */
#define LT_VARIANT_NEXT_MOE_TIME 4  /* Next-DiT-MoE/models/models.py:802 DiT_Llama: ONE MoE FFN per block, routed by the timestep
                                       embedding (every token of a sample visits the same two experts; models.py:459-477)  */
#define LT_VARIANT_NEXT_MOE_SPACE 5 /* Next-DiT-MoE/models/models1.py:802 DiT_Llama: ONE MoE FFN per block, routed per token   */

/* fixed-grid ODE methods, torchdiffeq names (lumina_next_t2i/transport/integrators.py:115) */
/* lt_set_softmax_rule: the self-attention softmax scale under proportional attention */
#define LT_SOFTMAX_T2I 0     /* sqrt(log(N, base_seqlen) / head_dim)   lumina_next_t2i/models/model.py:374 (default)   */
#define LT_SOFTMAX_ANAGRAM 1 /* log(N, base_seqlen) / sqrt(head_dim)   visual_anagrams/models/nextdit.py:333           */

#define LT_ODE_EULER 0
#define LT_ODE_MIDPOINT 1
#define LT_ODE_RK4 2
/* adaptive Runge-Kutta methods of lt_sample_ode_adaptive, torchdiffeq names */
#define LT_ODE_DOPRI5 3
#define LT_ODE_BOSH3 4
#define LT_ODE_FEHLBERG2 5
#define LT_ODE_ADAPTIVE_HEUN 6
/* the linear multistep methods of lt_sample_ode_multistep.  That call takes no method code - its weight table is the method; the codes name
 * the methods where another call refuses them (lt_sample_ode_masked and its packed form) */
#define LT_ODE_AB2 32
#define LT_ODE_AB3 33
#define LT_ODE_ABM2 34
#define LT_ODE_ABM3 35
/* lt_op_rk_*: most slopes a chain runs over (dopri5: 7), and the bytes of device workspace a norm needs */
/* lt_forward_cached: the kinds of a single evaluation under step caching */
#define LT_CACHE_PROBE 0
#define LT_CACHE_RUN 1
#define LT_CACHE_REUSE 2
#define LT_RK_MAX_SLOPES 7
#define LT_RK_WS_BYTES 8192
/* lt_sample_sde: method, last step, and the length (floats) of one stage record */
#define LT_SDE_EULER 0
#define LT_SDE_HEUN 1
#define LT_SDE_LAST_NONE 0
#define LT_SDE_LAST_MEAN 1
#define LT_SDE_LAST_TWEEDIE 2
#define LT_SDE_LAST_EULER 3
#define LT_SDE_REC 8
/* lt_op_sde_step: the fused kernels of lt_sample_sde */
#define LT_SDE_OP_EULER 0
#define LT_SDE_OP_HEUN_XHAT 1
#define LT_SDE_OP_HEUN_K1 2
#define LT_SDE_OP_HEUN_OUT 3
#define LT_SDE_OP_LAST_MEAN 4
#define LT_SDE_OP_LAST_TWEEDIE 5
#define LT_SDE_OP_LAST_EULER 6

typedef struct lt_engine lt_engine;

typedef struct lt_config {
    int32_t variant;       /* LT_VARIANT_*                                                        */
    int32_t dim;           /* model width d            (model.py:674)                             */
    int32_t n_layers;      /* L                        (model.py:675)                             */
    int32_t n_heads;       /* H                        (model.py:676)                             */
    int32_t n_kv_heads;    /* GQA kv heads, == n_heads for MHA (model.py:158)                     */
    int32_t ffn_hidden;    /* F, already rounded as in FeedForward.__init__ (model.py:469-473)    */
    int32_t patch_size;    /* 2                                                                   */
    int32_t in_channels;   /* 4                                                                   */
    int32_t out_channels;  /* 8 when learn_sigma (model.py:689)                                   */
    int32_t cap_feat_dim;  /* text feature width (2048 Gemma-2B); 0 for class-conditional         */
    int32_t adaln_dim;     /* min(dim, 1024)           (model.py:563)                             */
    int32_t qk_norm;       /* 1: affine LayerNorm over the full q/k projection (model.py:211-215) */
    int32_t num_classes;   /* class-conditional variants only (label table has num_classes+1 rows)*/
    float   norm_eps;      /* RMSNorm eps, 1e-5        (model.py:680)                             */
    int32_t max_batch;     /* max rows of the (cond+uncond) batch the workspace is sized for      */
    int32_t max_tokens;    /* max latent tokens per sample (N)                                    */
    int32_t max_text;      /* max text tokens per sample (T)                                      */
    int32_t rope_table_len;/* 384 (model.py:734); positions per axis in the 2-D RoPE table        */
    int32_t num_experts;   /* LT_VARIANT_NEXT_MOE*: experts per MoE layer (4 models2.py:696, 8 models.py / models1.py:666); top-2 */
} lt_config;

/* kwargs of NextDiT.forward_with_cfg (model.py:866-877) that are not tensors */
typedef struct lt_step_args {
    float   cfg_scale;         /* model.py:872                                                    */
    float   scale_factor;      /* model.py:873   RoPE extrapolation factor (rope_scaling_factor elsewhere) */
    float   scale_watershed;   /* model.py:874   t < watershed -> linear interp, else NTK          */
    int32_t base_seqlen;       /* model.py:875   0 = None                                          */
    int32_t proportional_attn; /* model.py:876                                                     */
    int32_t latent_h;          /* H of x[B,C,H,W]                                                  */
    int32_t latent_w;          /* W of x[B,C,H,W]                                                  */
    int32_t batch;             /* B (cond+uncond rows), even for forward_with_cfg                  */
    int32_t io_dtype;          /* LT_BF16 or LT_F32: dtype of x and out                            */
    int32_t cfg_channels;      /* 3 = reference quirk (model.py:908); in_channels = standard CFG   */
    float   ntk_factor;        /* ImageNet / Flag-DiT forward_with_cfg(ntk_factor=...) (models.py:946,  */
                               /* lumina_t2i model.py:866-875); there scale_factor = rope_scaling_factor; */
                               /* <= 0 means 1.0.  Ignored by LT_VARIANT_NEXT_T2I.                       */
} lt_step_args;

const char* lt_last_error(void);
/* library / build identification: "lumina_dit gfx950 r5" */
const char* lt_version(void);

/* ---- options ----------------------------------------------------------------------------------
 * The engine picks its kernels by problem shape; a handful of A/B and diagnostic options can override the choice.  They are NOT part
 * of the drop-in surface - an integrator never has to touch them - and are documented, one by one, in include/lumina_dit_debug.h.
 *   lt_set_option          sets the PROCESS DEFAULT of an option: what engines without an override of their own, and the lt_op_*
 *                          operator entry points, use
 *   lt_engine_set_option   overrides an option for ONE engine (every later call on that engine, from any thread; nothing else).
 *                          value LT_OPTION_INHERIT drops the override again.  Thread-safe against calls running on the same engine: every
 *                          engine entry point takes one snapshot of all options when it starts and finishes on that snapshot
 *   lt_engine_get_option   the value in effect for an engine (e == NULL: the process default)
 * Unknown names and out-of-range values are errors (lt_last_error names the range).  There is no other mutable state outside an
 * lt_engine. */
#define LT_OPTION_INHERIT INT32_MIN
int lt_set_option(const char* name, int32_t value);
int lt_engine_set_option(lt_engine* e, const char* name, int32_t value);
int lt_engine_get_option(lt_engine* e, const char* name, int32_t* value);

/* ---- engine lifetime ------------------------------------------------------------------------- */
int  lt_create(const lt_config* cfg, lt_engine** out);
void lt_destroy(lt_engine* e);

/* Upload one checkpoint tensor by its reference state_dict key, e.g.
 * "layers.3.attention.wq.weight".  The engine converts to bf16 and repacks into its own HBM arena
 * (QKV concatenated, w1/w3 interleaved in 32-row groups for the fused SwiGLU epilogue); the source
 * pointer is not retained.  Unknown keys are an error; lt_weights_ready() reports missing keys. */
int lt_set_weight(lt_engine* e, const char* key, const void* src_dev, int32_t dtype,
                  const int64_t* shape, int32_t ndim, void* stream);
int lt_weights_ready(lt_engine* e); /* 0 if every required tensor has been uploaded */

/* Step-invariant text work (model.py:421-422,602,847-850): masked mean pool + cap_embedder, and per
 * layer RMSNorm_y -> wk_y/wv_y -> ky_norm K/V.  cap_feats [B,T,cap_dim], cap_mask int32 [B,T]. */
int lt_prepare_prompt(lt_engine* e, const void* cap_feats_dev, int32_t cap_dtype,
                      const int32_t* cap_mask_dev, int32_t B, int32_t T, void* stream);
/* Compositional (regional) conditioning - lumina_next_compositional_generation/models/model.py:852-890, :422-446: Y captions
 * [Y,T,cap_dim] with masks; captions 0..Y-2 condition regions of the COND row (the latent grid cut into h_split x w_split cells,
 * cell (i,j) -> caption (i+1)(j+1)-1 as in the reference), caption Y-1 conditions the whole UNCOND row; the adaLN conditioning
 * is pooled from the one-row global caption [1,Tg,cap_dim].  Steps that follow run one image (batch 2).  A later
 * lt_prepare_prompt switches back to plain per-row captions.  Needs max_batch >= Y. */
int lt_prepare_prompt_regional(lt_engine* e, const void* cap_feats_dev, int32_t cap_dtype, const int32_t* cap_mask_dev,
                               int32_t Y, int32_t T, const void* global_feats_dev, const int32_t* global_mask_dev,
                               int32_t Tg, int32_t h_split, int32_t w_split, void* stream);
/* class-conditional variants: labels int32 [B] (null class = num_classes) */
int lt_prepare_labels(lt_engine* e, const int32_t* labels_dev, int32_t B, void* stream);

/* NextDiT.forward (model.py:836-864): x [B,C,H,W] -> out [B,C,H,W] (first in_channels kept). */
int lt_forward(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev,
               const lt_step_args* a, void* stream);
/* NextDiT.forward with a LIST of differently sized samples (patchify_and_embed list branch, model.py:789-834; unpatchify
 * :757-768): x_ptrs / out_ptrs are HOST arrays of a->batch device pointers, sample b is [in_channels, H_b, W_b] with
 * (H_b, W_b) = hw_host[2b], hw_host[2b+1] (a->latent_h / latent_w are ignored).  Sequences are padded to the longest one with
 * pad_token; padded keys are masked; each output has its own sample's shape (sigma half dropped).  Text-conditional
 * Next-DiT, plain forward only (the reference's forward_with_cfg takes tensors only). */
int lt_forward_packed(lt_engine* e, const void* const* x_ptrs, const int32_t* hw_host, const float* t_dev,
                      void* const* out_ptrs, const lt_step_args* a, void* stream);
/* Guidance on a LIST of differently sized samples, by composition of two unmodified pieces of the reference: NextDiT.forward on the list
 * [x_0 .. x_{B'-1}, x_0 .. x_{B'-1}] (captions cond_0 .. cond_{B'-1}, uncond_0 .. uncond_{B'-1}; t with 2 B' entries) and the guidance
 * expression of model.py:901-913 per sample (cfg_channels quirk included).  a->batch = 2 B'; hw_host = [a->batch][2] latent sizes with
 * hw[b] == hw[b + B'] (a->latent_h / latent_w are ignored).  x_flat_dev / out_flat_dev: ONE buffer each in a->io_dtype, sample b =
 * [in_channels, H_b, W_b] at element offset sum_{j<b} in_channels H_j W_j; the second half of x is not read (its pixels are the first
 * half's), both halves of out are written.  Padding, key mask, rotary grid width and the proportional-attention length as lt_forward_packed.
 * Evaluations go through the HIP-graph cache; the size list is part of the key.
 * Refused by name, leaving out untouched: a null argument; an odd batch; halves of different sizes; more than 64 samples or more than
 * max_batch; a size that is not a positive multiple of the patch size; a longest sequence above max_tokens or a grid above the RoPE
 * table; any variant other than LT_VARIANT_NEXT_T2I; a regional prompt. */
int lt_forward_cfg_packed(lt_engine* e, const void* x_flat_dev, const int32_t* hw_host, const float* t_dev, void* out_flat_dev,
                          const lt_step_args* a, void* stream);
/* NextDiT.forward_with_cfg (model.py:866-913): duplicates the first half, CFG on cfg_channels. */
int lt_forward_cfg(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev,
                   const lt_step_args* a, void* stream);

/* ode.sample (integrators.py:104-116) with torchdiffeq's fixed-grid euler / midpoint / rk4:
 * tgrid host pointer, n_grid points; z [B,C,H,W]; traj_dev (may be NULL) receives all n_grid
 * states [n_grid,B,C,H,W]; final_dev (may be NULL) receives the last state.  Every model call is
 * forward_with_cfg when use_cfg != 0, else forward.  t_round_to_state_dtype mirrors torchdiffeq's
 * _PerturbFunc cast of t to the state dtype. */
int lt_sample_ode(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev,
                  const float* tgrid_host, int32_t n_grid, int32_t method, int32_t use_cfg,
                  int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);

/* lt_sample_ode on a packed batch: z, each of the n_grid trajectory slots (traj_flat_dev, may be NULL) and the final state (final_flat_dev,
 * may be NULL) are flat buffers in the layout of lt_forward_cfg_packed.  Every model call is the packed forward_with_cfg when use_cfg != 0,
 * else the packed forward (any batch); stage times, stage arithmetic and rounding points are lt_sample_ode's, statement for statement.
 * lt_last_nfe = (n_grid - 1) * stages.  No synchronisation, no host read.  Refused by name with no partial result: what
 * lt_forward_cfg_packed refuses (the odd batch and the unequal halves under use_cfg only), an unknown method, n_grid < 2. */
int lt_sample_ode_packed(lt_engine* e, const void* z_flat_dev, const int32_t* hw_host, void* traj_flat_dev, void* final_flat_dev,
                         const float* tgrid_host, int32_t n_grid, int32_t method, int32_t use_cfg, int32_t t_round_to_state_dtype,
                         const lt_step_args* a, void* stream);

/* Inpainting: lt_sample_ode with a per-element blend after every full step.  mask_dev (1 = generate, 0 = keep), x1_dev (the
 * source latent) and noise_dev (the noise the trajectory started from) have the layout and dtype of the state.  After the step that ends at
 * grid point i + 1 (the last one included) the state becomes, every tensor op rounding to the state dtype R(),
 *     R(R(step mask) + R(R(R(noise (1 - t)) + R(x1 t)) R(1 - mask))),   t = tgrid[i + 1] and 1 - t (formed in double) multiplying in fp32,
 * in the kernel of the step's closing combine: no launch is added.  Stage-internal states (the midpoint half step, rk4 stages 2-4) are not
 * blended and z is taken as it is.  Stage times, dt, trajectory slots and lt_last_nfe are lt_sample_ode's.  The mask's values are not read
 * by the host: outside [0, 1] the blend extrapolates.  mask = 1 everywhere gives lt_sample_ode's states (up to the sign of a zero), mask = 0
 * everywhere the known path noise (1 - t) + x1 t, x1 at t = 1.  Every model variant.  No synchronisation, no host read.  Refused by name
 * with nothing written: what lt_sample_ode refuses; a null mask, source or noise. */
int lt_sample_ode_masked(lt_engine* e, const void* z_dev, const void* mask_dev, const void* x1_dev, const void* noise_dev, void* traj_dev,
                         void* final_dev, const float* tgrid_host, int32_t n_grid, int32_t method, int32_t use_cfg,
                         int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);
/* lt_sample_ode_masked on a packed batch: mask, source and noise are flat buffers of the layout of lt_forward_cfg_packed, like the state.
 * Refused by name with nothing written: what lt_sample_ode_packed refuses; a null mask, source or noise. */
int lt_sample_ode_masked_packed(lt_engine* e, const void* z_flat_dev, const int32_t* hw_host, const void* mask_flat_dev, const void* x1_flat_dev,
                                const void* noise_flat_dev, void* traj_flat_dev, void* final_flat_dev, const float* tgrid_host, int32_t n_grid,
                                int32_t method, int32_t use_cfg, int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);

/* ---- multi-view (visual-anagram) sampling: visual_anagrams/generate.py:389-414, Phase Init ------------------------------------------
 * ONE latent; per time interval every view v sees view_v(latent) with its own prompt, takes one ODE step of forward_with_cfg, and the mean
 * over the views of inverse_view_v(-increment) is subtracted from the latent.  A view is data: view_v(x)[c, i] = vsign[v][c] * x[c, perm[v][i]],
 * inverse_view_v(n)[c, i] = isign[v][c] * n[c, iperm[v][i]] over the H*W pixels of a channel.
 * lt_set_views: perm_dev int32 [V][latent_h * latent_w] (device), vsign_host / isign_host float [V][in_channels] of +-1 (host).  The tables
 * are copied into engine-owned memory, iperm is built on the device and the call SYNCHRONISES the stream to report a table that is not a
 * bijection.  Refused: V < 1, 2 V > max_batch, a latent that is not a multiple of the patch size or exceeds max_tokens, any variant other
 * than LT_VARIANT_NEXT_T2I.  V = 0 (perm_dev NULL) drops the tables.
 * lt_sample_views: z [1, C, H, W]; traj_dev (may be NULL) receives the n_grid latents [n_grid, C, H, W], final_dev (may be NULL) the last.
 * The prompt was prepared with lt_prepare_prompt at B = 2 V: rows 0..V-1 the view prompts, rows V..2V-1 the negative prompt; a->batch = 2 V
 * and a->latent_h / latent_w equal the tables'.  method LT_ODE_MIDPOINT (the reference's midpoint_solver, generate.py:212-219) or LT_ODE_EULER
 * (one stage: the increment is f(t0) dt); LT_ODE_RK4 is refused.  Every stage is ONE forward_with_cfg of 2 V rows (lt_last_nfe: 2 per
 * interval for midpoint).  dt and dt / 2 multiply in fp32 (Python floats in the reference), t is fp32.  No synchronisation, no host read. */
int lt_set_views(lt_engine* e, const int32_t* perm_dev, const float* vsign_host, const float* isign_host, int32_t V, int32_t latent_h,
                 int32_t latent_w, void* stream);
int lt_sample_views(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                    int32_t method, const lt_step_args* a, void* stream);

/* ---- tiled (MultiDiffusion, Bar-Tal et al. 2023) sampling: one canvas latent, the model on overlapping windows of it --------------------------
 * ONE canvas latent [1, C, Hc, Wc] is kept.  Every evaluation crops n windows of one size h x w out of it, evaluates them as ONE
 * forward_with_cfg of 2 n rows at the window size (rows 0 .. n-1 the crops with the window prompts, rows n .. 2n-1 the negative prompts), and
 * fuses the n predictions into the canvas velocity: per pixel, the sum over the windows that hold it of weight * prediction, divided by the
 * sum of those weights.  lumina-t2x_amd/transport/tiled.py is the definition (the reference has no such sampler): fuse states the arithmetic -
 * every product and sum one fp32 operation in window order, one division, one rounding to the state dtype - and the calls equal it bit for bit.
 * Nothing in the calls is family-specific: every variant is served, with labels prepared by lt_prepare_labels in the same row layout.
 * lt_set_windows: offsets_host int32 [n][2] = (top, left) of each window in latent pixels (HOST), weight_dev float [win_h * win_w] (DEVICE) or
 * NULL for all ones.  The table goes into engine-owned memory (allocated by the first call: the weights, the per-pixel weight sums and the
 * window rows going into and coming out of the model), the sums are formed on the device and the call SYNCHRONISES the stream once, to refuse
 * a canvas with a pixel that lies under no window or under weights whose sum is not finite and above 0.  n = 0 drops the table.  Refused by
 * name, with the table in force left as it was: a null engine or offset table; n < 0, n > 64 or 2 n > max_batch; sizes or offsets that are
 * not multiples of the patch size; a window larger than, or outside, the canvas; a window of more than max_tokens tokens or with a grid above
 * the RoPE table; a canvas with more pixels than its n windows; a stream under capture.
 * The canvas always fits the engine's state buffers: a covered canvas has at most n * h * w pixels, n <= max_batch / 2 and h * w pixels are
 * at most max_tokens tokens, and the state buffers hold max_batch samples of max_tokens tokens.
 * lt_forward_tiled: one canvas evaluation.  y_dev / v_dev [1, C, Hc, Wc] in a->io_dtype, t_dev float [2 n]; a->latent_h / latent_w are the
 * WINDOW's, a->batch = 2 n.  Three steps: the gather, forward_with_cfg of the 2 n rows through the evaluation's own graph cache (no new graph
 * key: it IS an lt_forward_cfg of that shape), the fusion.
 * lt_sample_ode_tiled: lt_sample_ode(use_cfg = 1) with the canvas as the state and lt_forward_tiled's three steps as every stage's velocity:
 * stage times, dt handling and every stage / closing combine are lt_sample_ode's.  z [1, C, Hc, Wc]; traj_dev (may be NULL) receives the n_grid
 * canvases, final_dev (may be NULL) the last.  lt_last_nfe = (n_grid - 1) * stages, lt_last_eval_rows = 2 n times that.  No synchronisation,
 * no host read.
 * Both refuse by name, before anything is launched: no window table; a->batch other than 2 n or a latent other than the table's window; a
 * regional prompt; a layer-skip or perturb set; a conditioning prepared for another batch; lt_sample_ode_tiled also a stream under capture, a
 * grid of fewer than 2 points and an unknown method. */
int lt_set_windows(lt_engine* e, const int32_t* offsets_host, int32_t n, int32_t win_h, int32_t win_w, int32_t canvas_h, int32_t canvas_w,
                   const float* weight_dev, void* stream);
int lt_forward_tiled(lt_engine* e, const void* y_dev, const float* t_dev, void* v_dev, const lt_step_args* a, void* stream);
int lt_sample_ode_tiled(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid, int32_t method,
                        int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);

/* ---- composed guidance (Composable Diffusion, Liu et al. 2022): K weighted prompts and one base prompt per image in one call ----------------
 *     g = u + sum_{k = 1 .. K} w_k (c_k - u)            a negative w_k is a negation ("A but NOT C"), K = 1 is classifier-free guidance
 * The state has B' rows.  Every evaluation replicates them K + 1 times and runs ONE plain forward (use_cfg = 0) of a->batch = (K + 1) B' rows
 * through the evaluation's own graph cache - no new graph key, no new evaluation kind: it IS an lt_forward of that shape.  Row layout of the
 * conditioning (lt_prepare_prompt / lt_prepare_labels at (K + 1) B' rows, every variant) and of the model's output: rows k B' + b belong to
 * prompt k of image b (k = 0 .. K-1), rows K B' + b to the base (negative / empty) prompt.  lumina-t2x_amd/transport/guidance.py is the
 * definition (the reference has no such sampler) and the calls equal it bit for bit: guided_compose on channels < a->cfg_channels, with R =
 * round to bf16 (the model's output dtype, whatever a->io_dtype) and every difference, product and sum one fp32 operation,
 *     acc = R(w_1 R(c_1 - u));   acc = R(acc + R(w_k R(c_k - u)))  for k = 2 .. K in this order;   g = R(u + acc)
 * which at K = 1 is lt_forward_cfg's chain word for word; channels >= a->cfg_channels are prompt 1's row, copied (the first half of
 * lt_forward_cfg's output under the reference's cfg_channels = 3 quirk).  The K weights are read on the HOST during the call and travel as a
 * kernel argument: no graph is re-recorded when they change.  A prompt of weight 0 is still evaluated (leaving its rows out would change the
 * row count, and with it the graph key).
 * lt_forward_compose: one evaluation.  x_dev / out_dev [B', C, H, W] in a->io_dtype, t_dev float [(K + 1) B'], w_host float [K].
 * lt_sample_ode_compose: lt_sample_ode(use_cfg = 0) on the B' rows with the three steps above as every stage's velocity: stage times, dt
 * handling, t_round and every stage / closing combine are lt_sample_ode's.  w_host float [(n_grid - 1) * stages][K]: stage s of interval i
 * uses row i * stages + s (transport/guidance.py compose_table).  traj_dev (may be NULL) receives the n_grid states [B', C, H, W], final_dev
 * (may be NULL) the last.  lt_last_nfe = (n_grid - 1) * stages, lt_last_eval_rows = (K + 1) B' times that.  No synchronisation, no host read.
 * The replicated rows and the model's outputs live in the engine-owned window-row buffers of the tiled calls (max_batch samples wide),
 * allocated by the first call that needs them (that call is refused on a stream under capture).
 * Both refuse by name, before anything is launched and with the outputs untouched: a null argument; K < 1 or K > LT_COMPOSE_MAX; a->batch not a
 * positive multiple of K + 1, or above max_batch; a weight that is not finite; a->cfg_channels outside 1 .. in_channels; what lt_forward
 * refuses of the shape; a regional prompt; a layer-skip or perturb set; a conditioning prepared for another batch; lt_sample_ode_compose also
 * a stream under capture, a grid of fewer than 2 points and an unknown method. */
#define LT_COMPOSE_MAX 7
int lt_forward_compose(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const float* w_host, int32_t K, const lt_step_args* a,
                       void* stream);
int lt_sample_ode_compose(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid, int32_t method,
                          const float* w_host, int32_t K, int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);

/* ---- multi-view sampling, Phase Upscale: visual_anagrams/generate.py:465-494 with midpoint_solver_extra (:222-262) -------------------------
 * lt_set_softmax_rule: the model of that phase is visual_anagrams/models/nextdit.py, which differs from LT_VARIANT_NEXT_T2I's model in ONE
 * scalar: under proportional_attn its self-attention softmax scale is log(N, base_seqlen) / sqrt(head_dim) (LT_SOFTMAX_ANAGRAM) where the T2I
 * model has sqrt(log(N, base_seqlen) / head_dim) (LT_SOFTMAX_T2I, the default); computed in double, cast once.  Without proportional_attn both
 * are sqrt(1 / head_dim).  The rule is engine state: it holds for every later evaluation on this engine until it is set again, and is part of
 * the HIP-graph key.  The fork's RoPE ("ntk_v1", nextdit.py:1014-1018: theta * scale_factor at every timestep) is the NTK branch of the T2I
 * table: pass scale_watershed = 0 in lt_step_args.  The fork walks the queries in int(N / base_seqlen + 0.99) chunks of base_seqlen rows, each
 * against all keys: the same result row by row, except where the chunks end before the rows do - under LT_SOFTMAX_ANAGRAM with
 * proportional_attn a shape with int(N / base_seqlen + 0.99) * base_seqlen < N is refused by name.  Refused too: any variant other than
 * LT_VARIANT_NEXT_T2I, an unknown rule.
 * lt_sample_views_guided: z, guidance, noise [1, C, H, W] in a->io_dtype (noise_dev may alias z_dev; none is written).  Prompt layout and view
 * tables as for lt_sample_views (lt_prepare_prompt at B = 2 V, lt_set_views).  Per interval [t0, t1], with dt = t1 - t0, half_dt = dt / 2 and
 * R = round to the state dtype, p = perm[v][i]:
 *   stage at t0:            s = y
 *   stage at t0 + half_dt:  s[c,p] = R(y[c,p] + isign[v][c] * R(f0[v][c,i] * half_dt))            f0: the first stage's output, per view
 *   model input of view v:  vsign[v][c] * R(R(k1c * s[c,p]) + R(kc * R(R(ft * guidance[c,p]) + R(f1t * noise[c,p]))))
 *   closing update:         y' = R(y - R((sum_v inverse_view_v(-R(f1_v * dt))) / V))               as lt_sample_views
 * Every stage is ONE forward_with_cfg of 2 V rows; lt_last_nfe = 2 per interval.  Stage times are the fp32 of the doubles t0 and t0 + half_dt.
 * coef_host float [(n_grid - 1)][2 stages][4] = { ft, f1t, kc, k1c } at the stage's time t: ft = fp32(t), f1t = fp32(1 - t) (the reference
 * multiplies by Python floats), kc = c, k1c = 1 - c with c = 0.5 (1 + cos(pi t)) evaluated in fp32 as the reference does.  Whether c and 1 - c
 * are rounded to the state dtype before the multiply is the caller's choice (PyTorch's CPU kernels do round such a 0-dim tensor operand,
 * its GPU kernels are expected to keep it in fp32; transport.integrators.views_guided_table offers both).  Midpoint is the only stepping rule
 * the reference has for this phase.  No synchronisation, no host read.  Refused by name, with no partial result, in this order: null
 * arguments; a variant other than LT_VARIANT_NEXT_T2I; n_grid < 2; no view tables; a->batch != 2 V; a latent that differs from the tables';
 * a batch or token count over the engine's limits; a coefficient that is not finite; (with LT_SOFTMAX_ANAGRAM) a shape the chunks do not cover. */
int lt_set_softmax_rule(lt_engine* e, int32_t rule);
int lt_sample_views_guided(lt_engine* e, const void* z_dev, const void* guidance_dev, const void* noise_dev, void* traj_dev, void* final_dev,
                           const float* tgrid_host, const float* coef_host, int32_t n_grid, const lt_step_args* a, void* stream);

/* ---- SDE sampling: sde.sample + the last step of Sampler.sample_sde (integrators.py:5-76, transport.py:285-344), velocity prediction ---------
 * The whole trajectory in one call, ONE model evaluation per stage: the reference's sde_drift = drift + D * score evaluates the model twice
 * on the same (x, t) (transport.py:172-173); the engine is deterministic, so the fused step kernels read the one output twice.
 * z [B,C,H,W] in the state dtype (a->io_dtype).  noise_dev [n_steps - 1, B,C,H,W], state dtype: the caller's draws, step by step (the engine
 * owns no RNG).  traj_dev (may be NULL) receives the n_steps - 1 loop states [n_steps - 1, B,C,H,W] (state 0 is the state AFTER the first
 * step, as in the reference).  final_dev receives the last-step state: fp32 [B,C,H,W] for LT_SDE_LAST_MEAN / _TWEEDIE whatever the state dtype
 * (the reference's last step runs at an fp32 time vector and type promotion makes the result fp32), the state dtype for LT_SDE_LAST_EULER;
 * with LT_SDE_LAST_NONE no last step runs and final_dev (may be NULL) receives a copy of the last loop state.
 * steps_host: (n_steps - 1) * stages records of LT_SDE_REC floats, stages = 1 (LT_SDE_EULER) or 2 (LT_SDE_HEUN: the stage at t, then the stage
 * at t + dt).  Record: { t, r, var, D, q, dt, sqrt_dt, hdt } - t the stage time handed to the model; r = alpha / alpha', var = sigma^2 - r sigma'
 * sigma and D the diffusion coefficient at t, q = sqrt(2 D): the VALUES of the [B,1,1,1] state-dtype tensors the path plan produces (same
 * contract as tgrid_host: already rounded); dt, sqrt_dt, hdt = 0.5 dt are fp32 and multiply in fp32.  A Heun step reads q, dt, sqrt_dt from
 * its first record and hdt from its second.  last_coef_host (LT_SDE_LAST_NONE: may be NULL): one record { t, r, var, D, h, a, c, 0 } at the
 * last time, all fp32 - h the last step size, a = alpha rounded to the state dtype and c = sigma^2 / alpha (Tweedie only).
 * Rounding points: csrc/sde.hip.  lt_last_nfe = (n_steps - 1) * stages + (last_step != LT_SDE_LAST_NONE).
 * Refused by name: unknown method / last_step, n_steps < 2, a var that is not finite and positive.  Score / noise prediction is not served
 * here (the Python sampler keeps its host loop for them).  Like lt_sample_ode: no synchronisation, no host read, the caller's stream. */
int lt_sample_sde(lt_engine* e, const void* z_dev, const void* noise_dev, void* traj_dev, void* final_dev, const float* steps_host,
                  int32_t n_steps, int32_t method, int32_t last_step, const float* last_coef_host, int32_t use_cfg, const lt_step_args* a,
                  void* stream);

/* ---- adaptive ODE sampling: ode.sample with torchdiffeq's dopri5 / bosh3 / fehlberg2 / adaptive_heun (transport/integrators.py: adaptive_odeint) ----
 * The whole trajectory in one call: stage arithmetic, error estimate, tolerance, norm, dense output and interpolation are fused kernels
 * (csrc/ode_adaptive.hip, rounding points there), the step-size controller runs on the host in C++.  z [B,C,H,W] in the state dtype
 * (a->io_dtype); traj_dev receives the n_grid states [n_grid,B,C,H,W], row 0 = z; tgrid_host: the fp32 grid, strictly increasing, at least 2
 * points.  Steps are the controller's own and may overshoot a grid point: the state there is the quartic dense output of the accepted step
 * that contains it.  Every model call is forward_with_cfg when use_cfg != 0, else forward; t_round_to_state_dtype as in lt_sample_ode.
 * Controller: what the host loop holds in 0-dim fp32 tensors is fp32 here (tcur + dt, tcur + fp32(alpha) dt, dt fp32(factor), the
 * interpolation argument (next_t - tprev) / (tcur - tprev)); what it computes in Python floats is double (factor = min(10, max(0.9 /
 * ratio^(1 / order), 0.2 or 1)), ratio == 0 -> factor 10).  The error ratio is the fp32 rounding of a float64 tree sum (the host loop reduces
 * in fp32), so dt may differ from the host loop's by fp32 ulps.
 * first_step > 0 is the first dt as given (ONE evaluation in front of the first step); first_step == 0 selects it by torchdiffeq's heuristic
 * (two evaluations, three norms); its (0.01 / max(d1, d2))^(1 / order) is computed in double and rounded to fp32, which may differ by an fp32
 * ulp from torch's device pow.  lt_last_nfe = (1 or 2) + stages * attempted steps.
 * stats (may be NULL): evaluation and step counts, the first dt used, and - when dt_host is set - the dt of every attempted step, at most
 * dt_cap of them (dt_count is the number of attempts, whatever dt_cap).
 * Refused by name, with no partial result: an unknown method; rtol or atol <= 0 or not finite; first_step < 0 or not finite; max_steps < 1;
 * n_grid < 2 or a grid that is not strictly increasing; "step size underflow" (tcur + dt == tcur, torchdiffeq's own assertion); more than
 * max_steps attempted steps inside one grid interval ("max_steps"); an error ratio that is not finite.
 * UNLIKE lt_sample_ode this call SYNCHRONISES the stream once per attempted step (and up to three times for the initial step): the host
 * reads the 4-byte error ratio, which adaptive stepping cannot avoid. */
typedef struct lt_ode_adaptive_stats {
    int64_t nfe;
    int32_t accepted, rejected;
    float   first_step;  /* the first dt: the given one, or the heuristic's */
    int32_t dt_cap;      /* in: floats dt_host has room for                */
    int32_t dt_count;    /* out: attempted steps                            */
    float*  dt_host;     /* in: may be NULL                                 */
} lt_ode_adaptive_stats;
int lt_sample_ode_adaptive(lt_engine* e, const void* z_dev, void* traj_dev, const float* tgrid_host, int32_t n_grid, int32_t method, float rtol,
                           float atol, float first_step, int32_t max_steps, int32_t use_cfg, int32_t t_round_to_state_dtype,
                           const lt_step_args* a, void* stream, lt_ode_adaptive_stats* stats);

/* Guidance schedules: lt_sample_ode with guidance whose scale changes from stage to stage.  cfg_host holds (n_grid - 1) *
 * stages fp32 scales (stages = 1 euler, 2 midpoint, 4 rk4): stage k of interval i uses w = cfg_host[i * stages + k].  The state has a->batch =
 * 2 B' rows (cond rows, then uncond rows); the prompt / the labels were prepared for all 2 B' rows, once.
 *   w != 1:  the stage's slope is forward_with_cfg at scale w - lt_forward_cfg's arithmetic, the scale read from device memory;
 *   w == 1 exactly:  the slope is the plain forward o of the B' cond rows on the cond half of the conditioning - bit for bit lt_forward at
 *            batch B' after a preparation of those rows alone - written to both halves of the slope (cat([o, o])): B' rows are evaluated, not
 *            2 B'.  (Under cfg_channels < in_channels the channels past cfg_channels of the second half then hold the cond rows' output where
 *            forward_with_cfg at scale 1 would hold the uncond rows'; the first half is the sample.)
 * Stage times, dt, rounding points, trajectory slots and lt_last_nfe = (n_grid - 1) * stages are lt_sample_ode's; lt_last_eval_rows =
 * 2 B' G + B' C for G guided and C conditional-only stages.  a->cfg_scale is ignored.  The scales are committed with the stage times and
 * every evaluation finds its own in a fixed device word, so a trajectory uses at most two HIP-graph keys (the 2 B'-row guided evaluation,
 * the B'-row conditional one) whatever the table holds.  Where the two sizes fall on different sides of the pair-layout threshold every
 * change between them converts all GEMM weights (lt_engine_get_option "layout_flips" counts the conversions of the last call).
 * No synchronisation, no host read.  Every variant lt_sample_ode serves with guidance.  Packed batches, inpainting masks and views are not
 * served by this call.  Refused by name with nothing written: a null argument; an unknown method; n_grid < 2; what lt_sample_ode refuses of
 * the shape; an odd batch; a scale that is not finite; a regional prompt (lt_prepare_prompt_regional); a conditioning prepared for another
 * batch. */
int lt_sample_ode_cfg_schedule(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                               int32_t method, const float* cfg_host, int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);

/* Rescaled and norm-limited guidance: lt_sample_ode_cfg_schedule / lt_forward_cfg whose guided output is multiplied, per
 * sample, by one factor f.  With c and u the cond and uncond rows' outputs on the first cfg_channels channels, g = u + w (c - u) with the
 * bf16 rounding points of lt_forward_cfg, and the sums over one sample's n = cfg_channels H W elements taken in float64:
 *   vc = sum c^2 / n - (sum c / n)^2, vg likewise;  ratio = sqrt(vc / vg) if vg > 0 and vc >= 0, else 1
 *   fr = rescale ratio + (1 - rescale)                                   ("guidance rescale": the std of g pulled towards that of c)
 *   fl = min(1, norm_limit sqrt(sum c^2) / (fr sqrt(sum g^2))) if norm_limit < inf and fr sqrt(sum g^2) > 0, else 1     (the norm of g at
 *        most norm_limit times that of c)
 *   f = fp32(fr fl), everything before it float64 without contraction; the guided channels become bf16(g f), one fp32 multiply.
 * The channels at or past cfg_channels pass through row by row, as in lt_forward_cfg.  rescale in [0, 1]; norm_limit > 0, +inf = off; at
 * (0, +inf) f is 1 and the results are lt_sample_ode_cfg_schedule's / lt_forward_cfg's bit for bit (through other kernels: callers that
 * want the rule off call those).
 * lt_sample_ode_cfg_rule: lt_sample_ode_cfg_schedule's arguments and behaviour plus the rule on every stage whose scale is not 1.  A stage
 * at scale 1 exactly is that call's conditional-only stage, WITHOUT the rule (with norm_limit < 1 the rule would have scaled it).  The two
 * parameters are committed with the scale table and read from device memory: a trajectory uses at most two HIP-graph keys (the guided
 * evaluation with the rule, the conditional one) whatever the table, rescale and norm_limit hold.  No synchronisation, no host read.
 * lt_forward_cfg_rule: ONE evaluation, always guided, at a->cfg_scale (any finite value, 1 included).  Both calls are refused on a stream
 * under capture (the trajectory for the reason lt_sample_ode is; the single evaluation because no test records it yet).
 * Not served: packed batches, regional prompts, views.  Refused by name with nothing written: what lt_sample_ode_cfg_schedule refuses (for
 * lt_forward_cfg_rule: a null argument, the shape, an odd batch, a scale that is not finite, a regional prompt, a conditioning prepared for
 * another batch); rescale outside [0, 1] or not finite; norm_limit not above 0, or NaN. */
int lt_sample_ode_cfg_rule(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                           int32_t method, const float* cfg_host, float rescale, float norm_limit, int32_t t_round_to_state_dtype,
                           const lt_step_args* a, void* stream);
int lt_forward_cfg_rule(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, float rescale, float norm_limit, const lt_step_args* a,
                        void* stream);

/* Projected guidance (transport/guidance.py: guided_project / sample_cfg_project are the definition, held bit for bit): two
 * published forms of the guided output that need inner products between the cond rows' output c and the uncond rows' output u, on the first
 * cfg_channels channels.  Sums run over one sample's n = cfg_channels H W elements in float64; the coefficients are float64 scalar arithmetic
 * without contraction, each rounded once to fp32; every elementwise operation is one fp32 operation that rounds on its own.
 *   form LT_PROJECT_APG (Sadat et al. 2024), parameters eta (finite), momentum beta (|beta| < 1), norm_threshold r (> 0, +inf = off):
 *     d = bf16(c - u);  m = d + beta m_prev  (fp32, kept in an engine buffer [B', cfg_channels, H, W] from one guided evaluation to the next)
 *     tn = min(1, r / sqrt(sum m^2)) if r < inf and sum m^2 > 0, else 1;   p = tn sum m c / sum c^2 if sum c^2 > 0, else 0
 *     a = fp32((w - 1) tn);  b = fp32((w - 1)(eta - 1) p);  g = bf16(c + (a m + b c))
 *     i.e. c + (w - 1)(orthogonal part + eta parallel part) of the clipped m, the projection taken on the model's velocity output.
 *     At eta = 1, beta = 0, r = +inf this is c + (w - 1)(c - u): plain guidance in ANOTHER rounding chain, not lt_forward_cfg's words.
 *   form LT_PROJECT_ZERO_STAR (Fan et al. 2025): s = fp32(sum c u / sum u^2) if sum u^2 > 0, else 1;  g = bf16(s u + w (c - s u));
 *     zero_init K >= 0: the first K grid intervals take zero velocity - their trajectory slots receive the state unchanged, NO evaluation is
 *     launched for them, lt_last_nfe / lt_last_eval_rows do not count them, their table entries are not read.  K >= n_grid - 1 is refused.
 * g goes to both halves; the channels at or past cfg_channels pass through row by row, as in lt_forward_cfg.
 * lt_sample_ode_cfg_project: lt_sample_ode_cfg_schedule's arguments and behaviour with the form on every stage whose scale is not 1; a stage
 * at scale 1 exactly is that call's conditional-only stage and neither reads nor writes the momentum.  The momentum is zeroed once, in stream
 * order, in front of the first evaluation of EVERY call; the guided evaluations advance it in evaluation order (the stages of midpoint / rk4
 * count).  The parameters are committed with the scale table and read from device memory: a trajectory uses at most two HIP-graph keys (the
 * projected evaluation of its form, the conditional one) whatever the table and the parameters hold.  The parameters of the form not chosen
 * are ignored (zero_init belongs to Zero*, and must be 0 under APG).  No synchronisation, no host read.
 * lt_forward_cfg_project: ONE evaluation, always guided, at a->cfg_scale.  keep_momentum 0: the momentum is zeroed first; 1: it continues
 * from the one the last projected APG evaluation left - refused by name when none is stored for this shape (none yet, another shape, or
 * lt_prepare_prompt* / lt_prepare_labels was called since).  Under Zero* keep_momentum must be 0.
 * Both calls are refused on a stream under capture.  Not served: packed batches, regional prompts, views, the rescale / norm-limit rule,
 * reuse, skip-layer and perturbed-attention guidance, step caching, masks, the multistep and adaptive solvers (each of those is another entry
 * point; none takes a form).  Refused by name with nothing written: what lt_sample_ode_cfg_schedule refuses; a form other than 1 / 2; eta not
 * finite; |momentum| >= 1 or NaN; norm_threshold not above 0, or NaN; zero_init < 0, or >= n_grid - 1, or non-zero under APG. */
#define LT_PROJECT_APG 1
#define LT_PROJECT_ZERO_STAR 2
int lt_sample_ode_cfg_project(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                              int32_t method, const float* cfg_host, int32_t form, float eta, float momentum, float norm_threshold,
                              int32_t zero_init, int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);
int lt_forward_cfg_project(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, int32_t form, float eta, float momentum,
                           float norm_threshold, int32_t keep_momentum, const lt_step_args* a, void* stream);

/* Linear multistep sampling (transport/multistep.py states the loop in torch ops and the engine is held to it bit for bit):
 * Adams-Bashforth predictors of 2 or 3 slopes (ab2, ab3) and the same with an Adams-Moulton corrector that costs no evaluation (abm2, abm3).
 * Exactly N = n_grid - 1 model evaluations, one per interval, none at the last grid point (lt_last_nfe).  With f_i = model(p_i, t_i):
 *   p_0 = y_0 = z
 *   y_i     = y_{i-1} + sum_j a_{i,j} f_{i-j}      where row i of the table has a corrector weight that is not 0, else y_i = p_i (any row,
 *                                                   not only row 0: a table may switch the corrector off for single intervals)
 *   p_{i+1} = y_i     + sum_j b_{i,j} f_{i-j}
 * and the result is p_N.  traj_dev (may be null) receives n_grid states: z, then y_i for 0 < i < N, then p_N; final_dev (may be null) p_N.
 * coef_host: N rows of 8 floats, a_{i,0..3} then b_{i,0..3}, j = 0 the newest slope; a sum runs over the entries of its half row up to the
 * last one that is not 0, and a row may name at most min(i + 1, 4) slopes.  The engine computes no weight: the caller fills the table, with q
 * the slopes kept (2 or 3) and L_j the Lagrange basis polynomials on the nodes named,
 *   b_{i,j} = integral over [t_i, t_{i+1}] of L_j(t) dt,  nodes t_i, t_{i-1}, .., t_{i-m+1},  m  = min(q, i + 1)      (step 0 is Euler)
 *   a_{i,j} = integral over [t_{i-1}, t_i] of L_j(t) dt,  nodes t_i, t_{i-1}, .., t_{i-m'},   m' = min(q, i), i >= 1  (i = 1: trapezoid rule)
 * in float64, rounded once to fp32.  corrector: 1 the a halves are used, 0 they are ignored (plain Adams-Bashforth).
 * Rounding, R = round to the state dtype (identity at fp32): acc = R(c_0 k_0); acc = R(acc + R(c_j k_j)); out = R(y + acc), no contraction;
 * the stage time of evaluation i is tgrid[i], rounded to the state dtype under t_round_to_state_dtype as in lt_sample_ode.
 * Guidance: use_cfg 0 the plain forward; 1 lt_forward_cfg at a->cfg_scale (cfg_host null) or at cfg_host[i] for evaluation i, N values, a
 * scale of 1 exactly being the conditional-only evaluation of lt_sample_ode_cfg_schedule; rescale / norm_limit other than (0, +inf) put the
 * rule of lt_sample_ode_cfg_rule on the guided evaluations (a null cfg_host then stands for a->cfg_scale at every evaluation).
 * lt_sample_ode_multistep_packed: the same loop on the flat state of a packed batch (lt_sample_ode_packed's layout), without a table or rule.
 * Refused by name with nothing written: a null argument; a stream under capture; n_grid < 2; a weight that is not finite or a row that names
 * more slopes than exist; corrector not 0 or 1; a guidance table or a rule with use_cfg = 0; what lt_sample_ode refuses of the shape; and
 * with a table or a rule what lt_sample_ode_cfg_rule refuses.  Inpainting with a multistep method is refused (lt_sample_ode_masked given
 * LT_ODE_AB2 .. LT_ODE_ABM3): the blend makes the state discontinuous, so the history's slopes no longer belong to it. */
int lt_sample_ode_multistep(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                            const float* coef_host, int32_t corrector, const float* cfg_host, float rescale, float norm_limit, int32_t use_cfg,
                            int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);
int lt_sample_ode_multistep_packed(lt_engine* e, const void* z_flat_dev, const int32_t* hw_host, void* traj_flat_dev, void* final_flat_dev,
                                   const float* tgrid_host, int32_t n_grid, const float* coef_host, int32_t corrector, int32_t use_cfg,
                                   int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);

/* Guidance reuse (transport/guidance.py: sample_cfg_reuse is the definition): a guided trajectory that takes the difference
 * d = cond - uncond on some evaluations (refresh) and reuses it on the others, which then evaluate the B' cond rows alone.  Per evaluation
 * the caller gives the scale w (cfg_host, as in lt_sample_ode_cfg_schedule) and a flag (reuse_host, int32, 0 / 1).  ch = min(cfg_channels,
 * in_channels), R = rounding to bf16, no contraction:
 *   w == 1 exactly (either flag): the conditional-only stage of lt_sample_ode_cfg_schedule, bit for bit; d is neither read nor written.
 *   w != 1, flag 0 (refresh): all 2 B' rows are evaluated; with c, u the bf16 final rows of a sample and its uncond partner d = R(c - u) and
 *            the output on the channels < ch is R(u + R(w d)) - lt_forward_cfg at scale w word for word, both halves, all channels - and d
 *            is stored in an engine-owned bf16 buffer [B', ch, H, W].
 *   w != 1, flag 1 (reuse): the B' cond rows are evaluated as the conditional-only stage evaluates them; with c' their bf16 output the
 *            channels < ch become R(R(c' - d) + R(w d)), w multiplying in fp32, the channels >= ch are the cond rows'; the result is written
 *            to rows b and b + B'.  d is not modified.
 * lt_sample_ode_cfg_reuse: lt_sample_ode_cfg_schedule's arguments, behaviour and refusals plus the flag table, one int32 per stage.  Stage
 * times, dt, rounding points and trajectory slots are lt_sample_ode's; lt_last_nfe = (n_grid - 1) * stages; lt_last_eval_rows = 2 B' G +
 * B' (R + C) for G refresh, R reuse and C conditional-only stages.  A trajectory replays at most three HIP-graph keys (refresh, reuse,
 * conditional-only) whatever the tables hold.  The buffer (max_batch / 2 * in_channels * max_tokens * patch^2 bf16) is allocated by the first
 * call that needs it, before anything is launched.
 * lt_sample_ode_multistep_cfg_reuse: lt_sample_ode_multistep with a table and without a rule, plus one flag per evaluation.
 * lt_forward_cfg_reuse: ONE evaluation at a->cfg_scale.  mode 0 is lt_forward_cfg and stores d (also at scale 1: a single call always guides);
 * mode 1 evaluates the cond rows and reuses d.  x has 2 B' rows in both modes, both halves of out are written.  The engine remembers the
 * stored d's signature (B', H, W, ch); every lt_prepare_prompt* / lt_prepare_labels call forgets it.  mode 1 without a stored d of this
 * signature is refused by name.
 * Not served: packed batches, regional prompts, views, inpainting, the rescale / norm-limit rule.  No synchronisation, no host read.
 * Refused by name with nothing written: everything lt_sample_ode_cfg_schedule refuses; a null reuse_host; a flag other than 0 / 1; a reuse
 * flag at a scale other than 1 with no refresh stage before it in the same call; a stream under capture; a mode other than 0 / 1. */
int lt_sample_ode_cfg_reuse(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                            int32_t method, const float* cfg_host, const int32_t* reuse_host, int32_t t_round_to_state_dtype,
                            const lt_step_args* a, void* stream);
int lt_sample_ode_multistep_cfg_reuse(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid,
                                      const float* coef_host, int32_t corrector, const float* cfg_host, const int32_t* reuse_host,
                                      int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);
int lt_forward_cfg_reuse(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, int32_t mode, const lt_step_args* a, void* stream);

/* ---- prompt-driven image editing: FlowEdit's inversion-free rule (Kulikov et al., 2024) as one call ---------------------------
 * transport/edit.py: sample_flowedit is the definition; the reference has no such sampler.  Lumina's path x_t = t x1 + (1 - t) x0, noise at
 * t = 0, the grid ascends.  The state is B' edits; a->batch = 4 B' rows per evaluation, conditioning prepared for them in the order
 * [src_0 .. src_{B'-1}, tgt_*, neg_src_*, neg_tgt_*].  x_src_dev [B',C,H,W]: the source latent; z_dev [B',C,H,W]: the edit at tgrid[0]
 * (normally x_src itself; may be the same buffer); noise_dev [n_grid - 1, B',C,H,W]: the caller's draws, one per interval (the engine owns no
 * RNG); scales_host: n_grid - 1 fp32 pairs (w_s, w_t), the guidance scale of the source and of the target branch - all tensors in the state
 * dtype a->io_dtype (bf16 or f32).  ch = a->cfg_channels, R = rounding to the state dtype, every scalar multiplies in fp32, nothing is
 * contracted.  Per interval i, with t = tgrid[i], omt = fp32(1 - double(t)), dt = fp32(double(tgrid[i+1]) - double(tgrid[i])):
 *   zs  = R(R(x_src t) + R(noise[i] omt))                        the source on the path
 *   zt  = R(zs + R(z - x_src))                                   the edit, shifted by the same amount: z == x_src gives zt == zs exactly (the
 *                                                                left-to-right (z + zs) - x_src would round the small edit delta away)
 *   [c_s, c_t, u_s, u_t] = the PLAIN forward of [zs, zt, zs, zt] at the fp32 time t (lt_forward on 4 B' rows, through the graph cache: one key)
 *   channels <  ch:  v_s = R(u_s + R(w_s R(c_s - u_s)))          v_t = R(u_t + R(w_t R(c_t - u_t)))       forward_with_cfg's expression per branch
 *   channels >= ch:  v_s = c_s                                   v_t = c_t
 *   z' = R(z + R(R(v_t - v_s) dt))
 * Euler only: the rule has no higher-order form.  traj_dev (may be NULL) receives every state [n_grid, B',C,H,W], slot 0 = z; final_dev (may
 * be NULL) the last one.  lt_last_nfe = n_grid - 1, lt_last_eval_rows = 4 B' (n_grid - 1).  Serves every variant lt_forward serves.  No
 * synchronisation, no host read, the caller's stream.  Averaging over several noise draws per interval (n_avg of the paper) is not served.
 * Refused by name with nothing written: a null argument other than traj_dev / final_dev; a stream under capture; n_grid < 2; a->batch that is
 * not a positive multiple of 4 or exceeds max_batch; a latent or io_dtype lt_sample_ode refuses; cfg_channels outside 1..in_channels; a grid
 * value or scale that is not finite; a regional prompt; conditioning prepared for another batch. */
int lt_sample_flowedit(lt_engine* e, const void* z_dev, const void* x_src_dev, const void* noise_dev, void* traj_dev, void* final_dev,
                       const float* tgrid_host, const float* scales_host, int32_t n_grid, const lt_step_args* a, void* stream);

/* Skip-layer guidance (transport/guidance.py: sample_cfg_slg is the definition).  An evaluation can leave out a set S of blocks,
 * which are then the identity on the residual stream: nothing of them is launched, and the block before prepares its output for the next
 * block that runs (the final layer, if none does).  skip_host: n_skip layer indices on the host, in any order.  The set belongs to the call:
 * no entry point returns with one left behind, error returns included.  Refused by name, before anything is launched or written: an index
 * outside 0 .. n_layers - 1, a repeated index, more indices than layers, a set that leaves no layer.
 * lt_forward_skip: lt_forward with the blocks of S left out; n_skip == 0 IS lt_forward.  With a set the call is refused on a stream under
 * capture.
 * lt_forward_cfg_slg: ONE guided evaluation, ch = min(cfg_channels, in_channels), R = rounding to bf16, no contraction:
 *   1. the first B' = batch / 2 rows of x are evaluated with S left out, on the first half of the conditioning (as the conditional-only stage
 *      of lt_sample_ode_cfg_schedule evaluates them); the channels < ch of the bf16 result, k, go to an engine-owned buffer [B', ch, H, W];
 *   2. all 2 B' rows are evaluated; with c, u a sample's cond and uncond word the channels < ch of both halves become
 *        R(R(u + R(w R(c - u))) + R(s R(c - k)))         w = cfg_scale, s = slg_scale, both multiplying in fp32
 *      and the other channels pass row by row.  At cfg_scale == 1 exactly the B' cond rows alone are evaluated, R(c + R(s R(c - k))), written to
 *      rows b and b + B'; the other channels are the cond rows'.
 *   slg_scale == 0: lt_forward_cfg at cfg_scale - its launches, its result (a->cfg_scale is ignored in every case).
 * lt_sample_ode_cfg_slg: lt_sample_ode_cfg_schedule's arguments, behaviour and refusals plus one skip-layer scale per stage (slg_host) and
 * the set.  A stage with s == 0 is the schedule call's stage, the half-row stage at w == 1 included; a stage with s != 0 is the two
 * evaluations above.  lt_last_nfe counts the skip evaluation (stages + the count of s != 0), lt_last_eval_rows adds its B' rows.  A
 * trajectory replays at most five HIP-graph keys (guided, conditional-only, skip, guided + slg, cond + slg) whatever the tables hold.  The
 * buffer (max_batch / 2 * in_channels * max_tokens * patch^2 bf16) is allocated by the first call that needs it, before anything is launched.
 * Not served: packed batches, regional prompts, views, inpainting, SDE, adaptive and multistep methods, a rescale / norm-limit rule, guidance
 * reuse.  Refused by name with nothing written: everything lt_sample_ode_cfg_schedule refuses; the set's refusals; a null or non-finite
 * slg_host / slg_scale; a regional prompt; conditioning prepared for another batch; a stream under capture. */
int lt_forward_skip(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const lt_step_args* a, const int32_t* skip_host,
                    int32_t n_skip, void* stream);
int lt_forward_cfg_slg(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, float cfg_scale, float slg_scale,
                       const int32_t* skip_host, int32_t n_skip, const lt_step_args* a, void* stream);
int lt_sample_ode_cfg_slg(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid, int32_t method,
                          const float* cfg_host, const float* slg_host, const int32_t* skip_host, int32_t n_skip, int32_t t_round_to_state_dtype,
                          const lt_step_args* a, void* stream);

/* Step caching (transport/cache.py: sample_teacache is the definition; the TeaCache rule).  An evaluation may leave the L blocks
 * out and add the residual r = bf16(x_L - x_0) that the stack produced the last time it ran.  Evaluation j = 0 .. ncalls - 1 of a fixed-grid
 * trajectory (ncalls = (n_grid - 1) * stages), R = rounding to bf16:
 *   head       patchify, embedding, conditioning, the first pre-norm + modulate - lt_forward's launches.  x0_j: the token stream before block
 *              0; h_j: the bf16 modulated input of the first block, all M = batch * tokens rows (cond and uncond together).
 *   indicator  for 0 < j < ncalls - 1: S1 = sum |h_j - h_{j-1}|, S0 = sum |h_{j-1}| over all M d words, every difference and sum in float64;
 *              rel = S1 / S0; acc += ((((c0 rel + c1) rel + c2) rel + c3) rel + c4), float64, no contraction.  h_{j-1} <- h_j on every evaluation.
 *   decision   the stack runs on the first and on the last evaluation, when S0 == 0 (acc then takes nothing), and when !(acc < threshold);
 *              whenever it runs acc = 0.  threshold == 0: it always runs.
 *   run        the L blocks, r = R(x_L - x_0) stored, final norm + modulate, final GEMM, closing kernel: the output is lt_forward's /
 *              lt_forward_cfg's for the same input word for word.
 *   reuse      x = R(x0_j + r); the final layer's LayerNorm (no affine, eps 1e-6) + modulate of x with THIS evaluation's modulation, the
 *              rounding chain of the last block's closing kernel; final GEMM, closing kernel.  No block launches anything.
 * lt_sample_ode_cached: lt_sample_ode's arguments, stage times, dt, rounding points and trajectory slots, plus threshold (fp32, >= 0),
 * coef_host (five float64, highest power first; (0, 0, 0, 1, 0) is the identity) and stats_host (NULL, or ncalls x 3 float64: rel, acc after
 * the add, 1 ran / 0 reused; the first and the last evaluation report rel 0, an evaluation with S0 == 0 rel +inf).  The host reads two float64
 * words per evaluation but the first and the last: one stream synchronisation each.  lt_last_nfe = ncalls, lt_last_eval_rows = batch * runs,
 * lt_last_cache_hits = reuses.  A trajectory replays three HIP-graph keys (head, stack + tail, reuse + tail) whatever the threshold.  Three
 * buffers of max_batch * max_tokens * dim bf16 (h_prev, x0, r) are allocated by the first call, before anything is launched.
 * lt_forward_cached: the single evaluations the host loop is built from.  LT_CACHE_PROBE: the head; sums_host[0] = S1, sums_host[1] = S0
 * against the previous probe's h (zeros before the first), out_dev unused (may be NULL).  LT_CACHE_RUN / LT_CACHE_REUSE: the rest of the
 * evaluation whose probe was the engine's last evaluation, with the same step arguments (x_dev is not read again; t_dev is); sums_host unused.
 * Every lt_prepare_prompt* / lt_prepare_labels call forgets the residual and the probe.
 * Serves every variant lt_forward serves, bf16 and f32 states.  Not served, refused by name with nothing written: packed batches, regional
 * prompts, a layer-skip set, guidance schedules / rules / reuse / skip-layer guidance, the multistep and adaptive solvers, inpainting masks,
 * MoE routing record / force, a stream under capture; a null argument; a negative or NaN threshold; a coefficient that is not finite;
 * conditioning prepared for another batch; LT_CACHE_RUN / _REUSE that do not follow their probe; LT_CACHE_REUSE without a stored residual
 * of this shape.  No coefficient set is built in: none has been verified against a trained checkpoint. */
int lt_sample_ode_cached(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid, int32_t method,
                         int32_t use_cfg, int32_t t_round_to_state_dtype, const lt_step_args* a, float threshold, const double* coef_host,
                         double* stats_host, void* stream);
int lt_forward_cached(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, int32_t mode, int32_t use_cfg, const lt_step_args* a,
                      double* sums_host, void* stream);
/* the evaluations of the last lt_sample_ode_cached call that reused the residual */
int64_t lt_last_cache_hits(lt_engine* e);

/* Perturbed-attention guidance (transport/guidance.py: sample_cfg_pag is the definition).  An evaluation can run a set P of
 * blocks PERTURBED: their self-attention map is replaced by the identity, so every query's output is its own value row,
 *   attn[b, n, h, :] = V[b, n, h / (H / Hkv), :]      V: the bf16 V projection of that layer (no norm, no RoPE), copied word for word;
 * the text families (Next-DiT T2I, Flag-DiT) keep their zero-init gated text cross-attention on top - the stand-alone text launch: q_norm + RoPE
 * queries, the key bias, tanh(gate), accumulated onto those rows with that route's rounding points.  The self keys are not used; everything
 * behind (O projection, both gated-residual-norm steps, feed-forward / MoE) is the block as it is.  perturb_host: n_perturb layer indices on
 * the host, in any order; P may hold every layer.  skip_host / n_skip: the set S of lt_forward_skip; S and P are disjoint, either may be empty.
 * The sets belong to the call: no entry point returns with one left behind, error returns included.
 * lt_forward_perturb: lt_forward with the blocks of S left out and the blocks of P perturbed; both empty IS lt_forward.  With a set the call
 * is refused on a stream under capture.
 * lt_forward_cfg_pag: lt_forward_cfg_slg with the third prediction taken under (S, P): R(R(u + R(w R(c - u))) + R(s R(c - p))), at w == 1
 * R(c + R(s R(c - p))); pag_scale == 0: lt_forward_cfg at cfg_scale.
 * lt_sample_ode_cfg_pag: lt_sample_ode_cfg_slg's arguments, behaviour, counters and graph keys with both sets; ONE scale table (pag_host).
 * The perturb set's words join the HIP-graph key behind a mark of their own (-2; the skip set's: -1): skip {1} and perturb {1} are two keys.
 * Refused by name with nothing written: everything the skip-layer entries refuse; for P an index outside 0 .. n_layers - 1, a repeated index,
 * more indices than layers; an index in both sets; both sets empty at a non-zero scale (lt_forward_cfg_pag / lt_sample_ode_cfg_pag); a
 * regional prompt; a stream under capture when a set is given.  Packed batches (size lists) have no entry point that takes a set. */
int lt_forward_perturb(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const lt_step_args* a, const int32_t* skip_host,
                       int32_t n_skip, const int32_t* perturb_host, int32_t n_perturb, void* stream);
int lt_forward_cfg_pag(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, float cfg_scale, float pag_scale,
                       const int32_t* skip_host, int32_t n_skip, const int32_t* perturb_host, int32_t n_perturb, const lt_step_args* a, void* stream);
int lt_sample_ode_cfg_pag(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid, int32_t method,
                          const float* cfg_host, const float* pag_host, const int32_t* skip_host, int32_t n_skip, const int32_t* perturb_host,
                          int32_t n_perturb, int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);

/* Smoothed-energy guidance (SEG; transport/guidance.py: sample_cfg_seg is the definition).  An evaluation can run a set Q of
 * blocks BLURRED: their self-attention reads Gaussian-blurred queries.  The blur acts on the POST-RoPE queries q[B, H, N, hd] (q_norm + RoPE
 * applied, bf16) as an image over the 2-D token grid, per (sample, head, channel), separably: a horizontal pass kept in fp32, a vertical pass
 * on it, ONE rounding to bf16; reflection without repeating the edge; Flag-DiT's end-of-line tokens are copied and are nobody's neighbour.
 * sigma > 0 gives the taps (transport/guidance.py: seg_taps - Gaussian in float64, normalised, rounded once to fp32; radius
 * min(ceil(3 sigma), LT_SEG_MAX_RADIUS)); sigma == +inf: every image query becomes the mean query, RN_bf16 of the float64 sum over the count.
 * Keys, values, and the text families' gated text cross-attention (which reads the UNBLURRED queries, on top, as the stand-alone text launch
 * does) are the block's as it is; so is everything behind the attention.  blur_host: n_blur layer indices on the host, in any order, disjoint
 * from the skip set; Q may hold every layer.  No entry combines a blur set with a perturb set.  The sets belong to the call: no entry point
 * returns with one left behind, error returns included.
 * lt_forward_blur: lt_forward with the blocks of S left out and the blocks of Q blurred; both empty IS lt_forward.
 * lt_forward_cfg_seg: lt_forward_cfg_slg with the third prediction b taken under (S, Q): R(R(u + R(w R(c - u))) + R(s R(c - b))), at w == 1
 * R(c + R(s R(c - b))); seg_scale == 0: lt_forward_cfg at cfg_scale.
 * lt_sample_ode_cfg_seg: lt_sample_ode_cfg_pag's arguments, behaviour, counters and stage rules with the blur set and sigma in place of the
 * perturb set; ONE scale table (seg_host); a stage whose scale is 0 launches no third evaluation; at most five HIP-graph keys per trajectory.
 * The blur set's words join the HIP-graph key behind a mark of their own (-4) with the mode and the radius; the taps live in a device buffer
 * the call writes, so another sigma of the same radius records nothing anew.
 * Refused by name with nothing written: everything the perturbed-attention entries refuse (with "blur" for "perturb"); sigma not positive or
 * NaN; a radius the call's grid cannot reflect (radius > min(rows, columns) - 1 of the image tokens); a packed batch; a regional prompt; a
 * stream under capture when a set is given. */
#define LT_SEG_MAX_RADIUS 31
int lt_forward_blur(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, const lt_step_args* a, const int32_t* skip_host,
                    int32_t n_skip, const int32_t* blur_host, int32_t n_blur, float sigma, void* stream);
int lt_forward_cfg_seg(lt_engine* e, const void* x_dev, const float* t_dev, void* out_dev, float cfg_scale, float seg_scale,
                       const int32_t* skip_host, int32_t n_skip, const int32_t* blur_host, int32_t n_blur, float sigma, const lt_step_args* a,
                       void* stream);
int lt_sample_ode_cfg_seg(lt_engine* e, const void* z_dev, void* traj_dev, void* final_dev, const float* tgrid_host, int32_t n_grid, int32_t method,
                          const float* cfg_host, const float* seg_host, const int32_t* skip_host, int32_t n_skip, const int32_t* blur_host,
                          int32_t n_blur, float sigma, int32_t t_round_to_state_dtype, const lt_step_args* a, void* stream);

/* number of model evaluations issued by the last lt_sample_ode /lt_sample_ode_packed / lt_sample_views / lt_sample_views_guided / lt_sample_sde / lt_sample_ode_adaptive call */
int64_t lt_last_nfe(lt_engine* e);
/* the rows those evaluations ran, summed: nfe * batch for every sampler but lt_sample_ode_cfg_schedule, whose conditional-only stages run half */
int64_t lt_last_eval_rows(lt_engine* e);
/* model evaluations served by replaying a captured HIP graph since lt_create (0 with lt_set_option("graph", 0), and below 1025 rows under the default "graph" 2) */
int64_t lt_graph_replays(lt_engine* e);

/* ---- mixture-of-experts routing hooks (parity tests: hold the discrete top-2 choice equal to a reference run's) ----
 * Tables are host int32 [n_layers][2 branches: 0 time-routed, 1 token-routed][rows][2], rows = batch * tokens of the call, expert
 * ids in ascending order per row; branches a variant does not run are -1.  Both hooks switch HIP-graph replay off while active.
 * record(on): every following forward stores the experts moe_route picked; read() returns the last forward's table.
 * force(sel, rows): the following forwards of exactly `rows` rows use these experts instead of their own top-2 (the softmax
 * weights are still computed from the call's own router logits); force(NULL, 0) ends it. */
int lt_moe_routing_record(lt_engine* e, int32_t on);
int lt_moe_routing_read(lt_engine* e, int32_t* host_out, int32_t rows);
int lt_moe_routing_force(lt_engine* e, const int32_t* host_sel, int32_t rows);

/* ---- profiling hooks (bench.py roofline object) ----------------------------------------------- */
/* class 0 = MFMA GEMM kernel, 1 = attention kernel, 2 = everything else.  When enabled, every
 * launch of that class is bracketed by HIP events on the launch stream. */
int lt_profile_enable(lt_engine* e, int32_t on); /* 0 off, 1 all classes, else bit mask: 1 GEMM | 2 attention | 4 other (1 alone = all) */
/* exact class selection: bit 0 GEMM, bit 1 attention, bit 2 everything else (mask 1 = GEMM launches ONLY; 0 = off) */
int lt_profile_enable_mask(lt_engine* e, int32_t mask);
/* after the caller synchronised the stream: total ms, launches and algorithmic flops per class */
int lt_profile_read(lt_engine* e, int32_t klass, double* ms, int64_t* launches, double* flops);
int lt_profile_reset(lt_engine* e);
/* bracket only the first max_event_launches launches of a class after each reset (the rest are counted, and
 * lt_profile_read scales the measured time to all launches: every NFE has the same launch mix); < 0 = no limit.
 * Event brackets serialise the queue (~1.4 ms per NFE when every launch is bracketed), so bench.py samples. */
int lt_profile_set_budget(lt_engine* e, int32_t klass, int64_t max_event_launches);
/* the same with the bracketed launches taken from the MIDDLE of a run: launches skip_launches .. skip_launches + max_event_launches
 * after a reset (the first launches after an idle queue run in a different power state than the steady stream) */
int lt_profile_set_window(lt_engine* e, int32_t klass, int64_t skip_launches, int64_t max_event_launches);

/* ---- operator-level entry points (parity tests call each kernel through these) ---------------- */
/* C[M,N] = A[M,K] * W[N,K]^T (+bias[N]) ; bf16 in/out, fp32 accumulate.  K % 64 == 0.
 * epilogue 0: plain, 1: SwiGLU on 32-row interleaved W (out has N/2 columns: silu(w1 x) * (w3 x)).
 * variant 0: what the engine uses (kernel picked from the problem size); 1 / 2: 256x256 / 256x288 tiles, classic double-buffered
 * loop; 3: 256x256 8-wave ping-pong; 7 / 8: 128x128 / 64x128 small-M tiles; 15 / 16: ONE persistent 4-wave kernel on 16x16x32 MFMAs,
 * 256x256 / 256x288 tiles, LDS ring and DMA prefetch carried across tile boundaries (K % 64 == 0, K >= 128, no bias) - the engine's
 * kernel for every large dense GEMM.
 * 4-6, 9-14, 17, 18 were study kernels of rounds 1-3 (csrc/experimental/, deleted in round 5) and are refused by name. */
int lt_op_gemm_bf16(const void* A_dev, const void* W_dev, const void* bias_dev, int32_t bias_dtype,
                    void* C_dev, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t variant,
                    void* stream);
/* V projection with the V^T epilogue: vt[b][h][d][perm(tok)] = sum_k A[b * tokens + tok][k] * W[h * hd + d][k] - the attention
 * kernels' transposed, key-permuted V image (lt_op_v_transpose layout with Npad = tokens) written straight from the GEMM.
 * M = B * tokens, tokens % 64 == 0, N = kv_heads * hd; variant 0 auto | 1 256x256 | 2 256x288. */
int lt_op_gemm_vt(const void* A_dev, const void* W_dev, void* vt_dev, int32_t M, int32_t N, int32_t K, int32_t tokens,
                  int32_t hd, int32_t variant, void* stream);
/* fused QKV projection (the engine's form at large M): C[M, N] gets columns [0, split) as a plain GEMM (row stride N; columns >= split
 * are left untouched), vt gets the V columns [split, N) as the transposed image of lt_op_gemm_vt.  One launch of the persistent
 * kernel on 256 x 288 tiles (split and N - split multiples of 288) or, round 3, 256 x 256 tiles (multiples of 256: Flag-DiT 5B);
 * tokens % 64 == 0 (a sample may end inside a row tile), M % tokens == 0, K % 64 == 0, ceil(M / 256) * N / tile width >= #CUs. */
int lt_op_gemm_qkv(const void* A_dev, const void* W_dev, void* C_dev, void* vt_dev, int32_t M, int32_t N, int32_t K, int32_t split,
                   int32_t tokens, int32_t hd, void* stream);
/* 1 if the engine runs this QKV projection as ONE launch (lt_op_gemm_qkv's conditions and the options allow it), else 0 */
int lt_op_gemm_qkv_fusable(int32_t M, int32_t N, int32_t K, int32_t split, int32_t tokens, int32_t hd);
/* round 6: the ROW-PAIR-INTERLEAVED operand layout of the persistent dense GEMM kernel.  Element (r, k) of a dense [rows][cols] bf16 matrix sits at
 * (r >> 1) * 2 cols + (k >> 5) * 64 + (r & 1) * 32 + (k & 31): the 64-byte pieces a 32-deep K slab takes from rows 2 i and 2 i + 1 are ONE 128-byte
 * line, so the kernel's LDS-DMA stream asks the L2 for whole lines (half the requests for the same bytes; the engine keeps the dense blocks'
 * GEMM weights and their activation operands in it whenever all four GEMMs of the block run on that kernel - lumina_dit_debug.h names the switch).
 * lt_op_pair_layout converts in place (to_pair 1: row-major -> pair, 0: back; rows even, cols % 32 == 0, cols <= 16384).
 * lt_op_gemm_bf16_pair = lt_op_gemm_bf16 (no bias, variant 0, shapes that run on the persistent kernel: >= one 256-row tile per CU) with A and W
 * in the pair layout; pair_c != 0 (epilogue 1 only): the [M][N / 2] output is written in it too.  Same products in the same order as the
 * row-major call: bit-identical results. */
int lt_op_pair_layout(void* m_dev, int64_t rows, int32_t cols, int32_t to_pair, void* stream);
int lt_op_gemm_bf16_pair(const void* A_dev, const void* W_dev, void* C_dev, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t pair_c,
                         void* stream);
/* name of the kernel lt_op_gemm_bf16(..., variant) would launch for a dense problem (bench.py labels its roofline line with it) */
int lt_op_gemm_describe(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t variant, char* out, int32_t cap);
/* the routing plan of one mixture-of-experts FFN (what replaces the host loop `for i, expert in enumerate(self.experts): batch_idx, nth =
 * torch.where(selected == i)` of Next-DiT-MoE/models/models2.py:470-476, :499-505): sel_dev int32 [rows][2] = every row's two experts in
 * ascending id (lt_op_attention-style callers write it; with sample_logits_dev != null - bf16 [rows / rows_per_sample][E], the time
 * branch - the kernel routes first and WRITES sel_dev and the bf16 softmax weights wts_dev [rows][2]).  Outputs: pos_dev int32
 * [rows][2] sorted position of each (row, expert) entry; src_dev int32 [max_tiles * 256] row of each sorted position, -1 = padding;
 * tile_expert_dev int32 [max_tiles] expert of each 256-row tile, -1 behind the last segment.  Segments are in expert order, each
 * starts on a tile, entries keep their row order inside a segment.  sel_dev / pos_dev need 4 ints of slack behind the last entry
 * (16-byte accesses); max_tiles * 256 >= 2 rows + E * 255.  Integer work: bit-exact against oracle/moe_plan_oracle.py. */
int lt_op_moe_plan(void* sel_dev, const void* sample_logits_dev, void* wts_dev, int32_t rows, int32_t rows_per_sample, int32_t E, void* pos_dev,
                   void* src_dev, void* tile_expert_dev, int32_t max_tiles, void* stream);
/* lt_op_gemm_bf16 on the 64 x 128 small-M tile with the K range split over two workgroups per tile (round 4: how the engine runs the
 * 512-row O / W2 projections of the 600M models - F.linear of Next-DiT-ImageNet/models/models.py:403, :494).  The caller lends the
 * workspace: part_f32 [tiles][2][64 * 128] floats and counters_u32 [tiles] (zero before the first launch, left zero by every launch);
 * tiles >= ceil(M / 64) * ceil(N / 128), K % 512 == 0, K >= 1024, else the call runs unsplit.  Launches sharing a workspace must be
 * stream-ordered.  Result: bf16(fp32 sum of the two halves' fp32 partial sums) - independent of which half finishes last. */
int lt_op_gemm_splitk(const void* A_dev, const void* W_dev, void* C_dev, int32_t M, int32_t N, int32_t K, void* part_f32_dev,
                      void* counters_u32_dev, int32_t tiles, void* stream);
/* lt_op_gemm_splitk with the tile shape and the split left to the launcher, exactly as the engine calls it (variant 0): slots of
 * [2][64 * 128] floats in part_f32 and one counter each; a dense plain-epilogue small-M problem splits K two ways on 64 x 128 tiles (one slot per
 * tile, K >= 1024) or - round 5, K >= 4096, K % 1024 == 0, 4 x ceil(M / 128) x ceil(N / 128) <= #CUs and <= slots - four ways on 128 x 128 tiles
 * (four slots per tile; the last arriver sums the four fp32 partials in K order), else runs unsplit. */
int lt_op_gemm_splitk_auto(const void* A_dev, const void* W_dev, void* C_dev, int32_t M, int32_t N, int32_t K, void* part_f32_dev,
                           void* counters_u32_dev, int32_t slots, void* stream);
/* grouped (mixture-of-experts) form of lt_op_gemm_bf16 - replaces the per-expert Python loop `for i, expert in
 * enumerate(self.experts): ... expert(x[batch_idx])` of Next-DiT-MoE/models/models2.py:470-476, :499-505 on expert-sorted
 * rows: rows [256 t, 256 t + 256) of A multiply with W_dev + tile_expert[t] * w_expert_stride (elements); tile_expert[t] < 0
 * marks a padding segment whose output rows are left untouched.  M % 256 == 0; tile_expert_dev: int32 [M / 256]. */
int lt_op_gemm_grouped(const void* A_dev, const void* W_dev, const void* tile_expert_dev, int64_t w_expert_stride,
                       void* C_dev, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t variant, void* stream);
/* lt_op_gemm_grouped (plain epilogue) on the persistent kernel with its tail split: when the valid tiles are not a whole number of rounds of the
 * CUs, the tiles of the partial last round are cut along K into 2 / 4 parts; parts hand fp32 accumulators through tail_part_f32_dev
 * ([cap_parts][256 x 256] floats) and count in on counters_u32_dev ([number of CUs] words, zero before the first launch and after every
 * launch); the last part of a tile to arrive sums the parts in K order, so the result does not depend on the arrival order. */
int lt_op_gemm_grouped_tail(const void* A_dev, const void* W_dev, const void* tile_expert_dev, int64_t w_expert_stride, void* C_dev,
                            int32_t M, int32_t N, int32_t K, void* tail_part_f32_dev, void* counters_u32_dev, int32_t cap_parts, void* stream);
/* the same with gather-on-load (round 3: how the engine runs the experts' W1 | W3 GEMM - no gather pass, no expert-sorted copy of
 * the FFN input): row m of the problem is row row_map_dev[m] (int32 [M]) of A_dev [a_rows, K]; -1 = a padding row that reads as
 * zero.  Ping-pong tile kernels (explicit 3 / 7 / 8) and the grouped mode of the persistent 16x16x32 kernel (explicit 15; K >= 256, all of A
 * below 2^30 bytes, at most 1024 row segments); variant 0 picks the persistent kernel from 1.5 tiles of 256 x 256 per CU on (option gemm_w4q_grouped: 2 = from two tiles per CU, 0 = never). */
int lt_op_gemm_grouped_gather(const void* A_dev, int32_t a_rows, const void* row_map_dev, const void* W_dev, const void* tile_expert_dev,
                              int64_t w_expert_stride, void* C_dev, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t variant,
                              void* stream);
/* interleave w1[F,K], w3[F,K] into the packed [2F,K] layout epilogue 1 expects */
int lt_op_pack_w13(const void* w1_dev, const void* w3_dev, void* out_dev, int32_t F, int32_t K,
                   void* stream);
/* out = RMSNorm(x; w, eps) * (1 + scale[b]) (+ shift[b]);  w/scale/shift may be NULL.
 * x,out bf16 [B*N, d]; scale/shift bf16 [B, ld_mod] (row stride ld_mod elements).
 * scale_pre != 0: `scale` already holds bf16(1 + scale) (lt_op_prep_mod), as the engine prepares it once per NFE. */
int lt_op_rmsnorm_mod(const void* x_dev, const void* w_dev, const void* scale_dev,
                      const void* shift_dev, int32_t ld_mod, void* out_dev, int32_t B, int32_t N,
                      int32_t d, float eps, int32_t scale_pre, void* stream);
/* x += gate' * post(y) ; h = pre_next(x) * (1+scale) (+shift)      (model.py:597-610)
 * post_mode 0: y, 1: RMSNorm(y; post_w).  gate_mode 0: gate, 1: tanh(gate), 2: no gate.
 * next_mode 0: none, 1: RMSNorm(x; next_w)(w may be NULL), 2: LayerNorm no-affine (eps_next). */
int lt_op_gated_residual_norm(void* x_dev, const void* y_dev, const void* post_w_dev,
                              const void* gate_dev, int32_t post_mode, int32_t gate_mode,
                              const void* next_w_dev, const void* next_scale_dev,
                              const void* next_shift_dev, int32_t next_mode, int32_t ld_mod,
                              void* h_dev, int32_t B, int32_t N, int32_t d, float eps,
                              float eps_next, int32_t scale_pre, void* stream);
/* y = A W^T (A bf16 [B*N, K], W bf16 [d, K]; `wo` / `w2`, model.py:436-438, :502) followed by the sandwich-norm step on it with the
 * engine's prepared vectors (gate = tanh(gate), next_scale = 1 + scale, both bf16 [B, ld_mod]):
 *   x += gate * RMSNorm(y; post_w) ; h = RMSNorm(x; next_w) * next_scale          (model.py:597-610)
 * use_ystat 1 (what the engine does by default): the projection's epilogue leaves every row's sum of squares in ystat_ws (fp32 [B*N, ystat_cap],
 * ystat_cap >= 2 * ceil(d / 256)) and the row kernel streams; refused when the problem does not take the persistent GEMM kernel.
 * use_ystat 0: the row kernel reduces y itself.  The two differ in the fp32 summation order of that statistic only. */
int lt_op_proj_gated_residual_norm(const void* A_dev, const void* W_dev, void* y_dev, void* ystat_ws_dev, int32_t ystat_cap, int32_t K,
                                   void* x_dev, const void* post_w_dev, const void* gate_dev, const void* next_w_dev,
                                   const void* next_scale_dev, int32_t ld_mod, void* h_dev, int32_t B, int32_t N, int32_t d, float eps,
                                   int32_t use_ystat, void* stream);
/* adaLN vectors, in place (mod bf16 [B, ld_mod] = L layers x `chunks` chunks of d, then the final layer's chunks): chunk c of
 * every layer -> bf16(tanh(.)) if bit c of tanh_mask, bf16(1 + .) if bit c of scale_mask; final_scale_chunk >= 0: that chunk
 * of the final layer -> bf16(1 + .).  The row kernels then run with gate_mode 0 and scale_pre 1. */
int lt_op_prep_mod(void* mod_dev, int32_t B, int32_t ld_mod, int32_t L, int32_t chunks, int32_t d,
                   uint32_t tanh_mask, uint32_t scale_mask, int32_t final_scale_chunk, void* stream);
/* q/k post-processing (model.py:361-371): affine LayerNorm over the full width (optional), 2-D or
 * 1-D RoPE, cast bf16, write head-major [B,heads,N,hd].  src bf16 [B*N, ld_src] at column col0.
 * rope_mode 0 none, 1 2-D interleaved (Next-DiT, model.py:959-961), 2 1-D (Flag-DiT).
 * cs_table_dev float2 [pos][hd/4 or hd/2] (cos,sin); grid_w = latent tokens per row.  out_scale multiplies the
 * result before that one rounding (1.0 = reference layout; the engine folds softmax_scale * log2(e) into K). */
int lt_op_qk_norm_rope(const void* src_dev, int32_t ld_src, int32_t col0, const void* ln_w_dev,
                       const void* ln_b_dev, float ln_eps, void* dst_dev, int32_t B, int32_t N,
                       int32_t heads, int32_t hd, int32_t rope_mode, const void* cs_table_dev,
                       int32_t grid_w, float out_scale, void* stream);
/* V -> transposed, key-permuted layout the attention kernel consumes: [B,kvh,hd,Npad]; key n of a sample sits at position
 * (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1) (bits 2 and 3 of the key index swapped inside every 16 keys), keys >= N are zero */
int lt_op_v_transpose(const void* src_dev, int32_t ld_src, int32_t col0, void* dst_dev, int32_t B,
                      int32_t N, int32_t Npad, int32_t kv_heads, int32_t hd, void* stream);
/* non-causal softmax(q k^T * scale + bias) v  (model.py:392-405 / 427-432).
 * q [B,H,N,hd], k [B,Hkv,Nk,hd], vt [B,Hkv,hd,Nkpad] (lt_op_v_transpose layout), bias float
 * [B,Nkpad] or NULL (0 / -inf per key), out bf16 [B,N,H*hd].
 * accumulate != 0: out = out + tanh(gate[h]) * result (model.py:433-434), gate bf16 [H].
 * k_prescaled != 0: k already carries scale * log2(e) (lt_op_qk_norm_rope out_scale) and `scale` is not applied again. */
int lt_op_attention(const void* q_dev, const void* k_dev, const void* vt_dev, const float* bias_dev,
                    void* out_dev, const void* gate_dev, int32_t accumulate, int32_t B, int32_t H,
                    int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad, int32_t hd, float scale,
                    int32_t k_prescaled, void* stream);
/* name of the kernel lt_op_attention would launch for these arguments under the current options (has_bias: bias_dev != NULL), "none" when
 * no kernel is built for them.  head_dim 128: "attn_fwd_kernel_hd128" for whole 64-key tiles without bias / accumulate (Nk % 64 == 0, Nk == Nkpad),
 * "attn_fwd_kernel<128>" otherwise. */
int lt_op_attention_describe(int32_t has_bias, int32_t accumulate, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad,
                             int32_t hd, char* out, int32_t cap);
/* lt_op_attention / lt_op_attention_fused / lt_op_attention_describe with per-sample key counts (the packed variable-resolution batches of
 * lt_forward_packed) and the pair layout of the output.
 *   nk_dev   DEVICE int32 [B] or NULL (NULL: the plain entry's launch): sample b attends its first nk_dev[b] image keys; Nk stays the layout
 *            stride of k [B,Hkv,Nk,hd] and vt [B,Hkv,hd,Nkpad] and must be a multiple of 64 here.  The caller's contract (a launch cannot
 *            read a device array): 1 <= nk_dev[b] <= Nk, and the K rows / V^T columns of the masked keys hold FINITE words - a masked key's
 *            weight is an exact zero, but 0 x NaN is not zero.  The text keys of the fused form keep tbias; nk_dev bounds the image keys only.
 *            head_dim 72 under attention_variant 4: the one-wave kernel (bit-identical to attention_variant 3); other head dims: the
 *            kernels that take a key bias.
 *   out_pair != 0: out [B*N, H*hd] in the row-pair-interleaved layout of lt_op_pair_layout (one-wave kernels only; B*N even).
 *   describe: has_nk / has_text as nk_dev != NULL / text keys given (Tkpad of them, padded); the kernel name under the current options.
 *            Both instantiations of the head_dim-72 one-wave kernel are named "attn_fwd_kernel_v4<72>". */
int lt_op_attention_nk(const void* q_dev, const void* k_dev, const void* vt_dev, const float* bias_dev, void* out_dev, const void* gate_dev,
                       int32_t accumulate, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad, int32_t hd, float scale,
                       int32_t k_prescaled, const int32_t* nk_dev, int32_t out_pair, void* stream);
int lt_op_attention_fused_nk(const void* q_dev, const void* k_dev, const void* vt_dev, const void* tk_dev, const void* tvt_dev,
                             const float* tbias_dev, const void* tgate_dev, void* out_dev, int32_t B, int32_t H, int32_t Hkv, int32_t N,
                             int32_t Nk, int32_t Nkpad, int32_t Tk, int32_t Tkpad, int32_t hd, const int32_t* nk_dev, int32_t out_pair,
                             void* stream);
int lt_op_attention_nk_describe(int32_t has_bias, int32_t accumulate, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad,
                                int32_t hd, int32_t has_nk, int32_t has_text, int32_t Tkpad, char* out, int32_t cap);
/* The two launches of a layer of the class-conditional 600M models at <= 512 tokens (round 5, option attn_small_fused): the QKV
 * projection on the small-M GEMM tiles, whose epilogue also leaves per-row (sum, sum of squares) of every 128-column tile in
 * rowstat_ws ([M][ceil(3 widths / 128)] float2), then ONE kernel that does q_norm / k_norm (affine LayerNorm over the full width, fp32),
 * 2-D RoPE, the softmax scale fold (k_scale = scale * log2 e) and bf16 rounding of q and k, the V transpose and the attention itself
 * (Next-DiT-ImageNet/models/models.py:358-404).  A [M, K], W [H hd + 2 Hkv hd, K] (q | k | v rows), qkv [M, H hd + 2 Hkv hd] (written),
 * LayerNorm weights / biases bf16 [H hd] / [Hkv hd], cs_table = the (cos, sin) table of lt_op_qk_norm_rope in rope_mode 1 (branch 1 is
 * used), out [M / tokens, tokens, H hd].  head_dim 48, 64 <= tokens <= 512 and tokens % 64 == 0, widths % 128 == 0. */
int lt_op_qkv_attention_small(const void* A_dev, const void* W_dev, void* qkv_dev, int32_t M, int32_t K, int32_t H, int32_t Hkv,
                              int32_t tokens, int32_t hd, const void* q_ln_w, const void* q_ln_b, const void* k_ln_w,
                              const void* k_ln_b, const void* cs_table, int32_t table_len, int32_t grid_w, float k_scale,
                              void* rowstat_ws, void* out_dev, void* stream);
/* self-attention + zero-init gated text cross-attention in ONE launch (hd 72 / 96, attention_variant 3 or 4; model.py:392-434):
 *   out = bf16(softmax(q k^T) v) + bf16(bf16(softmax(q tk^T + tbias) tv) * tanh(tgate[h]))
 * k and tk must already carry their softmax scale * log2(e) (lt_op_qk_norm_rope out_scale); layouts as lt_op_attention,
 * tk [B,Hkv,Tk,hd], tvt [B,Hkv,hd,Tkpad], tbias float [B,Tkpad] (0 / -inf, -inf in the padding), tgate bf16 [H]. */
int lt_op_attention_fused(const void* q_dev, const void* k_dev, const void* vt_dev, const void* tk_dev,
                          const void* tvt_dev, const float* tbias_dev, const void* tgate_dev, void* out_dev, int32_t B,
                          int32_t H, int32_t Hkv, int32_t N, int32_t Nk, int32_t Nkpad, int32_t Tk, int32_t Tkpad,
                          int32_t hd, void* stream);
/* the three kernels of lt_sample_views on caller-owned buffers.  perm / iperm int32 [V][HW], vsign / isign float [V][C] (DEVICE here),
 * HW = H * W (gather / reduce: a multiple of 4), dtype LT_F32 or LT_BF16.  Indices are clamped into [0, HW) before use.
 *   invert: iperm from perm; hits int32 [V * HW + 1] (zeroed by the call) counts the hits per target, its last word the entries that are
 *           out of range or name a target twice: 0 <=> every perm[v] is a bijection
 *   gather: out [V, C, HW] = view_v(y [C, HW]); f0 [V, C, HW] != NULL: the midpoint stage R(view_v(y) + R(f0 * half_dt)) (R: round to dtype)
 *   reduce: out [C, HW] = R(y - R((sum_v inverse_view_v(-R(f [V, C, HW] * dt))) / V)), fp32 sum in view order */
int lt_op_views_invert(const int32_t* perm_dev, int32_t* iperm_dev, int32_t* hits_dev, int32_t V, int32_t HW, void* stream);
int lt_op_views_gather(const void* y_dev, const int32_t* perm_dev, const float* vsign_dev, const void* f0_dev, void* out_dev, float half_dt,
                       int32_t V, int32_t C, int32_t HW, int32_t dtype, void* stream);
int lt_op_views_reduce(const void* y_dev, const void* f_dev, const int32_t* iperm_dev, const float* isign_dev, void* out_dev, float dt,
                       int32_t V, int32_t C, int32_t HW, int32_t dtype, void* stream);
/* the three kernels of lt_forward_tiled on caller-owned buffers.  offsets_host int32 [n][2] = (top, left) (HOST), 1 <= n <= 64 windows of
 * win_h x win_w, every one inside the canvas (refused by name otherwise, before anything is launched); weight_dev float [win_h * win_w]
 * (NULL: ones), dtype LT_F32 or LT_BF16.
 *   gather: out [n, C, win_h, win_w] = the crops of y [C, canvas_h, canvas_w] (exact copies; nothing behind row n - 1 is written)
 *   cover:  wsum float [canvas_h * canvas_w] = per pixel the fp32 sum, in window order, of the weights of the windows that hold it; bad (one
 *           int32, zeroed by the call) counts the pixels whose sum is not finite and above 0
 *   reduce: out [C, canvas_h, canvas_w] = R((sum_k weight * f [n, C, win_h, win_w]) / wsum): transport/tiled.py fuse (R: round to dtype) */
int lt_op_windows_gather(const void* y_dev, const int32_t* offsets_host, int32_t n, int32_t win_h, int32_t win_w, int32_t canvas_h, int32_t canvas_w,
                         void* out_dev, int32_t C, int32_t dtype, void* stream);
int lt_op_windows_reduce(const void* f_dev, const int32_t* offsets_host, int32_t n, int32_t win_h, int32_t win_w, int32_t canvas_h, int32_t canvas_w,
                         const float* weight_dev, const float* wsum_dev, void* out_dev, int32_t C, int32_t dtype, void* stream);
int lt_op_windows_cover(const int32_t* offsets_host, int32_t n, int32_t win_h, int32_t win_w, int32_t canvas_h, int32_t canvas_w,
                        const float* weight_dev, float* wsum_dev, int32_t* bad_dev, void* stream);
/* the two kernels of lt_forward_compose on caller-owned buffers.  1 <= K <= LT_COMPOSE_MAX, Bp = B' >= 1, HW = H * W, dtype LT_F32 or LT_BF16;
 * buffers of any element alignment (the group width 4 / 2 / 1 follows HW and the addresses).  Refused by name before anything is launched: a
 * null argument, a count out of range, cfg_channels outside 1 .. C, a weight that is not finite, an output inside the input's row groups.
 *   replicate: out [(K + 1) Bp, C, HW] = K + 1 exact copies of y [Bp, C, HW]
 *   guidance:  out [Bp, C, HW] = guided_compose (transport/guidance.py) of f [(K + 1) Bp, C, HW] with w_host float [K] (HOST) */
int lt_op_compose_replicate(const void* y_dev, void* out_dev, int32_t K, int32_t Bp, int32_t C, int32_t HW, int32_t dtype, void* stream);
int lt_op_compose_guidance(const void* f_dev, void* out_dev, const float* w_host, int32_t K, int32_t Bp, int32_t C, int32_t HW, int32_t cfg_channels,
                           int32_t dtype, void* stream);
/* one fused step kernel of lt_sample_sde on caller-owned buffers of n elements (any n >= 1; buffers that are not 16-byte aligned take the
 * one-element-per-thread form).  op = LT_SDE_OP_*, rec_host = the stage's LT_SDE_REC floats, dtype LT_F32 or LT_BF16 (R: round to dtype):
 *   EULER      out = R(R(x + R(drift(x, v) * dt)) + R(q * R(w * sqrt_dt)))       drift(x, v) = R(v + R(D * R(R(R(r * v) - x) / var)))
 *   HEUN_XHAT  out = R(x + R(q * R(w * sqrt_dt)))
 *   HEUN_K1    out2 = K1 = drift(x, v),  out = R(x + R(dt * K1))                  (x = xhat)
 *   HEUN_OUT   out = R(x + R(hdt * R(k1 + drift(xp, v))))                         (x = xhat, v = the model at xp, rec = the second stage's)
 *   LAST_MEAN / LAST_TWEEDIE / LAST_EULER: the last-step rules of lt_sample_sde; out is fp32 for the first two.
 * Operands an op does not read may be NULL. */
int lt_op_sde_step(int32_t op, const void* x_dev, const void* v_dev, const void* w_dev, const void* k1_dev, const void* xp_dev, void* out_dev,
                   void* out2_dev, const float* rec_host, int64_t n, int32_t dtype, void* stream);
/* the two state kernels of lt_sample_flowedit on caller-owned buffers (csrc/flowedit.hip; the chains are stated there and above), dtype LT_F32 or
 * LT_BF16, n_half = B' C H W elements per row group:
 *   mix:     out4 [4 B',C,H,W] = [zs, zt, zs, zt] from x_src, z (may be x_src; neither is written) and one interval's noise
 *   combine: z_next [B',C,HW] from z and the evaluation's rows out4 = [c_s, c_t, u_s, u_t]; z_next may be z, not inside out4 */
int lt_op_flowedit_mix(const void* x_src_dev, const void* z_dev, const void* noise_dev, void* out4_dev, float t, float one_minus_t, int64_t n_half,
                       int32_t dtype, void* stream);
int lt_op_flowedit_combine(const void* z_dev, const void* out4_dev, void* z_next_dev, float w_s, float w_t, float dt, int32_t Bp, int32_t C, int32_t HW,
                           int32_t ch, int32_t dtype, void* stream);
/* y[m,n] = sum_k act(a[m,k]) w[n,k] + b[n], m < M <= 8 (GEMV-style; adaLN / embedders).
 * act_in 0 none, 1 SiLU.  a bf16 [M,K], w bf16 [N,K], b bf16 [N] or NULL, y bf16 [M,N]. */
int lt_op_linear_small_m(const void* a_dev, const void* w_dev, const void* b_dev, void* y_dev,
                         int32_t M, int32_t N, int32_t K, int32_t act_in, void* stream);
/* 2-D RoPE (cos,sin) table builder (model.py:915-963): out float2 [2 branches][len][hd/4];
 * branch 0 = linear-interpolation (t < watershed), branch 1 = NTK. */
int lt_op_rope_table_2d(void* out_dev, int32_t len, int32_t hd, float theta, float scale_factor,
                        void* stream);
/* the same table in both layouts the engine keeps (round 4): out float2 [2][len][hd/4] and out_t float2 [2][hd/4][len] (the column
 * factors of the attention prologue: 32 consecutive positions per load) */
int lt_op_rope_table_2d_pair(void* out_dev, void* out_t_dev, int32_t len, int32_t hd, float theta, float scale_factor, void* stream);
/* Round 4, the attn_q_fused path of the engine as two stand-alone steps (model.py:355-371: wq | wk | wv, q_norm, k_norm, RoPE).
 * lt_op_qkv_qstat = lt_op_gemm_qkv (same layouts and conditions; q_cols a multiple of the launch's tile width) whose epilogue also leaves
 * per-row partial (sum, sum of squares) of the bf16-rounded Q columns in qstat_ws (float2 [M][32], scratch), followed by the K pass of
 * lt_op_qk_norm_rope (LayerNorm over the K columns [q_cols, split), 2-D RoPE from cs_table = ONE branch's [len][hd/4] table, out_scale folded in,
 * head-major k_out [B, (split - q_cols) / hd, tokens, hd]) which reduces the partials to q_mean_rstd float2 [M] = (mean, rsqrt(var + 1e-5))
 * of each row's Q columns.
 * lt_op_attention_qraw = lt_op_attention (k prescaled, no bias, head_dim 72, N % 64 == 0) with q == NULL: the kernel builds its query
 * fragments from qkv [B * N, ld] (this head's columns at q_col0 + h * hd) as RoPE(LayerNorm(x; q_mean_rstd, q_ln_w, q_ln_b)) with ONE
 * bf16 rounding - cs_table / cs_table_t from lt_op_rope_table_2d_pair (branch 1), token n at grid position (n / grid_w, n % grid_w). */
int lt_op_qkv_qstat(const void* A_dev, const void* W_dev, void* C_dev, void* vt_dev, int32_t M, int32_t N, int32_t K, int32_t split,
                    int32_t tokens, int32_t hd, int32_t q_cols, const void* k_ln_w_dev, const void* k_ln_b_dev, const void* cs_table_dev,
                    int32_t grid_w, float k_out_scale, void* k_out_dev, void* qstat_ws_dev, void* q_mean_rstd_dev, void* stream);
int lt_op_attention_qraw(const void* qkv_dev, int32_t ld, int32_t q_col0, const void* q_mean_rstd_dev, const void* q_ln_w_dev,
                         const void* q_ln_b_dev, const void* cs_table_dev, const void* cs_table_t_dev, int32_t table_len, int32_t grid_w,
                         const void* k_dev, const void* vt_dev, void* out_dev, int32_t B, int32_t H, int32_t Hkv, int32_t N, int32_t Nkpad,
                         int32_t hd, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LUMINA_DIT_H */
