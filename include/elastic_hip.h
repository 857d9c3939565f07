/*
 * elastic_hip.h -- C ABI of libelastic_hip.so: the MI355X (gfx950) kernels behind the patched global/local
 * denoising loop of ElasticDiffusion.generate_image().
 *
 * The reference (MoayedHajiAli/ElasticDiffusion-official) is pure Python and has NO FFI / plugin boundary; its glue
 * is eager torch ops inside /root/reference/elastic_diffusion.py ("ED:n" below) and
 * /root/reference/elastic_diffusion_w_controlnet.py ("EDC:n").  Each entry point names the reference lines it
 * replaces.  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - return value: hipError_t as int (0 == hipSuccess); never throws, never allocates, never synchronises (one exception:
 *     ed_canny_hysteresis, pre-processing outside the loop, see there);
 *   - image pre-processing entry points (ed_canny_*, ed_resize_*): uint8 images with interleaved channels, integer arithmetic, exact;
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensors), NCHW contiguous unless stated;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); NULL = default stream;
 *   - "dtype" arguments: ED_F32 / ED_F16 / ED_BF16 select the element type of the buffer crossing the torch model
 *     boundary (UNet / VAE / ControlNet tensors).  All latent-space state is fp32;
 *   - latent-space glue entry points (everything up to ed_tile_accumulate_normalise, ed_assemble_rows,
 *     ed_phase_epilogue): arithmetic is fp32 with contraction disabled, in the operation order of the reference's
 *     torch-CPU path, so results are bit-identical to it for fp32 model tensors;
 *   - entry points inside the UNet (ed_geglu .. ed_flash_attention): 16-bit tensors, fp32 math, every value rounded to
 *     the 16-bit type where the torch kernel it replaces rounds; ed_flash_attention accumulates in fp32 on the MFMA
 *     units and rounds the softmax probabilities to the I/O type before the second contraction;
 *   - re-entrant, stateless; one host thread per process, one process per GPU.
 */
#ifndef ELASTIC_HIP_H
#define ELASTIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { ED_F32 = 0, ED_F16 = 1, ED_BF16 = 2 };

/* "prediction_type" arguments of the *_pt entry points: what the scheduler config says the UNet predicts. */
enum { ED_PRED_EPSILON = 0, ED_PRED_V = 1 };

/* ABI version, bumped on any signature change. */
int ed_version(void);

/* Name of the last HIP error code (hipGetErrorString), for the Python wrapper's RuntimeError. */
const char* ed_error_string(int err);

/*
 * ed_gather_views -- ED:706-757 crop_with_context (S == 1: one contiguous window per view) + ED:845 cat, and the
 * pad-to-model-size of ED:404-411 when a view is smaller than the UNet's native size.
 *   latent  f32 [B,C,H,W]
 *   out     dtype [(V*B),C,PH,PW]   row = v*B + b
 *   win_y0/win_x0  int32[V]  window origin in the latent (context included); windows are Sh x Sw
 *   (off_y,off_x)  where the window lands inside the PH x PW row; outside it the row is `frame` (f32 [C,PH,PW],
 *                  the noised-background strips of ED:366-391) or 0 when frame == NULL
 *   Source positions outside the latent read 0 (used by ed_tile_gather_pad).  divisor != 1 divides every value
 *   taken from the latent (IEEE division).
 */
int ed_gather_views(const float* latent, void* out, int dtype, int B, int C, int H, int W,
                    const int32_t* win_y0, const int32_t* win_x0, int V, int Sh, int Sw,
                    int PH, int PW, int off_y, int off_x, const float* frame, float divisor, void* stream);

/*
 * ed_scatter_centres -- ED:852-861: write each view's centre into the full-resolution buffer where it is still
 * exactly 0, in view order (first writer wins, decided by VALUE like the reference's `!= 0` mask).
 * Implemented as a gather per destination pixel over the (<= 2 x 2) views whose centre covers it, ascending view
 * index, stop at the first value != 0; no read-modify-write, `local` need not be zeroed.
 *   pred    dtype [(V*B),C,PH,PW]  UNet output rows, row = v*B + b, view v = rb*n_col_blocks + cb
 *   local   f32 [B,C,H,W]
 *   row_blk int32[H*2]  the row-blocks rb whose centre covers latent row Y (ascending, -1 = none)
 *   row_src int32[H*2]  the row inside the PH x PW prediction that holds latent row Y for that block
 *   col_blk / col_src   same for columns
 */
int ed_scatter_centres(const void* pred, int dtype, float* local, int B, int C, int H, int W,
                       int PH, int PW, int n_col_blocks,
                       const int32_t* row_blk, const int32_t* row_src,
                       const int32_t* col_blk, const int32_t* col_src, void* stream);

/*
 * ed_pick_assemble -- ED:560-630 random_nearest_downsample (value path) + ED:436 cat([latent]*2) + ED:404-411
 * background_pad, for K resampling steps at once.  The random choice itself stays on the host (torch CPU
 * generator, parity): idx holds one pick in [0,4) per reduced pixel and step.
 *   latent  f32 [B,C,H,W]
 *   idx     uint8 [K, h*w]
 *   src_row int32[2h] / src_col int32[2w]  latent row/col behind each line of the 2h x 2w pick grid (ED:565-613)
 *   frame   f32 [C,PH,PW] or NULL; the reduced latent sits at (off_y,off_x) inside the PH x PW model input
 *   out     dtype [(K*2*B),C,PH,PW]  row = (k*2 + j)*B + b, j = 0 uncond copy, 1 cond copy
 *   low     f32 [K,B,C,h,w] or NULL  the picked reduced-resolution latents (ED:678, 686)
 */
int ed_pick_assemble(const float* latent, const uint8_t* idx, const int32_t* src_row, const int32_t* src_col,
                     const float* frame, void* out, int dtype, float* low,
                     int K, int B, int C, int H, int W, int h, int w, int PH, int PW, int off_y, int off_x,
                     void* stream);

/*
 * ed_unpad_direction -- ED:429-430 crop padding + ED:439-440 chunk(2), direction = cond - uncond, for K steps.
 *   unet_out dtype [(K*2*B),C,PH,PW]  rows as written by ed_pick_assemble
 *   dirs     f32 [K,B,C,h,w]
 *   uncond_last f32 [B,C,h,w] or NULL: uncond score of step K-1 (ED:687)
 */
int ed_unpad_direction(const void* unet_out, int dtype, float* dirs, float* uncond_last,
                       int K, int B, int C, int h, int w, int PH, int PW, int off_y, int off_x, void* stream);

/*
 * ed_fill_directions -- ED:633-647 fill_in_from_downsampled_direction applied for K steps in order + ED:688.
 * Per full-resolution pixel: the LAST step whose pick mask covers it supplies the value; if none, step K-1
 * (fill_all).  Value = nearest-upsampled direction of that step at the pixel.
 *   dirs    f32 [K,B,C,h,w]
 *   stamp   int8 [h*w, 4]  stamp[n][q] = last step k whose pick at reduced pixel n was q, -1 if never (built on the
 *                          host from the same draws as idx: the K masks of ED:550-556 folded into one table)
 *   inv_row int32[H*2] / inv_col int32[W*2]  lines of the 2h x 2w pick grid that fold onto latent row/col
 *                                            (ED:446-465 restore_mask_shape, ED:622-628), -1 = none
 *   up_row int32[H] / up_col int32[W]        F.interpolate(nearest) source index reduced<-full (ED:636)
 *   down_row int32[h] / down_col int32[w]    F.interpolate(nearest) source index full<-reduced (ED:688)
 *   target  f32 [B,C,H,W];  low_dir f32 [B,C,h,w] or NULL
 */
int ed_fill_directions(const float* dirs, const int8_t* stamp,
                       const int32_t* inv_row, const int32_t* inv_col,
                       const int32_t* up_row, const int32_t* up_col,
                       const int32_t* down_row, const int32_t* down_col,
                       float* target, float* low_dir,
                       int K, int B, int C, int H, int W, int h, int w, void* stream);

/*
 * ed_cfg_ddim_step -- ED:1031/1053 noise = local + g * direction, then diffusers DDIMScheduler.step (eta = 0,
 * epsilon prediction; call sites ED:1033, 1054):
 *   x0   = (x - sqrt_beta_t * noise) / sqrt_alpha_t
 *   prev = sqrt_alpha_prev * x0 + sqrt_one_minus_alpha_prev * noise
 * All buffers f32 [n]; coefficient scalars are computed on the host in fp32 exactly like diffusers does.
 */
int ed_cfg_ddim_step(const float* local, const float* direction, const float* x, float* prev, float* x0,
                     float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                     float sqrt_one_minus_alpha_prev, int64_t n, void* stream);

/*
 * ed_cfg_ddim_step_pt -- ed_cfg_ddim_step with the scheduler's prediction type as an argument.  ED_PRED_EPSILON is
 * ed_cfg_ddim_step itself (same kernels); ED_PRED_V reads the guided model output m = local + g * direction (formed in
 * model-output space either way, ED:1031) as a velocity, diffusers' v_prediction branch, every product rounded on its own:
 *   x0   = sqrt_alpha_t * x - sqrt_beta_t * m          eps = sqrt_alpha_t * m + sqrt_beta_t * x
 *   prev = sqrt_alpha_prev * x0 + sqrt_one_minus_alpha_prev * eps
 * No division by sqrt_alpha_t, so a zero-terminal-SNR timestep (alpha_bar_t = 0) is well defined.  Any other
 * prediction_type value returns hipErrorInvalidValue.
 */
int ed_cfg_ddim_step_pt(const float* local, const float* direction, const float* x, float* prev, float* x0,
                        float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                        float sqrt_one_minus_alpha_prev, int64_t n, int prediction_type, void* stream);

/*
 * ed_undo_step -- ED:692-704 RePaint re-noising: n_sub sequential x <- a_k * x + b_k * noise_k in registers.
 *   noise f32 [n_sub, n] (drawn on the host generator, parity);  coef f32 [n_sub,2] = (sqrt(1-beta), sqrt(beta))
 */
int ed_undo_step(const float* x_in, const float* noise, const float* coef, float* x_out,
                 int n_sub, int64_t n, void* stream);

/*
 * ed_rrg_update -- ED:885-940 reduced_resolution_guidance on cached low-res scores + ED:1078:
 *   eps_low = low_uncond + g * low_dir;  x0_low = (low_latent - sqrt_beta_t * eps_low) / sqrt_alpha_t
 *   up      = nearest-upsample(x0_low);  out = prev - ((norm * (x0 - up)) * weight)
 * which is the closed form of the reference's autograd of weight * mse_loss(up, x0) w.r.t. x0 (norm = 2/numel of
 * ONE sample, ED:927-936).  Full-res buffers f32 [B,C,H,W], low-res f32 [B,C,h,w].
 */
int ed_rrg_update(const float* prev, const float* x0, const float* low_latent, const float* low_uncond,
                  const float* low_dir, const int32_t* up_row, const int32_t* up_col, float* out,
                  float g, float sqrt_beta_t, float sqrt_alpha_t, float norm, float weight,
                  int B, int C, int H, int W, int h, int w, void* stream);

/*
 * ed_rrg_update_pt -- ed_rrg_update with the prediction type as an argument; with ED_PRED_V the reduced-resolution x0 is
 *   x0_low = sqrt_alpha_t * low_latent - sqrt_beta_t * (low_uncond + g * low_dir)
 * (scheduler.step's pred_original_sample at ED:920), the rest is unchanged.
 */
int ed_rrg_update_pt(const float* prev, const float* x0, const float* low_latent, const float* low_uncond,
                     const float* low_dir, const int32_t* up_row, const int32_t* up_col, float* out,
                     float g, float sqrt_beta_t, float sqrt_alpha_t, float norm, float weight,
                     int B, int C, int H, int W, int h, int w, int prediction_type, void* stream);

/*
 * ed_gather2d -- generic table-driven 2-D gather used for ED:868-883 nearest_interpolate, the ControlNet
 * condition handling (EDC:457-461 zero pad, EDC:932-949 upsample + per-view crop) and debugging:
 *   out[n,c,i,j] = (rows[n,i] < 0 || cols[n,j] < 0) ? 0 : in[src_n[n], c, rows[n,i], cols[n,j]]
 *   in  in_dtype [Bin,C,H,W];  out out_dtype [N,C,oh,ow];  rows int32[N,oh];  cols int32[N,ow];  src_n int32[N]
 */
int ed_gather2d(const void* in, int in_dtype, void* out, int out_dtype, int C, int H, int W,
                const int32_t* src_n, const int32_t* rows, const int32_t* cols, int N, int oh, int ow, void* stream);

/*
 * ed_tile_gather_pad -- ED:287-300: tiles of the zero-padded latent for the tiled VAE decode, already divided by
 * the VAE scaling factor (ED:269).  Same kernel as ed_gather_views with out-of-range reads = 0.
 *   latent f32 [B,C,H,W] -> tiles dtype [(T*B),C,Ts,Ts], tile origin (tile_y0[t]-pad, tile_x0[t]-pad)
 */
int ed_tile_gather_pad(const float* latent, void* tiles, int dtype, int B, int C, int H, int W,
                       const int32_t* tile_y0, const int32_t* tile_x0, int T, int Ts, float scaling_factor,
                       void* stream);

/*
 * ed_tile_accumulate_normalise -- ED:271 (img/2 + 0.5).clamp(0,1) per tile, ED:303-308 image += centre;
 * count += 1; image / count.  Gather form: per output pixel, sum the covering tiles in ascending tile order.
 *   decoded dtype [(T*B),Cimg,TP,TP] raw VAE output (TP = Ts*scale), row = t*B + b, tile t = rb*n_col_tiles + cb
 *   image   f32 [B,Cimg,HP,WP]
 *   row_tile int32[HP*MAXC] / row_src int32[HP*MAXC]: tiles (row index rb, ascending, -1 = none) covering pixel
 *   row Y and the row inside the decoded tile; same for columns.  MAXC = ED_TILE_MAXC.
 */
#define ED_TILE_MAXC 4
int ed_tile_accumulate_normalise(const void* decoded, int dtype, float* image, int B, int Cimg, int HP, int WP,
                                 int TP, int n_col_tiles,
                                 const int32_t* row_tile, const int32_t* row_src,
                                 const int32_t* col_tile, const int32_t* col_src, void* stream);

/* ---- fused memory-bound kernels inside the UNet (model side of the boundary ED:422-426; csrc/unet_kernels.hip) ---- */

/*
 * ed_geglu -- the GEGLU activation of the transformer feed-forward (diffusers GEGLU, reached through ED:422):
 *   out[m,i] = in[m,i] * gelu(in[m,I+i])   (exact erf GELU), 16-bit in/out, fp32 math, torch's rounding points.
 *   in dtype [M, 2I] row-major, out dtype [M, I]; I % 8 == 0; dtype = ED_F16 | ED_BF16.
 */
int ed_geglu(const void* in, void* out, int dtype, int64_t M, int I, void* stream);

/*
 * ed_groupnorm -- GroupNorm over NCHW 16-bit activations with optional fused SiLU (ResnetBlock2D norm1/norm2,
 * conv_norm_out) and optional [N,HW,C] token-layout output (Transformer2DModel.norm + the permute that follows).
 *   x dtype [N,C,HW] (NCHW contiguous), gamma/beta dtype [C], out dtype [N,C,HW] or [N,HW,C];
 *   conv_bias dtype [C] or NULL, chan_bias dtype [N,C] or NULL: when given, the tensor that is normalised is
 *   round16(round16(x + conv_bias[c]) + chan_bias[n,c]) -- the bias of the convolution that produced x (run bias-free:
 *   MIOpen would add it in a separate broadcast kernel) and the time-embedding add `h + temb[:, :, None, None]` that
 *   precedes norm2 in ResnetBlock2D, folded into both passes with the roundings of the kernels they replace;
 *   workspace: caller-owned fp32 scratch of ed_groupnorm_workspace(N, C, HW, G) bytes, or NULL.  Groups larger than
 *   64 K elements are then normalised by two fully parallel launches (per-chunk Welford partials, merged in order --
 *   deterministic) instead of one workgroup per (sample, group); with NULL (or small groups: workspace size 0) the
 *   single-launch kernel runs.  Statistics (here and in every ed_groupnorm_* below): fp32 sums of x - K and (x - K)^2 with K the
 *   group's first element as normalised, so the variance keeps its digits when the mean is large next to the spread.
 *   HW % 8 == 0, C % G == 0 (and (C/G) % 4 == 0 for tokens_out); dtype = ED_F16 | ED_BF16.
 */
int ed_groupnorm(const void* x, const void* gamma, const void* beta, const void* conv_bias, const void* chan_bias,
                 void* out, float* workspace, int dtype, int N, int C, int HW, int G, float eps, int act_silu,
                 int tokens_out, void* stream);
int64_t ed_groupnorm_workspace(int N, int C, int HW, int G);

/*
 * ed_bias_residual_add -- ResnetBlock2D's closing add with the convolution biases folded in:
 *   out[n,c,p] = round16(res[n,c,p] (+ res_bias[c])) + round16(h[n,c,p] + h_bias[c])
 * h = conv2 output (bias-free), res = the block input or the bias-free 1x1 shortcut convolution; either bias may be NULL.
 * 16-bit; channels_last == 0: [N,C,HW] NCHW contiguous, HW % 8 == 0; channels_last != 0: [N,HW,C] memory (torch
 * channels_last), C % 8 == 0; dtype = ED_F16 | ED_BF16.
 */
int ed_bias_residual_add(const void* h, const void* h_bias, const void* res, const void* res_bias, void* out, int dtype,
                         int N, int C, int HW, int channels_last, void* stream);

/*
 * ed_layernorm -- LayerNorm over the last dimension of [M, D] 16-bit activations (BasicTransformerBlock.norm1/2/3):
 * one wavefront per row, two passes over registers (mean, centred variance), one read + one write per element.
 *   D % 8 == 0, D <= 2048; gamma / beta dtype [D]; dtype = ED_F16 | ED_BF16.
 */
int ed_layernorm(const void* x, const void* gamma, const void* beta, void* out, int dtype, int64_t M, int D, float eps,
                 void* stream);
/*
 * ---- the fp32-residual-stream mode of the UNet (round 6; models.UNet2DConditionModel.residual_fp32) -----------------------------
 * The tolerance mode for configurations whose plain-fp16 latent ends outside north_star's 1e-3 (cfg2): the tensor that persists from
 * block to block is fp32, every branch computes in the 16-bit model dtype.  These entry points are the memory-bound layers that READ
 * the stream: same arithmetic as their 16-bit namesakes, x (ed_layernorm_s32, ed_groupnorm_nhwc_s32) or b and sum_out
 * (ed_add_layernorm_s32: sum_out = a + b in fp32, unrounded) are fp32, everything else -- gamma, beta, a, out -- has `dtype`.
 * ed_groupnorm_nhwc_s32 takes no folded biases and applies a (x - mean) + beta (the 16-bit namesake: a x + (beta - a mean));
 * workspace: ed_groupnorm_nhwc_workspace.  Same shape limits as the namesakes.
 */
int ed_layernorm_s32(const void* x, const void* gamma, const void* beta, void* out, int dtype, int64_t M, int D, float eps,
                     void* stream);
int ed_add_layernorm_s32(const void* a, const void* b, const void* gamma, const void* beta, void* sum_out, void* out,
                         int dtype, int64_t M, int D, float eps, void* stream);
int ed_groupnorm_nhwc_s32(const void* x, const void* gamma, const void* beta, void* out, float* workspace, int dtype, int N, int C,
                          int HW, int G, float eps, int act_silu, void* stream);

/*
 * ed_add_layernorm -- residual add + LayerNorm in one pass (BasicTransformerBlock: `x = attn(norm(x)) + x` and the
 * `norm(x)` that follows): sum_out = round16(a + b), out = LayerNorm(sum_out).  [M, D] 16-bit, same limits as
 * ed_layernorm; sum_out may alias a or b.
 */
int ed_add_layernorm(const void* a, const void* b, const void* gamma, const void* beta, void* sum_out, void* out,
                     int dtype, int64_t M, int D, float eps, void* stream);

/*
 * ed_tokens_add_nchw -- out[n,c,p] = x[n,c,p] + tokens[n,p,c]: the residual add that closes a Transformer2DModel
 * (token layout back to NCHW), through a 64 x 64 LDS tile so both layouts are read / written with 16-byte vectors.
 *   x, out dtype [N,C,HW]; tokens dtype [N,HW,C]; C % 64 == 0, HW % 64 == 0; dtype = ED_F16 | ED_BF16.
 */
int ed_tokens_add_nchw(const void* x, const void* tokens, void* out, int dtype, int N, int C, int HW, void* stream);

/*
 * ed_groupnorm_nhwc -- the same GroupNorm [+ SiLU] for channels-last activations: x / out dtype [N, HW, C] (the memory
 * of an NCHW tensor in torch.channels_last format, which is also the transformer's token layout).  Three launches
 * (partial sums of x - K per group, finalise in double, vectorised apply); `workspace` is caller-owned fp32 scratch of
 * ed_groupnorm_nhwc_workspace(N, C, HW, G) bytes.  conv_bias [C] / chan_bias [N,C] (optional) as in ed_groupnorm.
 * C % 8 == 0, C % G == 0, C / G >= 8, G <= 256; dtype = ED_F16 | ED_BF16.
 */
int ed_groupnorm_nhwc(const void* x, const void* gamma, const void* beta, const void* conv_bias, const void* chan_bias,
                      void* out, float* workspace, int dtype, int N, int C, int HW, int G, float eps, int act_silu,
                      void* stream);
int64_t ed_groupnorm_nhwc_workspace(int N, int C, int HW, int G);

/*
 * ed_groupnorm_nhwc_cat -- ed_groupnorm_nhwc of cat([x1, x2], channel axis) without the concatenated tensor ever existing: the up
 * blocks' `ResnetBlock2D(torch.cat([hidden, skip], 1))` (diffusers' CrossAttnUpBlock2D / UpBlock2D behind ED:393-432) reads the two
 * channels-last sources in place.  x1 dtype [N, HW, C1], x2 dtype [N, HW, C2], out dtype [N, HW, C1 + C2]; C1 % 8 == 0 (a 16-byte
 * vector never straddles the sources; a GROUP may: the statistics are per-column sums).  No folded biases.  Same limits on
 * C = C1 + C2 and G as ed_groupnorm_nhwc; workspace: ed_groupnorm_nhwc_workspace(N, C1 + C2, HW, G).  Bit-identical to
 * ed_groupnorm_nhwc on the materialised concatenation.
 */
int ed_groupnorm_nhwc_cat(const void* x1, const void* x2, const void* gamma, const void* beta, void* out, float* workspace, int dtype,
                          int N, int C1, int C2, int HW, int G, float eps, int act_silu, void* stream);

/*
 * ed_assemble_rows -- ed_pick_assemble + ed_gather_views in one launch: all rows of one fused model batch (K CFG pairs
 * of the randomly picked reduced latent + V context crops).  Arguments as in those two entry points ("g" = the global /
 * pick part with its own PH x PW and offsets, "v" = the view part); bit-identical to calling them one after the other.
 */
int ed_assemble_rows(const float* latent, int B, int C, int H, int W, const uint8_t* idx, const int32_t* src_row,
                     const int32_t* src_col, const float* gframe, void* g_rows, float* low, int K, int h, int w, int gPH,
                     int gPW, int g_off_y, int g_off_x, const int32_t* win_y0, const int32_t* win_x0,
                     const float* vframe, void* v_rows, int V, int Sh, int Sw, int vPH, int vPW, int v_off_y, int v_off_x,
                     int dtype, void* stream);

/*
 * ed_assemble_rows_x -- ed_assemble_rows for a model whose input rows carry E extra channels behind the C latent channels (the
 * 9-channel inpainting UNets: E = 5, the latent mask and the masked-image latent).  An addition, no
 * signature change, so still ABI v13.  Arguments as ed_assemble_rows, plus
 *   extra      f32 [B,E,H,W]  at the latent's resolution; no alignment condition
 *   pad_value  f32 [E]        (device) what channel C + e holds wherever a latent channel reads the frame (or 0 without one)
 * g_rows [(K*2*B),C+E,gPH,gPW] and v_rows [(V*B),C+E,vPH,vPW].  Channels 0..C-1 and `low` ([K,B,C,h,w]: the latent channels only)
 * are bit-identical to ed_assemble_rows; channel C + e is the SAME gather applied to extra[:, e] -- the pick (idx, src_row, src_col) of
 * that resampling step in a global row, the window (win_y0, win_x0) in a view row -- converted to `dtype` the same way.  One launch;
 * the 4-wide forms under ed_assemble_rows' conditions, the same bits as the scalar forms.  extra / pad_value NULL, E < 1 or a
 * window that does not fit its row are hipErrorInvalidValue before any launch.
 */
int ed_assemble_rows_x(const float* latent, int B, int C, int H, int W, const uint8_t* idx, const int32_t* src_row,
                       const int32_t* src_col, const float* gframe, void* g_rows, float* low, int K, int h, int w, int gPH,
                       int gPW, int g_off_y, int g_off_x, const int32_t* win_y0, const int32_t* win_x0,
                       const float* vframe, void* v_rows, int V, int Sh, int Sw, int vPH, int vPW, int v_off_y, int v_off_x,
                       int dtype, const float* extra, int E, const float* pad_value, void* stream);

/*
 * ed_phase_epilogue -- everything between the model call and the next latent in one launch: ed_unpad_direction +
 * ed_fill_directions + ed_scatter_centres + ed_cfg_ddim_step and, when x_next != NULL, ed_rrg_update
 * (ED:429-443, 633-647 x K, 688, 852-861, 1031/1053 + scheduler.step, 886-940 + 1078).  Every output element is a gather
 * over the model output rows, so no intermediate (dirs / direction / local) ever goes through HBM.  Bit-identical to the
 * chain of separate entry points (same fp32 operation order).
 *   g_out dtype [(K*2*B),C,gPH,gPW], v_out dtype [(V*B),C,vPH,vPW]: model output rows; x f32 [B,C,H,W] the latent the
 *   phase started from; stamp / inv_* / up_* / down_* as ed_fill_directions; row_blk .. col_src as ed_scatter_centres;
 *   prev, x0 f32 [B,C,H,W] (always written); low_dir, uncond_last f32 [B,C,h,w] and direction, local f32 [B,C,H,W] are
 *   optional by-products (NULL = skip); x_next f32 [B,C,H,W] (optional) = prev + RRG term, needs low_latent f32 [B,C,h,w]
 *   (the last picked reduced latent, ed_pick_assemble's `low[K-1]`), rrg_norm = 2/(C*H*W) and rrg_weight.
 */
int ed_phase_epilogue(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                      const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                      const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                      const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                      float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                      int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                      int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                      float sqrt_1m_alpha_prev, float rrg_norm, float rrg_weight, void* stream);

/*
 * ed_phase_epilogue_pt -- ed_phase_epilogue with the prediction type as an argument (still one launch): the DDIM update
 * is ed_cfg_ddim_step_pt's and the fused RRG term ed_rrg_update_pt's; bit-identical to that chain.  ED_PRED_EPSILON
 * launches the kernels ed_phase_epilogue launches.
 */
int ed_phase_epilogue_pt(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                         const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                         const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                         const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                         float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                         int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                         int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                         float sqrt_1m_alpha_prev, float rrg_norm, float rrg_weight, int prediction_type, void* stream);

/*
 * ---- guidance rescale (arXiv 2305.08891 section 3.4; the reference's rescale_noise_cfg, ED:800-811) ----
 * Wherever a guided model output m_cfg = local + g * direction is handed to the DDIM update (ED:1031, 1053) or to the
 * reduced-resolution x0 of RRG (ED:920), guidance_rescale > 0 replaces it by
 *   m = gr * (m_cfg * ratio[b]) + omgr * m_cfg,   ratio[b] = std(m_text[b]) / std(m_cfg[b]),   m_text = local + direction
 * with the unbiased std over all elements of sample b, gr = float32(guidance_rescale), omgr = float32(1 - guidance_rescale).
 * The elementwise part rounds every product and sum on its own in that order (bit-identical to torch on the CPU given the
 * same ratio); ratio is a float[B] DEVICE buffer written by one of the two moments entry points and read by the *_gr
 * consumers -- nothing synchronises the host.
 *
 * The moments entry points reduce deterministically (fixed partial layout in the caller's workspace, partials merged in a
 * fixed order by a second tiny launch, no atomics), in fp64 with shifted sums: each std is the fp32 rounding of its fp64
 * value, the ratio one fp32 division.  ed_guidance_moments_workspace -> bytes needed (8-byte aligned buffer) for B samples
 * of n_full elements plus, when n_low > 0, the reduced-resolution pair of n_low elements.
 */
int64_t ed_guidance_moments_workspace(int B, int64_t n_full, int64_t n_low);

/*
 * ed_guidance_moments -- ratio[b] for flat f32 buffers local, direction [B, n] and guidance g (the un-fused path and the
 * reduced-resolution pair uncond_last / low_dir).  text f32 [B, n] (optional): m_text as a tensor instead of
 * local + direction -- plain CFG (generate(), ED:761-796), where noise_pred_text is the conditional prediction itself.
 * workspace: ed_guidance_moments_workspace(B, n, 0) bytes.
 */
int ed_guidance_moments(const float* local, const float* direction, const float* text, float g, int B, int64_t n,
                        float* ratio, void* workspace, void* stream);

/*
 * ed_phase_moments -- the same ratios over the gathers of ed_phase_epilogue (same tables and model output rows; direction /
 * local still never go through HBM): ratio f32 [B] over (C,H,W) of local + g * direction and, when ratio_low != NULL,
 * ratio_low f32 [B] over (C,h,w) of uncond_last + g * low_dir (the pair of the fused RRG term).
 * workspace: ed_guidance_moments_workspace(B, C*H*W, ratio_low ? C*h*w : 0) bytes.
 */
int ed_phase_moments(const void* g_out, const void* v_out, int dtype, const int8_t* stamp, const int32_t* inv_row,
                     const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col, const int32_t* down_row,
                     const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src, const int32_t* col_blk,
                     const int32_t* col_src, float* ratio, float* ratio_low, void* workspace, int K, int B, int C, int H,
                     int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW, int n_col_blocks,
                     float g, void* stream);

/*
 * ed_cfg_ddim_step_gr / ed_rrg_update_gr / ed_phase_epilogue_gr -- the *_pt entry points with the rescale applied to the
 * guided model output (ratio f32 [B]; B samples of n / B elements for the flat step) and, in the RRG term, to the
 * reduced-resolution one (ratio_low f32 [B]; required by ed_phase_epilogue_gr when both ratio and x_next are given).
 * A NULL ratio launches exactly the kernels the *_pt entry point launches.
 */
int ed_cfg_ddim_step_gr(const float* local, const float* direction, const float* x, float* prev, float* x0,
                        float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                        float sqrt_one_minus_alpha_prev, int64_t n, int prediction_type, const float* ratio, float gr,
                        float omgr, int B, void* stream);
/*
 * ed_cfg_ddim_step_width -- launches nothing: the elements per thread (4 = the 16-byte kernels, 1 = the scalar ones) that
 * ed_cfg_ddim_step / _pt / _gr choose for these buffers, by the very predicate they launch by (ratio NULL = the plain entry
 * points, B ignored).  0 = arguments ed_cfg_ddim_step_gr refuses.  For tests and callers that want to know which path runs.
 */
int ed_cfg_ddim_step_width(const float* local, const float* direction, const float* x, const float* prev, const float* x0,
                           int64_t n, const float* ratio, int B);
int ed_rrg_update_gr(const float* prev, const float* x0, const float* low_latent, const float* low_uncond,
                     const float* low_dir, const int32_t* up_row, const int32_t* up_col, float* out,
                     float g, float sqrt_beta_t, float sqrt_alpha_t, float norm, float weight,
                     int B, int C, int H, int W, int h, int w, int prediction_type, const float* ratio_low, float gr,
                     float omgr, void* stream);
int ed_phase_epilogue_gr(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                         const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                         const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                         const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                         float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                         int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                         int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float sqrt_alpha_prev,
                         float sqrt_1m_alpha_prev, float rrg_norm, float rrg_weight, int prediction_type,
                         const float* ratio, const float* ratio_low, float gr, float omgr, void* stream);

/*
 * DPM-Solver++(2M): the multistep update in the places of the DDIM one.
 *
 * ed_cfg_ddim_step_ms / ed_phase_epilogue_ms -- the *_gr entry points (same arguments, same x0 = the DDIM step's
 * pred_original_sample of the guided, rescaled model output, same by-products, same fused RRG term) with the sample update
 *     prev = (c_x * x - b * x0) - half_b * (r_inv * (x0 - x0_hist))
 * evaluated left to right in fp32, every product rounded on its own.  The host passes c_x = sigma_prev / sigma_t,
 * b = alpha_prev * (exp(-h) - 1), half_b = 0.5 * b and r_inv = h / h0 in the places of sqrt_alpha_prev and
 * sqrt_1m_alpha_prev.  x0_hist f32 [n] (the flat step) / [B,C,H,W] (the epilogue) is the previous timestep's x0 at the output
 * element's index; NULL launches the first-order form prev = c_x * x - b * x0, which reads neither x0_hist nor half_b / r_inv.
 * The choice is per launch (two kernel instantiations), never per element.
 * hipErrorInvalidValue before any launch: a prediction_type other than ED_PRED_*, what the *_gr entry point refuses, and an
 * x0_hist that shares an element with prev or x0.  The 16-byte form of the flat step runs under ed_cfg_ddim_step_width's
 * conditions and, with a history, x0_hist 16-byte aligned; the scalar form otherwise.
 */
int ed_cfg_ddim_step_ms(const float* local, const float* direction, const float* x, float* prev, float* x0,
                        float g, float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b, float r_inv,
                        int64_t n, int prediction_type, const float* ratio, float gr, float omgr, int B,
                        const float* x0_hist, void* stream);
int ed_phase_epilogue_ms(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                         const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                         const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                         const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                         float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                         int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                         int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b,
                         float r_inv, float rrg_norm, float rrg_weight, int prediction_type, const float* ratio,
                         const float* ratio_low, float gr, float omgr, const float* x0_hist, void* stream);

/*
 * Stochastic samplers: DDIM with eta > 0 ("Euler a" is eta = 1), SDE-DPM-Solver++(2M) and LCM are the
 * deterministic update with other host scalars plus one term,
 *     prev = <the update> + c_n * noise,
 * the product rounded on its own, added last.  noise f32 [n] / [B,C,H,W] is read at the output element's index; the host draws it.
 *
 * ed_cfg_ddim_step_sde / ed_phase_epilogue_sde -- the *_ms entry points plus `form`, `c_n` and `noise`.
 *   form ED_FORM_DDIM:       prev = (c_x * x0 + b * eps) + c_n * noise -- the DDIM update of the *_gr entry points with c_x / b in
 *                            the places of sqrt_alpha_prev / sqrt_1m_alpha_prev (the host passes (1 - abar_prev - c_n^2)^0.5 as b);
 *                            half_b / r_inv are unused and x0_hist must be NULL.
 *   form ED_FORM_MULTISTEP:  prev = ((c_x * x - b * x0) - half_b * (r_inv * (x0 - x0_hist))) + c_n * noise, first order with a
 *                            NULL x0_hist as in *_ms.  LCM is this form at first order with its own c_x, b, c_n.
 * The fused RRG output x_next is formed from the prev that carries the noise.  c_n == 0 is not a stochastic step: the
 * deterministic kernels are launched and `noise` is not read.
 * hipErrorInvalidValue before any launch: what the *_ms entry point refuses, a NULL noise, a non-finite c_n, a form other
 * than ED_FORM_*, an x0_hist with ED_FORM_DDIM, and a noise that shares an element with prev, x0 or x_next.  The 16-byte form of
 * the flat step additionally needs noise 16-byte aligned; the scalar form otherwise.
 */
enum { ED_FORM_DDIM = 0, ED_FORM_MULTISTEP = 1 };
int ed_cfg_ddim_step_sde(const float* local, const float* direction, const float* x, float* prev, float* x0,
                         float g, float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b, float r_inv,
                         int64_t n, int prediction_type, const float* ratio, float gr, float omgr, int B,
                         const float* x0_hist, int form, float c_n, const float* noise, void* stream);
int ed_phase_epilogue_sde(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                          const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                          const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                          const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                          float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                          int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                          int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b,
                          float r_inv, float rrg_norm, float rrg_weight, int prediction_type, const float* ratio,
                          const float* ratio_low, float gr, float omgr, const float* x0_hist, int form, float c_n,
                          const float* noise, void* stream);

/*
 * Regional prompts: P = n + 1 conditional rows per resampling step and sample -- the base prompt and n
 * regions, 1 <= P <= 8 -- whose class directions cond_p - uncond are summed per pixel with the weights region_w f32 [P,H,W].
 * Model rows are step-major: [(K*(1+P)*B),C,gPH,gPW], within a step uncond first, then cond 0..P-1, each x B.  Additions, no
 * signature change: still ABI v13.  Every entry point below returns hipErrorInvalidValue before any launch for P (n + 1; copies - 1)
 * outside 1..8, for a NULL region_w with P > 1 and for a region_w that shares memory with an output.
 *
 * ed_region_weights -- masks u8 [n,HW] (255 = the region) and weights (a HOST array of n floats, each > 0) -> region_w f32 [n+1,HW],
 * plane 0 the base prompt's.  Per pixel, in fp32, each operation rounded on its own:
 *     r_p = weight_p * (m_p / 255),  s = r_1 + .. + r_n (in order),  r_0 = max(0, 1 - s),  tot = r_0 + s,  w_p = r_p / tot.
 * One launch; 4 pixels per thread when HW % 4 == 0 and the buffers allow, the same bits as the scalar form.
 *
 * ed_assemble_rows_n -- ed_assemble_rows_x with `copies` (2..9) rows written per resampling step and sample in the place of the fixed
 * 2: g_rows [(K*copies*B),C+E,gPH,gPW].  extra / pad_value may be NULL with E = 0.  The picked vector is gathered once and stored
 * `copies` times; copies = 2 gives the bits of ed_assemble_rows (E = 0) / ed_assemble_rows_x.
 *
 * ed_region_blend -- the un-fused path: out f32 [planes,HW] = sum_p region_w[p,HW] * dirs[p,planes,HW] (dirs f32, the P directions
 * of ed_unpad_direction + ed_fill_directions on the (uncond, cond_p) pair rows), with the rule of the fused kernels: a term whose
 * weight is 0 is skipped (its direction is not read), the first term that is not starts the sum, the rest are added in order of p;
 * 0 where every weight is 0.
 *
 * ed_phase_epilogue_rg -- ed_phase_epilogue_ms' argument list, then `multistep` (1: the DPM-Solver++ update as there; 0: the DDIM
 * update of ed_phase_epilogue_gr, with sqrt_alpha_prev / sqrt_1m_alpha_prev in the places of c_x / b and half_b, r_inv, x0_hist
 * unused -- x0_hist must be NULL), then region_w and P.  The direction of a pixel is the weighted sum above over the P cond rows of
 * its covering step (zero-weight rows are not read); everything else -- low_dir at (down_row, down_col), the rescale, the update,
 * the fused RRG term, the by-products -- is ed_phase_epilogue_ms' with that direction.  One launch.  A NULL region_w with P = 1
 * launches exactly what ed_phase_epilogue_ms / ed_phase_epilogue_gr launch.
 *
 * ed_phase_moments_rg -- ed_phase_moments over the same regional direction; a NULL region_w with P = 1 is ed_phase_moments.
 */
int ed_region_weights(const uint8_t* masks, const float* weights, int n, int64_t HW, float* region_w, void* stream);
int ed_assemble_rows_n(const float* latent, int B, int C, int H, int W, const uint8_t* idx, const int32_t* src_row,
                       const int32_t* src_col, const float* gframe, void* g_rows, float* low, int K, int h, int w, int gPH,
                       int gPW, int g_off_y, int g_off_x, const int32_t* win_y0, const int32_t* win_x0,
                       const float* vframe, void* v_rows, int V, int Sh, int Sw, int vPH, int vPW, int v_off_y, int v_off_x,
                       int dtype, const float* extra, int E, const float* pad_value, int copies, void* stream);
int ed_region_blend(const float* dirs, const float* region_w, float* out, int P, int planes, int64_t HW, void* stream);
int ed_phase_epilogue_rg(const void* g_out, const void* v_out, int dtype, const float* x, const int8_t* stamp,
                         const int32_t* inv_row, const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col,
                         const int32_t* down_row, const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src,
                         const int32_t* col_blk, const int32_t* col_src, const float* low_latent, float* prev, float* x0,
                         float* x_next, float* low_dir, float* uncond_last, float* direction, float* local, int K, int B,
                         int C, int H, int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW,
                         int n_col_blocks, float g, float sqrt_beta_t, float sqrt_alpha_t, float c_x, float b, float half_b,
                         float r_inv, float rrg_norm, float rrg_weight, int prediction_type, const float* ratio,
                         const float* ratio_low, float gr, float omgr, const float* x0_hist, int multistep,
                         const float* region_w, int P, void* stream);
int ed_phase_moments_rg(const void* g_out, const void* v_out, int dtype, const int8_t* stamp, const int32_t* inv_row,
                        const int32_t* inv_col, const int32_t* up_row, const int32_t* up_col, const int32_t* down_row,
                        const int32_t* down_col, const int32_t* row_blk, const int32_t* row_src, const int32_t* col_blk,
                        const int32_t* col_src, float* ratio, float* ratio_low, void* workspace, int K, int B, int C, int H,
                        int W, int h, int w, int gPH, int gPW, int g_off_y, int g_off_x, int vPH, int vPW, int n_col_blocks,
                        float g, const float* region_w, int P, void* stream);

/*
 * ed_flash_attention -- fused attention forward of the UNet's transformer blocks (what diffusers' AttnProcessor2_0
 * does with F.scaled_dot_product_attention inside `self.unet(...)`, ED:422-426): out = softmax(scale * Q K^T) V per
 * (batch, head), never materialising the Nq x Nk score matrix.  MFMA 32x32x16 (bf16 / f16), online softmax in fp32.
 *   q   dtype [B, Nq, H, 64]   element strides q_sb (batch), q_sn (token); head stride 64, unit d stride
 *   k,v dtype [B, Nk, H, 64]   strides likewise (q/k/v may be column slices of one fused projection output)
 *   out dtype [B, Nq, H, 64]   strides o_sb, o_sn
 *   head_dim = 64 (SDXL, SD 2.x: every v_path below) or 40 / 80 / 160 (SD 1.x's 8 heads: one generic kernel with the head
 *   dimension zero-padded to a multiple of 32 inside the kernel, v_path ignored); dtype = ED_F16 | ED_BF16; q/k/v 16-byte aligned with strides % 8 == 0, out 8-byte aligned
 *   with strides % 4 == 0.  Nk need not be a multiple of the 64-key tile (cross-attention: 77 text tokens per prompt chunk).
 *   v_path: kernel variant.  0 = V transposed on the fly by ds_read_b64_tr_b16, 1 = V^T tile staged in LDS; +2 = 64
 *   query rows per wave (0..3 give bit-identical results).  4 = software-pipelined kernel (softmax of tile t issued in
 *   the shadow of the MFMAs of tiles t+1 / t-1, deferred O rescale; K / V addressed with 32-bit offsets: returns
 *   hipErrorInvalidValue when (Nk + 128) * max(k_sn, v_sn) * 2 >= 2^31).  5 = 4 without the per-tile row maximum after the
 *   first tile (numerators against the standing reference; exact redo of a tile whose sum exceeds 2^6).  8 = small-KV kernel for Nk <= 160 (cross
 *   attention on the text tokens, 77 per prompt chunk: K / V staged once per 512 query rows, single pass, no online rescale; 2 / 3 / 5
 *   blocks of 32 keys for Nk <= 64 / 96 / 160, Nk > 160 returns hipErrorInvalidValue before any launch).
 *   4, 5 and 8 agree with 0..3 to the rounding of P (same fp32 accumulation, different summation grouping).
 *   6 = 5 for EXPONENT-DOMAIN queries: the caller has multiplied q by scale * log2(e) (the model folds it into the query
 *   projection weights), `scale` is ignored and out = sum_k 2^(q.k) v / sum_k 2^(q.k).  The row reference -m is the initial
 *   value of the S accumulators (the MFMA's C operand), so a numerator is one v_exp_f32 of the accumulator: no FMA, no
 *   per-tile maximum (exact maximum of the first tile, then the lazy check of 5).  Same limits as 4 / 5; Nk >= 64.
 *   7 = 4 with every LDS operand read issued three MFMAs ahead of its use instead of one (a 4-deep register ring).
 *   9 / 10 = 4 / 5 with 8 waves (256 query rows) per workgroup: each K / V tile is staged once for twice the query rows.
 *   K / V tile loads of 4 .. 7, 9, 10 carry their whole byte offset in the per-lane offset: rows past Nk read as zeros by the
 *   buffer range check, which does not cover a scalar offset.  6, 7, 9 and 10 return hipErrorInvalidValue for Nk < 64 (less than one
 *   full key tile); the exponent-domain contract of 6 (q pre-multiplied, `scale` ignored) can only be honoured by the caller -- the
 *   Python wrapper is what checks it.
 */
int ed_flash_attention(const void* q, const void* k, const void* v, void* out, int dtype, int B, int H, int Nq, int Nk,
                       int head_dim, int64_t q_sb, int64_t q_sn, int64_t k_sb, int64_t k_sn, int64_t v_sb, int64_t v_sn,
                       int64_t o_sb, int64_t o_sn, float scale, int v_path, void* stream);

/*
 * ed_flash_attention_ip -- IP-Adapter decoupled cross attention in one launch (an addition, no
 * signature change, so still ABI v13):
 *       out = softmax(q k_t^T scale) v_t + ip_scale * softmax(q k_i^T scale) v_i
 *   k, v dtype [B, Nt + Ni, H, 64]: the Nt text rows first, then the Ni image rows (to_k_ip / to_v_ip projections of the image
 *   tokens); q, out, dtype, strides and alignment as ed_flash_attention.  head_dim = 64 only, 1 <= Nt <= 160, 1 <= Ni <= 32;
 *   anything else returns hipErrorInvalidValue before any launch.  A sibling of the small-KV kernel (v_path 8): text keys in 2 / 3 /
 *   5 blocks of 32 for Nt <= 64 / 96 / 160 and the image keys in one further block, two independent single-pass softmaxes, two
 *   fp32 accumulators, combined as fl(o_t * inv_t) + fl(ip_scale * fl(o_i * inv_i)) and rounded once to dtype.  The text term is
 *   the small-KV kernel's operation for operation: at ip_scale = 0 the output equals ed_flash_attention(v_path 8) on the text rows
 *   alone bit for bit.
 */
int ed_flash_attention_ip(const void* q, const void* k, const void* v, void* out, int dtype, int B, int H, int Nq, int Nt, int Ni,
                          int head_dim, int64_t q_sb, int64_t q_sn, int64_t k_sb, int64_t k_sn, int64_t v_sb, int64_t v_sn,
                          int64_t o_sb, int64_t o_sn, float scale, float ip_scale, void* stream);

/*
 * ed_flash_attention_ipn -- several IP-Adapters in one launch (an addition, still ABI v13):
 *       out = softmax(q k_t^T scale) v_t + sum_{a < A} w[a] * softmax(q k_a^T scale) v_a
 *   k, v dtype [B, Nt + sum ni, H, 64]: the Nt text rows, then adapter 0's ni[0] rows, adapter 1's ni[1] rows, ...; ni is a HOST
 *   array of A ints, w a DEVICE pointer to A fp32 weights read when the kernel runs (a captured graph replays a change of weights).
 *   q, out, dtype, strides and alignment as ed_flash_attention_ip.  head_dim = 64, 1 <= Nt <= 160, 1 <= A <= 4, every ni[a] >= 1,
 *   sum ni <= 32; anything else returns hipErrorInvalidValue before any launch.  ed_flash_attention_ip's staging with the image
 *   block cut into A segments: one maximum and one sum per segment, probabilities normalised and weighted in fp32 before they are
 *   packed (p_j = e_j * fl(w[a] * inv_a)), one accumulator for the whole image term, stored fl(o_t * inv_t) + o_i rounded once.
 *   The text term is the small-KV kernel's operation for operation: with every w[a] = 0 the output equals
 *   ed_flash_attention(v_path 8) on the text rows alone bit for bit.
 */
int ed_flash_attention_ipn(const void* q, const void* k, const void* v, void* out, int dtype, int B, int H, int Nq, int Nt, int A,
                           const int* ni, int head_dim, int64_t q_sb, int64_t q_sn, int64_t k_sb, int64_t k_sn, int64_t v_sb,
                           int64_t v_sn, int64_t o_sb, int64_t o_sn, float scale, const float* w, void* stream);

/*
 * IP-Adapter attention masks (additions, still ABI v13).
 *
 * ed_flash_attention_ipm -- ed_flash_attention_ipn with a factor per query row and adapter on the image term:
 *       out = softmax(q k_t^T scale) v_t + sum_{a < A} (w[a] * m[b, a, i]) * softmax(q k_a^T scale) v_a      (i: the query row)
 *   ed_flash_attention_ipn's argument list, then m, a DEVICE pointer to fp32 read when the kernel runs -- element (b, a, i) at
 *   m + b * m_sb + a * m_sa + i -- and its batch and adapter strides in floats.  m_sb may be 0 (one mask for the whole batch);
 *   m 4-byte aligned, m_sb >= 0, m_sa >= Nq.  Range and every other condition as ed_flash_attention_ipn; anything else, a NULL or
 *   misaligned m or m_sa < Nq returns hipErrorInvalidValue before any launch.  The kernel is ed_flash_attention_ipn's with the
 *   segment coefficient of a row c_a = fl(fl(w[a] * m[b, a, i]) * inv_a); m is read for i < Nq only.  m == 1 gives
 *   ed_flash_attention_ipn's output bit for bit; m == 0, or every w[a] = 0, gives ed_flash_attention(v_path 8) on the text rows.
 *
 * ed_ip_mask_rows -- the masks every row of a fused model batch reads, all four levels, in one launch.  masks f32 [B, A, H, W]
 *   (values in [0, 1] at latent resolution), 1 <= A <= 4; the gather arguments are ed_assemble_rows_n's (idx .. g_off_x for the
 *   K * copies * B global rows, win_y0 .. v_off_x for the V * B view rows) with ONE padded row size PH x PW, both multiples of 8,
 *   for both parts.  m f32 [(K * copies + V) * B, A, S], S = sum_{L < 4} (PH >> L)(PW >> L), rows in the model batch's order,
 *   level L at offset sum_{l < L} (PH >> l)(PW >> l).  Level 0 is what ed_assemble_rows_n writes into its extra channels from
 *   extra = masks with pad_value = 0 and fp32 rows: the picked source pixel's value for a global row, the window's for a view row,
 *   0 on pad strips and outside the picture.  Level L + 1 is the 2 x 2 mean 0.25f * ((l[2y,2x] + l[2y,2x+1]) + (l[2y+1,2x] +
 *   l[2y+1,2x+1])), every operation rounded in fp32 in that association.  hipErrorInvalidValue before any launch: a NULL masks / m
 *   (or gather table of a part that has rows), A outside 1..4, copies outside 2..9, PH or PW not a multiple of 8, a picked frame
 *   or a window that does not fit the row.
 */
int ed_flash_attention_ipm(const void* q, const void* k, const void* v, void* out, int dtype, int B, int H, int Nq, int Nt, int A,
                           const int* ni, int head_dim, int64_t q_sb, int64_t q_sn, int64_t k_sb, int64_t k_sn, int64_t v_sb,
                           int64_t v_sn, int64_t o_sb, int64_t o_sn, float scale, const float* w, const float* m, int64_t m_sb,
                           int64_t m_sa, void* stream);
int ed_ip_mask_rows(const float* masks, int B, int A, int H, int W, const uint8_t* idx, const int32_t* src_row,
                    const int32_t* src_col, int K, int h, int w, int g_off_y, int g_off_x, const int32_t* win_y0,
                    const int32_t* win_x0, int V, int Sh, int Sw, int v_off_y, int v_off_x, int PH, int PW, int copies, float* m,
                    void* stream);

/*
 * ed_groupnorm_f32 -- GroupNorm (+SiLU) of an fp32 NCHW activation: the VAE's normalisation layers (AutoencoderKL inside
 * ED:270 decode / ED:350 encode; fp32 like the reference keeps it, ED:328).  HW % 4 == 0.  Two launches: partial sums over
 * 64 K-element chunks of every (sample, group), then an apply pass whose blocks combine their group's partials in double.
 *   x, out f32 [N, C, HW]; gamma, beta f32 [C]; workspace: ed_groupnorm_f32_workspace(N, C, HW, G) bytes
 */
int64_t ed_groupnorm_f32_workspace(int N, int C, int HW, int G);
int ed_groupnorm_f32(const void* x, const void* gamma, const void* beta, void* out, float* workspace, int N, int C, int HW,
                     int G, float eps, int act_silu, void* stream);

/*
 * ed_softmax_rows -- x[r, :] = softmax(scale * x[r, :]) in place, fp32, rows x cols contiguous (cols % 4 == 0).  The VAE
 * mid-block attention (AutoencoderKL inside ED:270 decode / ED:350 encode; one 512-wide head, fp32) runs as
 * Q K^T (library fp32 GEMM) -> ed_softmax_rows -> S V (library fp32 GEMM) instead of the AOTriton SDPA kernel.
 */
int ed_softmax_rows(void* x, int64_t rows, int64_t cols, float scale, void* stream);

/*
 * ---- dense contractions inside the UNet (csrc/gemm_kernels.hip): one 256 x 256 x 64, 8-wave, 8-phase MFMA main loop
 * (LDS-DMA staging with counted vmcnt, st_16x32-swizzled LDS image) behind three entry points.  16-bit I/O, fp32
 * accumulation, ONE rounding of the epilogue's fp32 result.  All pointers 16-byte aligned; byte sizes of x and w below
 * 2^31 (32-bit buffer offsets); hipErrorInvalidValue for a shape outside these limits (the caller keeps the library call).
 *
 * ed_geglu_gemm -- diffusers GEGLU.forward (`h, gate = proj(x).chunk(2, -1); h * gelu(gate)`) in one kernel:
 *   out[m, n] = (x[m,:] . w[n,:] + bias[n]) * gelu(x[m,:] . w[I+n,:] + bias[I+n])
 *   x [M, K], w [2I, K] (torch Linear weight), bias [2I] or NULL, out [M, I]; K % 64 == 0, I % 128 == 0.
 *   gelu = x Phi(x) with erfc by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7), evaluated on the fp32 accumulator: the
 *   projection output is never rounded to 16 bits and never touches HBM.
 */
int ed_geglu_gemm(const void* x, const void* w, const void* bias, void* out, int dtype, int64_t M, int K, int I, void* stream);

/*
 * ed_linear -- torch.nn.functional.linear with an optional fused residual: out = x w^T + bias (+ residual)
 *   x [M, K], w [N, K], bias [N] or NULL, residual [M, N] or NULL, out [M, N]; K % 64 == 0, N % 8 == 0.
 */
int ed_linear(const void* x, const void* w, const void* bias, const void* residual, void* out, int dtype, int64_t M, int K, int N,
              void* stream);

/*
 * ed_conv3x3_nhwc -- Conv2d(Cin, N, 3, stride 1, padding 1) on a channels-last image as an implicit GEMM (K = 9 Cin; the A
 * operand row of output pixel m at tap (dy, dx) is the Cin vector of pixel m + dy W + dx, zeros outside the image), with
 * ResnetBlock2D's adds in the epilogue:
 *   out[b,y,x,n] = sum_{dy,dx,c} x[b,y+dy,x+dx,c] w[n,dy,dx,c] + bias[n] + sample_bias[b,n] + residual[b,y,x,n]
 *   x [B,H,W,Cin], w [N,3,3,Cin] (a torch Conv2d weight in channels_last memory format), bias [N] / sample_bias [B,N] /
 *   residual [B,H,W,N] or NULL, out [B,H,W,N]; Cin % 64 == 0, N % 8 == 0.
 */
int ed_conv3x3_nhwc(const void* x, const void* w, const void* bias, const void* sample_bias, const void* residual, void* out,
                    int dtype, int B, int H, int W, int Cin, int N, void* stream);

/*
 * ed_conv3x3_nhwc_up2x -- Upsample2D (diffusers: F.interpolate(x, scale_factor = 2, mode = "nearest") + conv 3x3, behind ED:393-432) as ONE
 * launch: ed_conv3x3_nhwc whose A operand is the 2x nearest-neighbour upsampling of x, never written -- output pixel (y, x) at tap
 * (dy, dx) reads source pixel ((y + dy) >> 1, (x + dx) >> 1).  x dtype [B, H/2, W/2, Cin] channels-last, H and W = the OUTPUT size (even),
 * w / bias / out as in ed_conv3x3_nhwc; no sample bias, no residual.  Same products in the same order as ed_conv3x3_nhwc on the
 * materialised upsampling: bit-identical to it.
 */
int ed_conv3x3_nhwc_up2x(const void* x, const void* w, const void* bias, void* out, int dtype, int B, int H, int W, int Cin, int N,
                         void* stream);

/*
 * ed_conv3x3_nhwc_s2 -- Downsample2D of the UNet (diffusers: conv 3x3, stride 2, padding 1, behind ED:393-432) on the same main loop: output
 * pixel (y, x) at tap (dy, dx) reads input pixel (2 y + dy, 2 x + dx), zeros outside.  x dtype [B, 2H, 2W, Cin] channels-last, H and W =
 * the OUTPUT size, w [N, 3, 3, Cin] / bias [N] / out [B, H, W, N] as in ed_conv3x3_nhwc; no sample bias, no residual.
 */
int ed_conv3x3_nhwc_s2(const void* x, const void* w, const void* bias, void* out, int dtype, int B, int H, int W, int Cin, int N,
                       void* stream);

/*
 * ---- the fp32 VAE's ResnetBlock convolutions on split 16-bit operands (csrc/vae_kernels.hip + the fp32-output epilogue of the
 * GEMM main loop; round 5).  The reference runs the VAE in fp32 (elastic_diffusion.py:267-310 decode, :327-364 pad-strip encodes,
 * kept out of autocast at :328); these entry points keep fp32 accuracy (~3e-7 relative per convolution) on the 16-bit MFMA pipe:
 * an fp32 value v is carried as hi = fp16(v), lo = fp16(v - hi), and  x.w = xh.wh + xl.wh + xh.wl  is ONE 16-bit convolution over
 * 3 Cin channels, x'' = [xh | xl | xh] per pixel against w'' = [wh | wh | wl] per tap, accumulated in fp32 by the MFMA.
 *
 * ed_groupnorm_nhwc_f32 -- GroupNorm [+ SiLU] of an fp32 channels-last activation x [N, HW, C] (statistics in fp32 partial sums
 *   combined in double, fixed order):  split16 = 0: out fp32 [N, HW, C];  split16 = 1: out fp16 [N, HW, 3 C] = [hi | lo | hi], the
 *   A operand of ed_conv3x3_nhwc_f32out (after GroupNorm + SiLU the values are bounded by the affine parameters: fp16's range is
 *   safe; hi and lo nevertheless SATURATE at +-65504 -- a value beyond the range gives a finite, clamped operand, never inf - inf).  (C / G) % 4 == 0, G <= 256; workspace: ed_groupnorm_nhwc_f32_workspace bytes; pointers 16-byte aligned.
 * ed_conv3x3_nhwc_f32out -- ed_conv3x3_nhwc's main loop with an fp32 epilogue:
 *   out[b,y,x,n] = out_scale * sum_{dy,dx,c} x[b,y+dy,x+dx,c] w[n,dy,dx,c] + bias[n] + residual[b,y,x,n]      (no 16-bit rounding)
 *   x fp16 [B,H,W,Cin'] and w fp16 [N,3,3,Cin'] (Cin' = 3 Cin for split operands; any Cin' % 64 == 0 works), bias fp32 [N] or NULL,
 *   residual fp32 [B,H,W,N] or NULL, out fp32 [B,H,W,N]; dtype must be ED_F16; out_scale: a power of two that undoes the
 *   pre-scaling of the split weights (which keeps wl out of fp16's subnormal range); act_absmax: NULL, or the device float that
 *   ed_split_f32_nhwc scaled the activation by (the result is multiplied by 2^e, see there).  N % 8 == 0, 32-bit operand offsets as above.
 * ed_split_f32_nhwc -- the same (hi, lo) split for a RAW fp32 channels-last activation x [N, H, W, C] (the VAE decoder's upsampler
 *   convolutions, whose input is the un-normalised stream): out fp16 [N, U H, U W, 3 C] = [hi | lo | hi], U = 2 with upsample2x (nearest-
 *   neighbour upsampling folded into the write), else 1.  The raw stream is NOT bounded (the real SDXL decoder stream leaves fp16's
 *   range -- it is why that VAE produces NaNs in fp16), so the split is made exact over the whole fp32 range by a per-tensor power of
 *   two (round 6):  absmax -> e = max(0, exponent(absmax) - 14);  the kernel splits 2^-e v (|2^-e v| < 2^15: hi never
 *   saturates) and ed_conv3x3_nhwc_f32out multiplies its result by 2^e (its `act_absmax` argument: the SAME device float).  Scaling
 *   by a power of two is exact, so hi + lo = v to 2^-22 |v| as in the bounded case.  absmax = NULL: no scaling; hi AND lo then saturate
 *   at +-65504 (finite, never inf - inf; exact up to |v| = 65504, 11 bits up to 1.3e5).  C % 4 == 0; pointers 16-byte aligned.
 * ed_absmax_f32 -- out[0] = max |x[i]| over n fp32 values (bit pattern maximum: a NaN input yields a NaN, an Inf an Inf), the
 *   per-tensor figure above.  One device float, written by this call in stream order (memset + atomic max of the non-negative bit
 *   patterns: order-independent, bit-reproducible).
 */
int ed_absmax_f32(const void* x, int64_t n, float* out, void* stream);
int ed_split_f32_nhwc(const void* x, void* out, int N, int C, int H, int W, int upsample2x, const float* absmax, void* stream);
int64_t ed_groupnorm_nhwc_f32_workspace(int N, int C, int HW, int G);
int ed_groupnorm_nhwc_f32(const void* x, const void* gamma, const void* beta, void* out, float* workspace, int N, int C, int HW, int G,
                          float eps, int act_silu, int split16, void* stream);
int ed_conv3x3_nhwc_f32out(const void* x, const void* w, const float* bias, const float* residual, float* out, int dtype, int B, int H, int W,
                           int Cin, int N, float out_scale, const float* act_absmax, void* stream);

/*
 * ed_conv3x3_nhwc_f32out_s2 -- the VAE encoder's Downsample2D (diffusers: F.pad(x, (0, 1, 0, 1)) + conv 3x3, stride 2, padding 0; AutoencoderKL
 * behind ED:327-364) on the split-operand main loop at fp32 accuracy: output pixel (y, x) at tap (ty, tx) in 0..2 reads input pixel
 * (2 y + ty, 2 x + tx), zeros past the bottom / right edge.  x fp16 [B, 2H, 2W, Cin'] = the split operand of the raw fp32 stream
 * (ed_split_f32_nhwc; Cin' = 3 Cin), H and W = the OUTPUT size, w / bias / out / out_scale / act_absmax as in ed_conv3x3_nhwc_f32out; no residual.
 */
int ed_conv3x3_nhwc_f32out_s2(const void* x, const void* w, const float* bias, float* out, int dtype, int B, int H, int W, int Cin, int N,
                              float out_scale, const float* act_absmax, void* stream);

/*
 * ---- Canny condition extraction (csrc/canny_kernels.hip): EDC:1102-1110, cv2.Canny(img, 100, 200) of the ControlNet variant's
 * process_condition_image.  The algorithm is OpenCV 4.x cv::Canny(apertureSize = 3, L2gradient = false) for 8-bit input (DESIGN.md
 * "Canny condition extraction"); all arithmetic is integer, the result is exact.  C in {1, 3}, 1 <= H, W <= 8192, anything else is
 * hipErrorInvalidValue without a launch.  Three stages, separate so that each can be tested alone:
 *
 * ed_canny_map -- img uint8 [H, W, C] -> map uint8 [H, W]: Sobel 3x3 (replicated border), |dx| + |dy|, the channel of the largest
 *   magnitude (lowest index on ties), non-maximum suppression, thresholds low / high (already floored; swapped when low > high).
 *   Map codes as in OpenCV: 1 = not an edge, 0 = candidate (low < m <= high), 2 = strong (m > high).
 * ed_canny_hysteresis -- in place: every candidate that is 8-connected through candidates to a strong pixel becomes 2.  One launch
 *   floods each 64 x 32 tile inside LDS; the host relaunches until a pass promotes nothing and reports the number of passes in
 *   *passes_out (a HOST int32).  THIS ENTRY POINT SYNCHRONISES THE STREAM once per pass to read the "changed" word: it is pre-processing
 *   of one image before the loop starts and must not be called while the stream is being captured into a graph.  workspace:
 *   ed_canny_workspace bytes of device memory.  More than H W + 1 passes (impossible for a monotone flood: every pass but the last
 *   promotes a pixel) returns hipErrorUnknown rather than a truncated result.
 * ed_canny_edges -- map -> edges uint8 [H, W, 3] (255 where map == 2, else 0) and / or cond fp32 [1, 3, H, W] (1.0 / 0.0: what the
 *   pipeline makes of that image); either may be NULL, not both.
 */
int64_t ed_canny_workspace(int H, int W, int C);
int ed_canny_map(const uint8_t* img, int H, int W, int C, int low, int high, uint8_t* map, void* stream);
int ed_canny_hysteresis(uint8_t* map, int H, int W, void* workspace, int32_t* passes_out, void* stream);
int ed_canny_edges(const uint8_t* map, int H, int W, uint8_t* edges, float* cond, void* stream);

/*
 * ---- Pillow-exact resize of 8-bit images (csrc/resize_kernels.hip): Image.resize with the BICUBIC (EDC:1392, PIL's default) or
 * LANCZOS (EDC:173-175, 1017) filter on an L / RGB image, one axis per entry point.  The caller computes Pillow's fixed-point
 * tables on the host (elasticdiffusion_official_amd/resample.py; DESIGN.md "Pillow-exact resize"): coeff int32 [n_out, ksize] with
 * 22 fraction bits, zero-padded, and bounds int32 [n_out, 2] = (first source index, taps) per output index.  Each output byte is
 * clamp((2^21 + sum_{x < taps} in[first + x] * coeff[x]) >> 22, 0, 255) in int32: exact, independent of the order of summation.
 * C in {1, 3} interleaved channels, every input and output extent in 1..8192; anything else is hipErrorInvalidValue without a launch.
 * Table entries are clamped to the source extent and to ksize before use.  A two-dimensional resize is ed_resize_rows_u8 over the
 * source rows the vertical tables read, into a uint8 intermediate, then ed_resize_cols_u8 with the bounds shifted to that window.
 *
 * ed_resize_rows_u8 -- horizontal: src [H, W, C] with rows src_pitch bytes apart (any alignment) -> dst [H, W_out, C] with rows
 *   dst_pitch bytes apart.  dst and dst_pitch must be multiples of 4 and dst_pitch >= W_out C rounded up to 4: the kernel stores
 *   whole dwords and writes 0 into the bytes between W_out C and that bound.
 * ed_resize_cols_u8 -- vertical: src [H, W, C] seen as H rows of WC_bytes = W C bytes, src_pitch bytes apart (any alignment) ->
 *   dst_u8 uint8 [H_out, W, C] contiguous and / or dst_cond fp32 [1, 3, H_out, W] = byte / 255 (correctly rounded division, what
 *   torch's .div(255.0) gives; C = 1 is replicated to the three planes); either may be NULL, not both.
 */
int ed_resize_rows_u8(const uint8_t* src, int H, int W, int C, int src_pitch, const int32_t* coeff, const int32_t* bounds, int ksize,
                      int W_out, uint8_t* dst, int dst_pitch, void* stream);
int ed_resize_cols_u8(const uint8_t* src, int H, int WC_bytes, int src_pitch, const int32_t* coeff, const int32_t* bounds, int ksize,
                      int H_out, int C, uint8_t* dst_u8, float* dst_cond, void* stream);

/*
 * ---- image-to-image and masked inpainting (additions, no signature change, so still ABI v13).  The
 * reference has neither; the semantics are those of diffusers' StableDiffusionImg2ImgPipeline and of the 4-channel-UNet branch
 * of StableDiffusionInpaintPipeline.  Streaming kernels: 4 elements per thread with 16-byte accesses when the extents are
 * multiples of 4 and the pointers aligned, one element per thread otherwise, the same bits either way.  fp32 arithmetic rounded
 * per operation, in the torch-CPU order given.
 *
 * ed_u8_to_vae_input -- VaeImageProcessor.preprocess after the resize: img uint8 [H, W, 3] (interleaved RGB) ->
 *   out [1, 3, H, W] (planar) of `dtype` = 2 * (float(v) / 255) - 1.
 * ed_img2img_init -- latent_dist.sample() * scaling_factor, then scheduler.add_noise at the first executed timestep:
 *   z0 = (mean + std * eps) * sf;  x = a * z0 + b * noise.   mean / std of `dtype` (ED_F32 / ED_F16 / ED_BF16, converted to fp32
 *   exactly), eps / noise / z0 / x f32, n elements each.  std, not logvar: exp on the device is not torch-CPU's exp.
 * ed_mask_to_latent -- torch's nearest interpolate of the binarised mask: mask[y, x] = src[scale * y, scale * x] >= threshold
 *   (1 = repaint, 0 = keep), src uint8 [H, W] with H = Hl * scale and W = Wl * scale (anything else is hipErrorInvalidValue),
 *   mask uint8 [Hl, Wl].  threshold = 128 for an 8-bit picture (v / 255 >= 0.5), 1 for a mask that is already 0 / non-zero.
 * ed_inpaint_blend -- out = mask ? x : known over `planes` = B * C planes of HW elements (the mask broadcast over them), with
 *   known = a * z0 + b * noise, or z0 itself when `clean` != 0 (after the last timestep; noise may then be NULL).  A select: the
 *   side not taken is never combined arithmetically.  out may be x (in place).
 */
int ed_u8_to_vae_input(const uint8_t* img, int H, int W, void* out, int dtype, void* stream);
/* ed_u8_to_clip_input -- CLIPImageProcessor after its resize: centre crop, rescale, normalise in one launch.
 *   img uint8 [H, W, 3] (interleaved RGB), crop origin (y0, x0) with y0 + S <= H and x0 + S <= W (else hipErrorInvalidValue),
 *   out f32 [3, S, S] (planar) = (float(double(v) * (1 / 255)) - mean_c) / std_c, the subtraction and the division in fp32. */
int ed_u8_to_clip_input(const uint8_t* img, int H, int W, int y0, int x0, int S, float* out, float mean0, float mean1, float mean2,
                        float std0, float std1, float std2, void* stream);
int ed_img2img_init(const void* mean, const void* std, int dtype, const float* eps, const float* noise, float sf, float a,
                    float b, float* z0, float* x, int64_t n, void* stream);
int ed_mask_to_latent(const uint8_t* src, int H, int W, int scale, int threshold, uint8_t* mask, int Hl, int Wl, void* stream);
int ed_inpaint_blend(const float* x, const uint8_t* mask, const float* z0, const float* noise, float a, float b, int clean,
                     float* out, int planes, int64_t HW, void* stream);

/*
 * ed_u8_to_vae_input_masked (an addition, still ABI v13) -- the picture with the hole blanked, what a
 * 9-channel inpainting UNet's masked-image latent is encoded from: ed_u8_to_vae_input where mask[y, x] < threshold, exactly +0.0
 * where mask[y, x] >= threshold (a select).  img uint8 [H, W, 3], mask uint8 [H, W], threshold in 1..255 (128 = diffusers'
 * mask < 0.5 on the byte / 255), out [1, 3, H, W] of `dtype`.  4 pixels per thread when H * W % 4 == 0 and the pointers allow it
 * (img and mask on 4 bytes, out on 16), one element per thread otherwise, the same bits either way.
 */
int ed_u8_to_vae_input_masked(const uint8_t* img, const uint8_t* mask, int threshold, int H, int W, void* out, int dtype,
                              void* stream);

/*
 * ---- soft-edged inpainting (additions, no signature change, so still ABI v13): the mask blurred with
 * Pillow's bytes, graded masks, Image.composite fused with the float -> 8-bit conversion, the outpainting canvas.  Integer or
 * select arithmetic, exact; uint8 images are dense (pitch = width * channels), sides 1..8192.
 *
 * ed_box_blur3_rows_u8 / ed_box_blur3_cols_u8 -- PIL.ImageFilter.GaussianBlur(radius) on an L image is the rows launch followed by
 *   the columns launch (src != dst in both).  Each launch performs the THREE box passes of its direction, every pass on the
 *   previous pass's bytes, with the line (rows) or a strip of ed_box_blur3_cols_strip(H, W) columns (columns) staged in LDS.  One
 *   pass over a line of n bytes, c(i) = clamp(i, 0, n - 1):
 *       out[x] = (ww * sum_{d = -r..r} in[c(x + d)] + fw * (in[c(x - r - 1)] + in[c(x + r + 1)]) + 2^23) >> 24      (uint32)
 *   The caller computes (r, ww, fw) from the radius as Pillow does: sigma2 = radius^2 / 3, Lw = sqrt(12 sigma2 + 1),
 *   l = floor((Lw - 1) / 2), a = (2l + 1)(l(l + 1) - 3 sigma2) / (6 (sigma2 - (l + 1)^2)), fr = float32(l + a), r = int(fr),
 *   ww = uint32(float32(2^24) / (2 fr + 1)) in float32, fw = (2^24 - (2r + 1) ww) / 2.  Weights with (2r + 1) ww + 2 fw > 2^24 (the
 *   result would not be a byte) are hipErrorInvalidValue.
 * ed_box_blur3_cols_strip -- no launch: the strip width in columns (a power of two in 4..32) the columns launch uses for an
 *   H x W image; 0 for sides outside 1..8192.
 * ed_mask_levels_to_latent -- ed_mask_to_latent's gather without the comparison: level[y, x] = src[scale * y, scale * x].
 * ed_inpaint_blend_level -- ed_inpaint_blend with (level[p] <= thr) in place of (mask[p] == 0): out = level > thr ? x : known.
 *   thr in 0..255; the caller's rule for target timestep index j of T is thr = (255 * (T - j)) / T (integer division).
 * ed_composite_u8 -- u = (uint8)(decoded * 255) (fp32 product, truncated; decoded f32 [1, 3, H, W] in [0, 1]), then
 *   PIL.Image.composite(u, init, mask) per channel: t = u * m + init * (255 - m) + 128; out = (t + (t >> 8)) >> 8.
 *   init / out uint8 [H, W, 3] (interleaved), mask uint8 [H, W].  4 pixels per thread when W % 4 == 0 and the pointers allow it.
 * ed_canvas_pad_u8 -- np.pad(img, mode="edge"): canvas uint8 [H + top + bottom, W + left + right, 3] and mask uint8 of the same
 *   extent, 255 on the new border and 0 over the original; the padded sides must stay within 8192.
 */
int ed_box_blur3_rows_u8(const uint8_t* src, int H, int W, int r, int ww, int fw, uint8_t* dst, void* stream);
int ed_box_blur3_cols_u8(const uint8_t* src, int H, int W, int r, int ww, int fw, uint8_t* dst, void* stream);
int ed_box_blur3_cols_strip(int H, int W);
int ed_mask_levels_to_latent(const uint8_t* src, int H, int W, int scale, uint8_t* level, int Hl, int Wl, void* stream);
int ed_inpaint_blend_level(const float* x, const uint8_t* level, int thr, const float* z0, const float* noise, float a, float b,
                           int clean, float* out, int planes, int64_t HW, void* stream);
int ed_composite_u8(const float* decoded, const uint8_t* init, const uint8_t* mask, uint8_t* out, int H, int W, void* stream);
int ed_canvas_pad_u8(const uint8_t* img, int H, int W, int left, int top, int right, int bottom, uint8_t* canvas, uint8_t* mask,
                     void* stream);

/*
 * ---- LoRA adapters merged into the weights (an addition, still ABI v13).
 *
 * ed_lora_merge -- ONE launch writes every touched weight of a model from its pristine copy and its active adapters.  A weight is a
 *   dense row-major [N, K] matrix in its physical memory order (N = output features / channels, K = input features, or kh * kw * Cin
 *   in the memory order of a convolution weight: channels-last [N, kh, kw, Cin] for the 16-bit UNet).  Adapters j of the tensor in
 *   table order:
 *       W[n, k] = rn_dtype( f32(base[n, k]) + s ),    s = sum_j c_j * ( sum_q up_j[n, q] * down_j[q, k] )
 *   inner and outer sum are fp32 fmaf chains from +0 (q ascending, then j ascending), then one fp32 add and ONE rounding to the
 *   weight's type.  An element's bits depend on its own tensor's records only, not on the rest of the table.  A tensor whose adapter
 *   range is empty is a plain copy of its base.
 *
 *   The table is one array of int64 words; the caller keeps it twice with identical contents: `table_host` in HOST memory (the one
 *   pointer of this ABI that is not a device pointer; every word of it is checked before anything is launched) and `table_dev` in
 *   device memory (what the kernel reads; 8-byte aligned).  The pointers INSIDE the table are device pointers.
 *     words [8 t, 8 t + 8), t in [0, n_tensors)                   -- tensor record:
 *       0 base   const void*, dtype elements, N * K of them        4 dtype  ED_F32 / ED_F16 / ED_BF16 (base and dst alike)
 *       1 dst    void*, the weight's own storage; != base          5 a0     first adapter record of this tensor
 *       2 N      >= 1                                              6 a1     one past its last; a0 == a1: copy base -> dst
 *       3 K      >= 1, N * K < 2^31                                7 tile0  sum of the tile counts of the tensors before it
 *     words [8 n_tensors + 4 a, 8 n_tensors + 4 a + 4), a in [0, n_adapters)   -- adapter record:
 *       0 up     const float* [N, r]      1 down   const float* [r, K] (K in the weight's physical order)
 *       2 r      1 .. 65536               3 c      the bits of the fp32 coefficient in the low 32 bits (finite), high bits 0
 *   A tensor has ceil(N / 64) * ceil(K / 128) tiles (ED_LORA_TILE_N x ED_LORA_TILE_K); n_tiles is their sum over the table (the
 *   grid).  The adapter ranges of consecutive tensors are consecutive (tensor 0 starts at 0, the last ends at n_adapters).  A null
 *   or misaligned pointer, a dtype code, an extent, a range, a tile0 or an n_tiles that breaks these rules is hipErrorInvalidValue
 *   and nothing is launched.
 */
enum { ED_LORA_TENSOR_WORDS = 8, ED_LORA_ADAPTER_WORDS = 4, ED_LORA_TILE_N = 64, ED_LORA_TILE_K = 128 };
int ed_lora_merge(const int64_t* table_host, const int64_t* table_dev, int n_tensors, int n_adapters, int64_t n_tiles,
                  void* stream);

/*
 * ---- score PCA maps (additions, still ABI v13): pca_diffusion_scores.py:165-179 on the device.  A score is
 * f32 [B, C = 4, H, W], dense, n = H * W pixels per sample; sample b's pixels are the rows of X_b [n, 4].
 *
 * ed_score_pca_workspace -- no launch: bytes of the workspace both calls below take for B samples of n pixels (0 outside their
 *   bounds).  8-byte aligned; ed_score_pca_map reads what ed_score_pca_fit left in it.
 * ed_score_pca_fit -- per sample: mean and covariance (divided by n - 1) of X_b from fp64 sums shifted by the sample's first pixel,
 *   merged in a fixed order (a fixed number of blocks per sample write partials into the workspace, one wave per sample merges them);
 *   the covariance diagonalised by cyclic Jacobi in fp64; the three largest eigenpairs in descending order, every component turned
 *   so that its entry of largest magnitude is positive (sklearn's svd_flip(u_based_decision=False)).
 *     components f32 [B, 3, 4], mean f32 [B, 4], explained_variance f32 [B, 3], norm f32 [B, 2] = (min, max) of the WHOLE tensor.
 *   normalize != 0: the fit is that of s' = (s - min) / (max - min) * 2 - 1, the reference's normalisation of the class direction,
 *   formed per element with its four fp32 operations (one more launch finds min and max first).  A constant tensor (max == min,
 *   where the reference divides by zero) is left un-normalised.
 * ed_score_pca_map -- out uint8 [B, H, W, 3]: r_j = fp32(sum_c (x_c - mean_c) components[b][j][c]), the sum in fp64 (differences
 *   first, then products and sums left to right) from the fit's fp64 mean and components, which it left in the workspace;
 *   lo / hi = the minimum / maximum of r over the sample's pixels and three components, out = (uint8)((r - lo) / (hi - lo) * 255)
 *   in fp32, truncated; 0 where hi == lo.  norm: the buffer ed_score_pca_fit wrote when it normalised (x is then s' as above),
 *   NULL when it did not.
 *
 * C != 4, H * W < 4, H * W > 2^28, B < 1, a null or misaligned buffer (4 bytes; the workspace 8) or two buffers that overlap are
 * hipErrorInvalidValue and nothing is launched.  Two launches each (three for a normalising fit); no host sync, no atomics: equal
 * inputs give equal bits.
 */
int64_t ed_score_pca_workspace(int B, int64_t n);
int ed_score_pca_fit(const float* score, int B, int C, int H, int W, int normalize, float* components, float* mean,
                     float* explained_variance, float* norm, void* workspace, void* stream);
int ed_score_pca_map(const float* score, int B, int C, int H, int W, const float* norm, uint8_t* out, void* workspace,
                     void* stream);

/*
 * ---- weighted statistics for the narrowed constant-image VAE encode (additions, no signature change, so
 * still ABI v13).  The encode of a constant-colour image varies only in a border; the encoder is run on an image with fewer rows /
 * columns in which ONE row / column per level stands for a run of identical ones.  What is global in the encoder -- the GroupNorm
 * statistics and the mid-block attention's softmax -- must count that row / column with its multiplicity:
 *
 * ed_groupnorm_nhwc_f32_weighted / ed_groupnorm_f32_weighted -- ed_groupnorm_nhwc_f32 / ed_groupnorm_f32 on an [N, C, H, W] activation
 *   (HW = H * W) whose pixel (y, x) counts wy[y] * wx[x] times in the mean and the variance: both shifted sums carry the weight and
 *   the element count is (C / G) sum(wy) sum(wx).  wx f32 [W] or NULL, wy f32 [H] or NULL (NULL = all ones), 4-byte aligned.  The
 *   apply pass and every other argument are the unweighted entry point's; the workspace is THREE TIMES its ed_*_workspace bytes,
 *   16-byte aligned: every pixel is summed once by the unweighted code and the excess (w - 1) of the heavy pixels in double, in
 *   double partials behind the fp32 ones (a few heavy terms can dominate a sum; their rounding would not average out).  All-ones
 *   weights give the unweighted entry point's bits, and wx = wy = NULL is that entry point.
 * ed_softmax_rows_bias -- x[r, :] = softmax(scale * x[r, :] + bias) in place: ed_softmax_rows with one fp32 bias per column
 *   (16-byte aligned), the log multiplicity of the key.  bias = NULL is ed_softmax_rows; a zero bias gives the same bits.
 */
int ed_groupnorm_nhwc_f32_weighted(const void* x, const void* gamma, const void* beta, void* out, float* workspace, int N, int C, int H,
                                   int W, int G, float eps, int act_silu, int split16, const float* wx, const float* wy, void* stream);
int ed_groupnorm_f32_weighted(const void* x, const void* gamma, const void* beta, void* out, float* workspace, int N, int C, int H,
                              int W, int G, float eps, int act_silu, const float* wx, const float* wy, void* stream);
int ed_softmax_rows_bias(void* x, int64_t rows, int64_t cols, float scale, const float* bias, void* stream);

/*
 * ---- Multi-ControlNet hand-off (an addition, still ABI v13).
 *
 * ed_control_residuals -- ONE launch adds the weighted residuals of up to ED_CONTROL_MAX_NETS ControlNets to every skip tensor of a
 *   UNet forward and to its mid-block output.  A level is a dense tensor of B batch rows of `count` elements each, in whatever
 *   memory order its tensors share (NCHW-contiguous or channels-last: the batch row is outermost in both).  For batch row b and
 *   element i of a level, with w f32 [B, n_nets] in device memory:
 *       acc = skip ? f32(skip[b, i]) : +0.0f
 *       for n = 0 .. n_nets - 1, if w[b, n] != 0:   acc = fadd_rn(acc, fmul_rn(w[b, n], f32(r_n[b, i])))
 *       out[b, i] = rn_dtype(acc)
 *   -- a product and a sum each rounded to fp32 (no contraction), one rounding to the type of `out`: the torch fp32 sequence
 *   `acc = acc + w * r`, bit for bit.  A zero weight leaves its term out and its residual UNREAD: a non-finite value in a closed
 *   net does not reach the output.  All-zero weights copy the skip (or write +0).
 *
 *   The table is one array of int64 words in HOST memory, laid out in the manner of ed_lora_merge's; every word of it is checked
 *   before anything is launched.  It has no device copy: the checked table travels BY VALUE in the kernel's arguments (at most
 *   ED_CONTROL_MAX_LEVELS records, 3 KiB), so a launch captured into a hipGraph carries its table in the graph node and no
 *   host-to-device copy has to be captured for tensors whose addresses exist only during the capture.  The pointers INSIDE the
 *   table, and `w`, are device pointers.
 *     words [12 l, 12 l + 12), l in [0, n_levels)                  -- level record:
 *       0 skip    const void* or 0 (no skip: out = the weighted sum)   4 dtype   ED_F32 / ED_F16 / ED_BF16 of skip and out
 *       1 out     void*; == skip (in place) or disjoint from it        5 rdtype  the residuals' type: == dtype, or 16-bit under an
 *       2 count   elements per batch row, >= 1                                   ED_F32 dtype (fp32 residual stream); == dtype if skip == 0
 *       3 B       batch rows, >= 1, the same in every level            6 tile0   sum of the tile counts of the levels before it
 *       7 0 (reserved)         8 .. 11  r_n const void*, n < n_nets; 0 for n >= n_nets; none may overlap out
 *   A level has B * ceil(count / ED_CONTROL_TILE) tiles; n_tiles is their sum over the table (the grid).  Accesses are 16 bytes
 *   wide where count % 8 == 0 and every pointer of the level is 16-byte aligned, one element wide otherwise -- the same bits either
 *   way.  A null or misaligned pointer, a dtype code or pair, a count, n_nets outside 1 .. ED_CONTROL_MAX_NETS, n_levels outside
 *   1 .. ED_CONTROL_MAX_LEVELS, an overlap, a tile0 or an n_tiles that breaks these rules is hipErrorInvalidValue and nothing is launched.
 */
enum { ED_CONTROL_MAX_NETS = 4, ED_CONTROL_LEVEL_WORDS = 12, ED_CONTROL_TILE = 4096, ED_CONTROL_MAX_LEVELS = 32 };
int ed_control_residuals(const int64_t* table_host, int n_levels, int n_nets, const float* w, int64_t n_tiles, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ELASTIC_HIP_H */
