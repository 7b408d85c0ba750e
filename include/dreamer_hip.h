/*
 * dreamer_hip.h — C-ABI of libdreamer_hip.so (MI355X / gfx950, HIP, fp32).
 *
 * This is the drop-in boundary of the DreamerV2 gradient-step hot path.  pydreamer itself has no FFI:
 * everything below is what a `torch.autograd.Function` in a pydreamer-style `Dreamer.training_step`
 * binds instead of the ATen ops the reference dispatches from its nn.Modules (file:line citations are
 * into /root/reference).  See INTEGRATION.md for the ctypes stub a maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous fp32 (unless typed otherwise), owned by the caller
 *    (torch tensors); the library never allocates or frees device memory and never synchronises;
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *  - every function returns 0 on success or a negative DM_E_* code; dm_last_error() gives the
 *    thread-local message; nothing throws across the ABI;
 *  - tensors are time-major: row index n = t*B + b for (T,B,...) tensors (reference layout,
 *    pydreamer/data.py:188, rssm.py:21-78); matrices are row-major with explicit leading dimension
 *    where a `ld*` argument is given;
 *  - workspaces: `ws` is scratch (size from dm_workspace_bytes), `acts` holds activations saved by a
 *    *_fwd call for the matching *_bwd call (size from dm_<op>_acts_floats); both are caller-allocated.
 */
#ifndef DREAMER_HIP_H
#define DREAMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM_OK 0
#define DM_E_SHAPE (-1)       /* bad / unsupported shape or config */
#define DM_E_WORKSPACE (-2)   /* workspace or acts buffer too small */
#define DM_E_HIP (-3)         /* HIP runtime error (captured with hipGetLastError) */
#define DM_E_DEVICE (-4)      /* not a gfx950 device */
#define DM_E_NULL (-5)        /* required pointer is null */

#define DM_MAX_MLP_LAYERS 8

/* model / batch geometry: the config/defaults.yaml keys the hot path reads (dreamer.py:23-58,237-277) */
typedef struct dm_shape {
  int32_t T, B, I;          /* batch_length, batch_size, iwae_samples (conv decoder: N = T*B*I frames; RSSM calls take B*I as B, I = 1) */
  int32_t H;                /* imag_horizon */
  int32_t D, Hd;            /* deter_dim, hidden_dim */
  int32_t S, C;             /* stoch_dim, stoch_discrete (Z = S*C) */
  int32_t E;                /* embed dim: the RSSM takes any E >= 1.  32*cnn_depth for the convolution encoder (encoders.py:76), + 256
                               with a vecobs MLP beside it, 256 for the dense image encoder and for an image-less model
                               (encoders.py:25,34; then cnn_depth = img = img_ch = 0: no image geometry is read or sized) */
  int32_t A;                /* action_dim */
  int32_t mlp_hidden;       /* 400 (a2c.py:16, decoders.py:259,289) */
  int32_t mlp_layers;       /* 4  (defaults.yaml:83,85; a2c.py:17) */
  int32_t cnn_depth;        /* 48 */
  int32_t img, img_ch;      /* 64, 3 */
  int32_t flags;            /* bits 0-1: actor distribution, 0 = onehot, 1 = tanh_normal, 2 = normal_tanh (a2c.py:43-55);
                               bit 4 (DM_FLAG_IMAGE_U8): the `image` / `target` pointers of the conv encoder / decoder are the
                               replay's native uint8 (N,H,W,C) frames; x/255-0.5 and HWC->CHW (preprocessing.py:21-29) happen
                               inside the first conv's patch loader and the MSE kernel */
} dm_shape;
#define DM_FLAG_IMAGE_U8 16
/* bits 5-6: recurrent cell (rnn.py:40-67 `gru_type`): 0 = gru (nn.GRUCell), 1 = gru_layernorm (NormGRUCell, rnn.py:95-114),
 * 2 = gru_layernorm_dv2 (NormGRUCellLateReset, rnn.py:117-138) */
#define DM_FLAG_GRU_SHIFT 5
/* bit 7: mixed precision (the reference's `amp` switch, train.py:166; BASELINE configs[2]/[4]) for THIS call: every
 * contraction the call runs takes its operands rounded to bf16 (RNE) into bf16 MFMA with fp32 accumulation; results,
 * LayerNorm, losses and storage stay fp32.  Precision is a per-call argument (here, dm_mlp_params.precision, DM_GEMM_BF16);
 * there is no process-wide switch. */
#define DM_FLAG_BF16 128
/* dm_shape.C = 0: Gaussian latents - z is S wide, the prior / posterior parameter rows 2*S wide (mean | raw std). */
/* bits 8-9: gru_layers - 1 (GRUCellStack depth, rnn.py:40-67; up to 4 layers, plain GRU cells only) */
#define DM_FLAG_GRU_LAYERS_SHIFT 8
#define DM_FLAG_GRU_LAYERS_MASK (3 << DM_FLAG_GRU_LAYERS_SHIFT)
#define DM_FLAG_GRU_MASK (3 << DM_FLAG_GRU_SHIFT)

/* ---------------------------------------------------------------- library ---------------------- */
int dm_version(void);                 /* ABI version, currently 17 (v2: LayerNorm-GRU slots; v3: per-call precision; v4: GRUCellStack layer slots;
                                         v5: dm_kl_sampled_gauss_*, dm_chain_graph_*, dm_fp32_mode - additions only;
                                         v6: LayerNorm slots of GRUCellStack layers 1..3, dm_rssm_params grows to 58;
                                         v7: dm_wgrad_side_arm / _join, dm_dream_rollout_marks, dm_mlp_head_fwd_rows - additions only;
                                         v8: dm_rssm_lds_* replace dm_rssm_persist_*;
                                         v9: dm_bptt_fold_enable added; the split-bf16 fp32 product mode and its dm_fp32_mode query removed;
                                         v10: dm_gemm_dma_enable added; the dm_chain_graph_ family (hipGraph replay of the launch chains: GPU-neutral in three rounds of
                                         measurement) and the persistent BPTT kernel with its switch dm_rssm_lds_bwd_enable - slower inside the step at every shard size - removed;
                                         dm_prof_end reports 44 kinds;
                                         v11: dm_dec_l4_bwd_direct_enable added;
                                         v12: dm_rssm_lds_status_ack / dm_rssm_lds_gave_up; the native exchange step dm_rccl_* / dm_allreduce_grads;
                                              dm_rollout_fuse_act_enable;
                                         v13: dm_wgrad_side_touch added;
                                         v14: dm_conv_encoder_fwd_rows, dm_conv_decoder_mse_fwd_rows, dm_rssm_sequence_fwd_steps removed (the forward
                                              time-chunk pipeline);
                                         v15: the native exchange step dm_rccl_available / _version / _unique_id / _comm_init / _comm_destroy
                                              and dm_allreduce_grads removed;
                                         v16: dm_rssm_last_schedule added; later, still 16 (additions only): the per-cell categorical
                                              loss family dm_cat_target_index / dm_cat_image_loss / dm_cat_image_pred / dm_cat_concat_rows
                                              of the map probe; dm_replay_gather of the device-resident replay; dm_goals_stats /
                                              dm_goals_stats_ws_floats of the goals probe; the dm_gru_sequence_ family of the
                                              gru_probe baseline; dm_dense_image_rows / dm_elu_rows_fwd / dm_elu_rows_bwd /
                                              dm_cat_image_loss_mix of the dense categorical image path; dm_convt_kskip_enable;
                                              dm_kl_staged_enable; dm_dec_l4_fwd_shared_enable; dm_policy_draw /
                                              dm_policy_draw_ws_floats of the acting path; dm_policy_draw_mode of the
                                              collection loop; dm_metric_accum / dm_batch_stats / dm_masked_mean /
                                              dm_export_image_u8 of the trainer loop's device-side logging;
                                              dm_head_loss_catsup of the categorical reward decoder; dm_disag_reward /
                                              dm_ensemble_mse of Plan2Explore;
                                         v17: dm_gemm_plan_query added; later, still 17 (additions only): dm_cem_draw / dm_cem_update
                                              of the latent-space planner; dm_twohot_decode / dm_twohot_loss / dm_return_norm of the
                                              two-hot critic and the percentile return normalisation; dm_mlp_plan_query;
                                              dm_workspace_query; dm_conv_plan_query; dm_kl_free_fwd / dm_kl_free_bwd (free bits) and
                                              dm_twohot_head_loss (the symlog two-hot reward head) */
const char* dm_last_error(void);      /* thread-local message of the last failing call */
int dm_device_check(void);            /* DM_OK iff the current HIP device is gfx950 */
/* Scratch that serves any call below for this shape: the maximum of the fused operators' own workspace layouts (each sized
 * with every optional piece the shape could select), plus a slack of 4096 floats, in bytes.  Touches no device. */
size_t dm_workspace_bytes(const dm_shape* shp);
/* The terms of that maximum, in floats: parts[0..8) = conv encoder forward, conv encoder backward, conv decoder forward, conv
 * decoder backward, dm_rssm_sequence_fwd, dm_rssm_sequence_bwd, dm_dream_rollout (M = T * B * I rows), the MLP heads
 * (dm_mlp_ws_floats over (H + 1) * T * B * I rows).  A convolution part is 0 where its entry points refuse the geometry.  A
 * call given exactly its part runs the schedule it runs on dm_workspace_bytes.  n: room in parts (>= 8). */
int dm_workspace_query(const dm_shape* shp, size_t* parts, int n);
/* A stream confined to the CUs whose bit is set in mask[0..words) (32 CUs per word), for CU-reservation experiments (no
 * reference counterpart: torch exposes no CU masks). */
int dm_stream_create_cu_mask(const uint32_t* mask, int words, void** stream);
int dm_stream_destroy(void* stream);
/* Weight gradients off the critical chain.  In the world-model backward (train.py:189 loss_model.backward()) only the DATA
 * gradients are a chain - image decoder -> BPTT loop -> encoder; every weight / bias / LayerNorm gradient is a leaf that
 * nothing waits for until the gradient clip.  dm_wgrad_side_arm(1) arms the CALLING THREAD: while armed,
 * dm_conv_decoder_mse_bwd*() and dm_rssm_sequence_bwd() enqueue their parameter-gradient kernels on a library-owned
 * low-priority stream that waits (events) for the gradient rows they read, so they run beside the BPTT loop - a B-row
 * latency chain that leaves most CUs idle - instead of in front of / behind it (dm_rssm_sequence_bwd cuts its batched weight
 * gradients into up to four time chunks for this, armed or not: the sums are the same either way).
 * Contract while armed: the `ws` handed to such a call must not be reused by any other call before the join (the deferred
 * kernels read their gradient buffers, tables and split-K scratch there), and the parameter gradients are complete on
 * `stream` only after dm_wgrad_side_join(stream), which makes `stream` wait for the side stream and disarms the thread.
 * Unarmed (the default for every direct caller) everything is enqueued on the caller's stream.  Results are bit-identical
 * either way (same kernels, same arguments).  No reference counterpart (autograd orders these itself). */
int dm_wgrad_side_arm(int on);
int dm_wgrad_side_touch(void);          /* create the side stream now and give it one command: it then holds its hardware queue before later streams ask for one */
int dm_wgrad_side_join(void* stream);

/* ---------------------------------------------------------------- primitives ------------------- */
/* C[m,n] (ldc) = epi( sum_k A(m,k) * B(n,k) ), fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * a_layout 0: A(m,k) = A[m*lda+k]   1: A(m,k) = A[k*lda+m]
 * b_layout 0: B(n,k) = B[n*ldb+k]   1: B(n,k) = B[k*ldb+n]
 * epi(v) = act( v + bias[n] + add[m*ldadd+n] + (flags&DM_GEMM_ACCUM ? C[m,n] : 0) ), act = ELU if DM_GEMM_ELU.
 * Replaces torch.nn.functional.linear and its backward (common.py:37-65, rssm.py:138-146, rnn.py:48-49). */
#define DM_GEMM_ACCUM 1
#define DM_GEMM_ELU 2
#define DM_GEMM_BF16 256      /* this product only: operands rounded to bf16 (RNE) on their way into LDS, fp32 accumulation */
int dm_gemm_f32(int a_layout, int b_layout, int M, int N, int K,
                const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                const float* bias, const float* add, int ldadd, int flags,
                void* ws, size_t ws_bytes, void* stream);
/* The same product with operands STORED as bf16 (conf.amp's weight / activation twins: train.py:166 autocast casts them per
 * call, here they live in HBM in that format): fp32 accumulation, fp32 C and an optional bf16 twin C_h of it (same ldc).
 * Leading dimensions in elements; minor extents in multiples of 8, rows 16-byte aligned. */
int dm_gemm_bf16h(int a_layout, int b_layout, int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb,
                  float* C, int ldc, uint16_t* C_h, const float* bias, int flags, void* ws, size_t ws_bytes, void* stream);
/* Calls with DM_FLAG_BF16 keep bf16 twins of their activations / per-call weight copies and feed them to dm_gemm_bf16h's
 * kernel (activation arenas of such calls are larger: the *_acts_floats functions account for it; a backward entry point uses
 * the arena twins only if the forward call that filled that `acts` buffer wrote them - the library keeps a host-side note per
 * buffer).  1 / 0 switches that path on / off, -1 queries; returns the state.  Off = the fp32-storage products of dm_gemm_f32(DM_GEMM_BF16); results agree to fp32 summation order. */
int dm_bf16_twins_enable(int on);
/* fp32 products whose operands take the 16-byte load path run gemm_dma_kernel: global_load_lds (LDS-DMA) into a 2-3 stage LDS
 * ring, counted vmcnt across a raw s_barrier, inline-asm fragment reads (csrc/gemm.hip).  Same tiles, k order and epilogue as the
 * register-staged gemm_f32_kernel: bit-identical results, so the library picks per call: the LDS-DMA loop from 14 k-tiles per
 * work item up, the register-staged loop (higher residency) below.  1 / 0 switches it on / off, 2 = on for every k extent (the
 * bit-identity test), -1 queries; returns the state (default 1). */
int dm_gemm_dma_enable(int on);
/* Which kernel would answer a plain dense product, and how it would cut the work: the shape test of the skinny kernel and the
 * planner (tile / split-K cost model, main loop) that a launch runs, asked without a device.  mode 0 = a dm_gemm_f32 call, 1 = the
 * same with DM_GEMM_BF16, 2 = a dm_gemm_bf16h call (has_add is ignored).  base_align: the alignment in bytes to assume for the
 * operand base addresses (16: the 16-byte-load path, 4: the scalar-load path); ws_bytes: the split-K workspace of the call (0 =
 * none).  The answer follows dm_gemm_dma_enable's state.
 * out = {loop: 0 register-staged, 1 LDS-DMA, 2 bf16 operands, 3 bf16 storage, 4 skinny; tile index in dm_prof_end's order (-1
 * for skinny); split count; k per split; column groups; 1 if both operands take 16-byte loads; dm_prof_end's kind (-1 for
 * skinny); 0}.  Returns DM_OK, or the error the launch would return for that shape. */
int dm_gemm_plan_query(int mode, int a_layout, int b_layout, int M, int N, int K, int lda, int ldb, int ldc, int flags,
                       int has_add, int base_align, size_t ws_bytes, int32_t out[8]);
/* The gather-form transposed convolutions (decoder layer 3 forward, the encoder's data gradients; csrc/conv.hip) are one product
 * over the (hs + k/2 - 1)^2 class pixels of a frame, whose patches reach into a zero border.  In fp32 mode the rows of that
 * product are enumerated (chunk of 128 frames, yy, xx, frame in chunk), so that a row tile lies inside one class pixel, and the
 * tile loops walk a per-tile list of the 32-k tiles that hold a valid tap instead of all of them.  The terms left out are 0 * w:
 * same bits for finite weights.  1 / 0 switches it on / off (off: rows ordered (frame, yy, xx), every k-tile), -1 queries;
 * returns the state (default 1).  bf16-mode calls are not affected. */
int dm_convt_kskip_enable(int on);
/* What a convolution entry point would do at a shape - the plan its launch loop carries out (csrc/conv.hip), asked without a
 * device.  which 0 = dm_conv_encoder_fwd(_planes), 1 = dm_conv_encoder_bwd(_planes), 2 = dm_conv_decoder_mse_fwd, 3 =
 * dm_conv_decoder_mse_bwd(_rows); planes != 0: the _planes variant with reward_input (encoder only).  The answer follows
 * dm_convt_kskip_enable, dm_dec_l4_bwd_direct_enable and dm_bf16_twins_enable as they stand.
 * out[l], l = 0..4 = form | bits << 8 of layer l (encoder layers 0..3, decoder layers 1..4; -1: no such layer).  Forms: 0 direct
 * kernel (conv_direct.hip), 1 direct kernel with the reward / terminal planes, 2 explicit patch matrix, 3 implicit (gathered)
 * patch matrix, 4 gather-form transposed convolution, 5 column matrix + col2im, 6 one input pixel (the product writes NHWC).
 *   encoder forward: out[0] in {0, 2}, out[1..3] = 3;  encoder backward: out[0] in {0, 1, 2} is layer 0's weight gradient,
 *   out[l] in {4, 5} the data gradient out of layer l = 1..3;  decoder forward: out[l] in {0, 4, 5, 6};  decoder backward:
 *   out[l] in {0, 3}.
 * Bits: 1 the gather form's padded operand and weights are stored as bf16, 2 the layer's output channels are padded to a
 * multiple of 4 (decoder backward), 4 the data gradient is written at the padded pitch of the layer below, over a zero-filled
 * buffer (decoder backward).  out[5] = 1 if gather-form products skip the zero border's k-tiles; out[6..7] = 0.
 * need_floats (nullable): the workspace the call needs, in floats (at most the entry point's part of dm_workspace_query).
 * Returns DM_OK, or DM_E_SHAPE for a geometry the entry point refuses. */
int dm_conv_plan_query(int which, const dm_shape* shp, int planes, int32_t out[8], size_t* need_floats);
/* The categorical KL-balance kernels behind dm_kl_balance_fwd / _bwd address one group of C logits per lane.  Where the shape
 * fits (C <= 63: two tensors of 128 groups at pitch C + 1 in 64 KB of LDS; forward also S <= 32, where a wave takes two rows) a
 * workgroup first copies its groups into LDS with coalesced 16-byte loads, and the backward writes both gradients back through
 * LDS the same way (csrc/elementwise.hip).  Same arithmetic in the same order: same bits.  1 / 0 switches it on / off (off: the
 * per-lane-addressed kernels at every shape), -1 queries; returns the state (default 1).  Gaussian latents (C = 0) are not affected. */
int dm_kl_staged_enable(int on);
/* The image layer of the decoder (ConvTranspose2d(d -> 3, k6, s2), decoders.py:154-155) runs its backward - data gradient with
 * the ELU' of the layer below folded in, weight gradient - as two direct MFMA kernels that read the 3-channel output gradient
 * of a frame from LDS (csrc/conv_direct.hip) instead of as gather-form products through the generic tile (3 -> 4 channel pad, 48
 * columns in a 64-wide tile).  Same sums in another order (fp32 rounding only).  1 / 0 switches it on / off, -1 queries; returns
 * the state (default 1). */
int dm_dec_l4_bwd_direct_enable(int on);
/* The same layer's forward is, per parity class of the output, a 3 x 3 convolution over the input, and the four classes of a
 * class pixel read the same patch.  On: one kernel reads each patch element from LDS once for all 4 x 3 outputs, as the
 * (9 d) -> 12 product on v_mfma_f32_16x16x4_f32 - per output the same k-ordered chain of f32 FMAs from the bias - with the weights
 * in LDS.  Off: one class per wave on packed FMAs, the class weights as wave-uniform vector loads.  Same bits either way.
 * 1 / 0 switches it on / off, -1 queries; returns the state (default 1). */
int dm_dec_l4_fwd_shared_enable(int on);
/* The posterior T loop (rssm.py:38-58, cell rssm.py:125-153, nn.GRUCell rnn.py:40-67) runs, when the shape qualifies (plain
 * single-layer GRU, LayerNorm, categorical latents, B <= 64, the layer slices fit one CU's LDS), as ONE persistent kernel with
 * one workgroup per compute unit that keeps its 4-column slice of every layer's weights in LDS for all T steps and exchanges
 * the small activation rows through poison-filled per-step buffers (csrc/rssm_lds.hip) - instead of five
 * dependent launches per step that re-stream the weights.  Same arithmetic up to fp32 summation order, same sampler rule.
 * dm_rssm_lds_enable: 1 / 0 switches it on / off, 2 = on also for small models (slices under half a CU's LDS: tests), -1 queries;
 * returns the state (default 1).
 * Co-residency is checked with the occupancy API before the first launch of a variant (>= 1 workgroup per CU at its LDS size; the grid
 * never exceeds the CU count) and the spin loops are bounded (a cooperative launch was measured slower - it drains the other streams
 * around the kernel - and is not built).
 * dm_rssm_lds_status: non-zero once such a kernel has given up in a spin loop (that step's outputs are invalid; every later call
 * takes the launch chain).  dm_rssm_lds_status_ack: the same word, read AND cleared - the give-up is reported once
 * (Dreamer.check_device_status() / packed_metrics_host() raise on it) while the kernel stays switched off for the life of the
 * process (dm_rssm_lds_gave_up: the acknowledged status), so a trainer can restore a checkpoint and continue on the launch chain.
 * dm_rssm_lds_prof: 16 sums of clock ticks (100 MHz) of its workgroup 0, one per phase / sub-phase, since the last reset (diagnostic). */
int dm_rssm_lds_enable(int on);
int dm_bptt_fold_enable(int on);        /* launch schedule of the BPTT loop: the two LayerNorm+ELU backward stages of a step folded into the products
                                            that consume them, dx W = rstd (g W - mean(g) colsum(W) - mean(g xhat) xhat W), so those products start
                                            with their operand loads instead of a row reduction.  ON by default; -1 queries. */
int dm_rssm_lds_status(void);
int dm_rssm_lds_status_ack(void);
int dm_rssm_lds_gave_up(void);
int dm_rssm_lds_prof(unsigned long long* out16, int reset);

/* y = ELU(LayerNorm(x; gamma, beta, eps)) row-wise; stats[r] = {mean, rstd}. (common.py:44-49, rssm.py:105-115) */
int dm_ln_elu_fwd(int rows, int n, const float* x, int ldx, const float* gamma, const float* beta, float eps,
                  float* y, int ldy, float* stats, void* stream);
/* dx from dy; dgamma/dbeta overwritten (column sums over rows). */
int dm_ln_elu_bwd(int rows, int n, const float* x, int ldx, const float* y, int ldy, const float* stats,
                  const float* gamma, const float* dy, int lddy, float* dx, int lddx,
                  float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
/* out[c] = sum_r x[r*ld+c]  (bias gradients). */
int dm_colsum(int rows, int n, const float* x, int ld, float* out, void* ws, size_t ws_bytes, void* stream);

/* nn.GRUCell gate math (rnn.py:48-49; torch GRUCell: r,z,n row blocks).  gi,gh: (rows,3D) incl. biases. */
int dm_gru_gates_fwd(int rows, int D, const float* gi, const float* gh, const float* h_in, int ldh,
                     float* h_out, int ldo, void* stream);
/* dgi, dgh (rows,3D) overwritten; dh_in overwritten with the direct path dh_out*u (the gh path is added by the caller's GEMM). */
int dm_gru_gates_bwd(int rows, int D, const float* gi, const float* gh, const float* h_in, int ldh,
                     const float* dh_out, int lddh, float* dgi, float* dgh, float* dh_in, int lddi, void* stream);

/* OneHotCategorical(StraightThrough) sample (rssm.py:147-148,195-201; dreamer.py:198-200):
 * per group of C logits: p = softmax(logits); cdf = sequential fp32 cumsum(p);
 * idx = #{k : cdf_k <= u*cdf_{C-1}} clamped to C-1 (the inverse-CDF rule the oracle patches into torch.multinomial);
 * if forced_idx != NULL it is used instead of sampling.  onehot (rows, groups*C) with leading dim ldo.
 * C = 0 selects Gaussian latents (stoch_discrete = 0; rssm.py:202-203, functions.py:46-56 diag_normal): a `logits` row is
 * (mean[groups] | raw[groups]), std = 2 sigmoid(raw) + 0.1, `u` holds STANDARD-NORMAL draws and `onehot` receives
 * z = mean + std * u (Normal.rsample), groups wide; forced_idx must be NULL, idx (if given) is zero-filled. */
int dm_sample_onehot(int rows, int groups, int C, const float* logits, int ldl, const float* u,
                     const int32_t* forced_idx, float* onehot, int ldo, int32_t* idx, void* stream);

/* KL(post||prior), entropies (dreamer.py:326-343,369-379; torch/distributions/kl.py:248-252).  C = 0: rows of Gaussian
 * parameters (mean[S] | raw std[S]) and the Normal-Normal KL / entropies (torch/distributions/kl.py kl_normal_normal). */
int dm_kl_balance_fwd(int rows, int S, int C, const float* post, const float* prior,
                      float* kl, float* ent_post, float* ent_prior, void* stream);
/* dpost = scale_post * dKL/dpost, dprior = scale_prior * dKL/dprior (overwrite). */
int dm_kl_balance_bwd(int rows, int S, int C, const float* post, const float* prior,
                      float scale_post, float scale_prior, float* dpost, float* dprior, void* stream);
/* Free bits per row (DreamerV3's rule; the reference has no counterpart).  The kernels, dispatch branches and dm_kl_staged_enable
 * switch of the pair above, in this order per row r:
 *   kl[r], ent_post[r], ent_prior[r]: the expressions of dm_kl_balance_fwd in its order (the same bits)
 *   kl_clip[r] = fmaxf(free, kl[r]);  closed[r] = kl[r] <= free ? 1.0f : 0.0f
 * dm_kl_free_bwd: rows with closed[r] == 0 get dm_kl_balance_bwd's values; every element of the others (S C, or 2 S for C = 0) of
 * dpost and dprior is written +0.0f.  One launch each.  Checked on the host before the launch: a NULL post, prior, kl, kl_clip,
 * closed, dpost or dprior -> DM_E_NULL (ent_post, ent_prior are optional); S < 1, C < 0, free negative or not finite -> DM_E_SHAPE. */
int dm_kl_free_fwd(int rows, int S, int C, const float* post, const float* prior, float free, float* kl, float* kl_clip,
                   float* closed, float* ent_post, float* ent_prior, void* stream);
int dm_kl_free_bwd(int rows, int S, int C, const float* post, const float* prior, const float* closed, float scale_post,
                   float scale_prior, float* dpost, float* dprior, void* stream);
/* straight-through backward: dlogits (+)= softmax-jacobian(logits)^T dz per group (accumulate if accum). */
int dm_st_softmax_bwd(int rows, int groups, int C, const float* logits, int ldl, const float* dz, int lddz,
                      float* dlogits, int lddl, int accum, void* stream);

/* IWAE (iwae_samples = I > 1).  Row index n = (t*B + b)*I + i everywhere (rssm.py:35-41).
 * Sampled KL (dreamer.py:340-343): out[n] = log q(z_n) - log p(z_n), z given by its indices (rows,S). */
int dm_kl_sampled_fwd(int rows, int S, int C, const float* post, const float* prior, const int32_t* idx, float* out, void* stream);
/* dpost = scale*row_w[n]*(onehot - softmax(post)), dprior = -scale*row_w[n]*(onehot - softmax(prior)); row_w nullable. */
int dm_kl_sampled_bwd(int rows, int S, int C, const float* post, const float* prior, const int32_t* idx, float scale,
                      const float* row_w, float* dpost, float* dprior, void* stream);
/* The same for Gaussian latents (stoch_discrete = 0, rssm.py:202-203): post / prior rows are (mean | raw std), z (rows, S; row
 * stride ldz) is the reparameterised posterior sample, through which a gradient flows too: dz (row stride lddz) is
 * ACCUMULATED with scale*row_w[n]*d(log q - log p)/dz, dpost / dprior receive the explicit parameter gradients. */
int dm_kl_sampled_gauss_fwd(int rows, int S, const float* post, const float* prior, const float* z, int ldz, float* out,
                            void* stream);
int dm_kl_sampled_gauss_bwd(int rows, int S, const float* post, const float* prior, const float* z, int ldz, float scale,
                            const float* row_w, float* dpost, float* dprior, float* dz, int lddz, void* stream);
/* x (TB,I,W) -> out (TB,W): mode 0 mean over I, mode 2 sum, mode 1 (W = 1) -logavgexp(-x) (functions.py:97-102) with the
 * optional importance weights w_out (TB,I) = softmax_i(-x) = d out/d x_i. */
int dm_reduce_i(int TB, int I, int W, const float* x, int mode, float* out, float* w_out, void* stream);
/* out[r] = sum_j w[j]*x_j[r], j < count <= 8 (x: host array of device pointers, w: host floats): dreamer.py:362. */
int dm_combine_rows(int count, int64_t n, const float* const* x, const float* w, float* out, void* stream);
/* x[r, 0..n) *= w[r]*scale (ldx leading dim): per-sample importance weights on row gradients. */
int dm_scale_rows(int64_t rows, int n, float* x, int ldx, const float* w, float scale, void* stream);

/* rows of h and z multiplied by (1-reset[r]) (rssm.py:41,134-135). */
int dm_mask_rows(int rows, int n, const float* x, int ldx, const uint8_t* reset, float* y, int ldy, void* stream);

/* stride-2 "valid" conv patch gather / scatter used by ConvEncoder and ConvDecoder (encoders.py:80-96, decoders.py:144-161).
 * Small image (n, hs, ws) relates to big image (n, hb, wb) by y_big = 2*y_small + ky, ky in [0,k).
 * im2col: col[(n,ys,xs)][(ky,kx,c)] = big[n, 2ys+ky, 2xs+kx, c]   (big NHWC, or NCHW if big_nchw: col order (c,ky,kx))
 * col2im: big[n,y,x,c] = act( bias[c] + sum_{ky,kx valid} col[(n,ys,xs)][(ky,kx,c)] ) * (mul_elu_grad_of ? ELU'(ref) : 1) */
int dm_im2col_s2(int n, int hb, int wb, int c, int k, const float* big, int big_nchw, float* col, void* stream);
#define DM_C2I_ELU 1
int dm_col2im_s2(int n, int hb, int wb, int c, int k, const float* col, const float* bias, int flags,
                 const float* elu_ref, float* big, void* stream);

/* ---------------------------------------------------------------- fused operators -------------- */
/* MLP = [Linear, LayerNorm(eps 1e-3), ELU] x layers, Linear  (common.py:37-65). */
typedef struct dm_mlp_params {
  const float* w[DM_MAX_MLP_LAYERS + 1];   /* w[l]: (hidden,in_l) ; w[layers]: (out,hidden) */
  const float* b[DM_MAX_MLP_LAYERS + 1];
  const float* ln_g[DM_MAX_MLP_LAYERS];
  const float* ln_b[DM_MAX_MLP_LAYERS];
  int32_t precision;                       /* 0 = fp32; 1 = bf16 operands / fp32 accumulate for the calls given this struct */
  int32_t reserved_;
} dm_mlp_params;
typedef struct dm_mlp_grads {
  float* w[DM_MAX_MLP_LAYERS + 1];
  float* b[DM_MAX_MLP_LAYERS + 1];
  float* ln_g[DM_MAX_MLP_LAYERS];
  float* ln_b[DM_MAX_MLP_LAYERS];
} dm_mlp_grads;
size_t dm_mlp_acts_floats(int rows, int hidden, int layers);
/* scratch floats (incl. the split-K region) that are enough for dm_mlp_head_fwd* / dm_mlp_head_bwd over `rows` rows: an upper
 * bound over in_dim <= 4096, both precisions, any sparse_cols, with or without `acts` (a wider input runs, without the optional
 * pieces).  A smaller workspace is an error only below what the call must have; dm_mlp_plan_query tells. */
size_t dm_mlp_ws_floats(int rows, int hidden, int layers);
/* What a forward (which = 0) or backward (which = 1) call of a head would do, asked without a device: the plan every such call
 * makes before it launches.  base_align (16 or 4): the alignment in bytes to assume for x and every weight matrix (the
 * workspace counts as 16-byte aligned); normed: LayerNorm parameters given; precision: dm_mlp_params.precision; has_acts: an
 * activation set is given; has_wpack / has_add0 / has_sample: the internal callers' packed weights, sparse addend and fused
 * action sampler (the imagination rollout; 0 for the exported forwards); ws_bytes: the call's workspace.  The answer follows
 * dm_mlp_chain_min_rows.  The backward ignores in_dim, out_dim, ldx, sparse_cols and the has_* arguments.
 * out = {path: 0 row panels, 1 whole-MLP kernel, 2 per-layer launches; k0: the layer-0 columns multiplied densely (in_dim when
 * there is no sparse split); sparse addend: 0 none, 1 computed by the call, 2 the caller's; 1 if the call packs the whole-MLP
 * kernel's weights itself; 1 if it makes bf16 weight copies; 1 if the output layer rides in the last row-panel launch;
 * need_floats - the workspace floats the plan touches - low 32 bits; its high 32 bits}.  Optional pieces are dropped, in the
 * call as here, when ws_bytes has no room for them.  Returns DM_OK, or the error the call would return. */
int dm_mlp_plan_query(int which, int rows, int in_dim, int hidden, int layers, int out_dim, int ldx, int sparse_cols,
                      int base_align, int normed, int precision, int has_acts, int has_wpack, int has_add0, int has_sample,
                      size_t ws_bytes, int32_t out[8]);
/* acts may be NULL when no backward will follow (critic_target a2c.py:39,84; the dream's reward / terminal heads
 * dreamer.py:205-206; inference dreamer.py:92-111): activations then ping-pong through `ws` and nothing is saved.
 * For rows >= 16384 and hidden 400 each Linear -> LayerNorm -> ELU is ONE row-panel launch (csrc/panel.hip) and the output
 * layer (out_dim <= 32) rides in the last one's epilogue. */
int dm_mlp_head_fwd(int rows, int in_dim, int hidden, int layers, int out_dim,
                    const float* x, int ldx, const dm_mlp_params* p, float* acts, float* out,
                    void* ws, size_t ws_bytes, void* stream);
/* The same head when the LAST sparse_cols columns of x are known to be mostly zero - the one-hot latent part of a feature
 * row (rssm.py:83-84: feature = cat(h, z), z = 32 one-hot groups of 32).  Same result (x W^T = x_dense W_d^T + sum over the
 * non-zero e of x_e W^T[e], exact for ANY x); on the row-panel path layer 0 then multiplies only the dense columns and
 * adds the sparse ones as a sum of weight rows (63 % of that layer's flops for the 600 + 1024 feature).  acts / out as above,
 * dm_mlp_head_bwd unchanged. */
int dm_mlp_head_fwd_sparse(int rows, int in_dim, int sparse_cols, int hidden, int layers, int out_dim,
                           const float* x, int ldx, const dm_mlp_params* p, float* acts, float* out,
                           void* ws, size_t ws_bytes, void* stream);
/* Rows [row0, row0 + rows) of dm_mlp_head_fwd(_sparse) over rows_total rows; x, out and acts are the FULL arrays (acts
 * carved for rows_total rows, or NULL).  A row's result does not depend on the window, so a forward over 40 000 imagined
 * states can be issued in pieces as the rollout produces them (host mirror: the heads of the first horizon steps run on an
 * idle stream while the rollout finishes; dreamer.py:212-213, a2c.py:85,113 apply the heads to the stacked features). */
int dm_mlp_head_fwd_rows(int rows_total, int row0, int rows, int in_dim, int sparse_cols, int hidden, int layers, int out_dim,
                         const float* x, int ldx, const dm_mlp_params* p, float* acts, float* out,
                         void* ws, size_t ws_bytes, void* stream);

/* dout (rows,out_dim); grads overwritten; dx (rows,in_dim; ld lddx) written if non-null (accumulated if dx_accum). */
int dm_mlp_head_bwd(int rows, int in_dim, int hidden, int layers, int out_dim,
                    const float* x, int ldx, const dm_mlp_params* p, const float* acts, const float* dout,
                    const dm_mlp_grads* g, float* dx, int lddx, int dx_accum,
                    void* ws, size_t ws_bytes, void* stream);

/* loss epilogues of the dense heads: kind 0 = reward, 0.5*(mu-y)^2 + c (decoders.py:302-304); 1 = terminal,
 * BCE-with-logits (decoders.py:263-269).  loss[r]; dout[r] = scale * dloss/dout; mean_out[r] = mu or sigmoid(logit). */
int dm_head_loss(int kind, int rows, const float* out, const float* target, float scale, float loss_const,
                 float* loss, float* dout, float* mean_out, void* stream);

/* the same for a DenseNormalDecoder with out_dim = V > 1 (decoders.py:295-304, Independent(Normal, 1): the vecobs decoder):
 * out / target / dout / mean_out are (rows,V); loss[r] = 0.5 * sum_v (mu-y)^2 + V * loss_const; dout = scale * (mu-y). */
int dm_head_loss_normal_nd(int rows, int V, const float* out, const float* target, float scale, float loss_const,
                           float* loss, float* dout, float* mean_out, void* stream);

/* the same for a DenseCategoricalSupportDecoder (csrc/cat_support.hip; decoders.py:322-362 over CategoricalSupport,
 * common.py:77-86: reward_decoder_categorical): a categorical distribution over K fixed support values.
 * logits (rows, K) with leading dimension ld >= K; support (K) on the device; target (rows / I) - row r reads target r / I as
 * dm_cat_image_loss does, rows % I == 0.  With b = argmin_k (t - support[k])^2 - the reference's own fp32 arithmetic
 * (d = t - support[k], d * d, strict '<' scanning k upwards: bit for bit torch.square(t[:, None] - support).argmin(-1)):
 *   loss[r] = logsumexp_k x - x[b];  dlogits[r][k] = scale * (softmax_k - [k == b]), dense, leading dimension K;
 *   mean_out[r] = sum_k softmax_k * support[k];  bin[r / I] = b, int32 (rows / I).
 * Every output pointer is optional.  target == NULL is the mean-only form (the imagined rows, dreamer.py:212, where only
 * `.mean` is read): loss, dlogits and bin must then be NULL too; its mean_out has the bits of the full form's.
 * fp32 arithmetic with the maximum subtracted, whatever the precision of the products around it; one launch; no float atomics
 * (the same inputs give the same bits).  Checked on the host before anything is launched: K outside 2 .. 32, rows < 0, I < 1,
 * rows % I != 0 or ld < K -> DM_E_SHAPE; NULL logits or support, or a NULL target beside a non-NULL loss, dlogits or bin ->
 * DM_E_NULL; rows == 0 -> DM_OK with nothing launched. */
int dm_head_loss_catsup(int rows, int I, int K, const float* logits, int ld, const float* support, const float* target, float scale,
                        float* loss, float* dlogits, float* mean_out, int32_t* bin, void* stream);

/* Plan2Explore's disagreement ensemble (csrc/disag.hip; DreamerV2 expl.py - the reference has no counterpart): K one-step
 * predictors of the next stochastic state.  means is K blocks of (rows, D) with leading dimension ld >= D, block k starting
 * k * head_stride floats behind block 0; dmeans, where given, has the same layout.  fp32 arithmetic whatever the precision of
 * the products around them; one launch each; no float atomics and every sum in a fixed order (the same inputs give the same
 * bits); 16-byte accesses where a row's addresses allow them, else one float per lane.
 * The intrinsic reward, the heads' population standard deviation (ddof 0, expl.py's std(0)) averaged over the columns:
 *   reward[r] = scale * (1/D) * sum_d sqrt((1/K) * sum_k (x_k - mu)^2),  x_k = m_k[r][d] - m_0[r][d],  mu = (sum_k x_k) / K,
 * k ascending.  The shift by head 0 keeps only the heads' spread in the sums (no cancellation against a large common
 * value) and makes K identical heads give exactly 0.0f.  One wave per row: lane l adds its columns l, l + 64, ... in ascending
 * order, the 64 partial sums meet in an xor butterfly.  reward is dense, rows floats.
 * Checked on the host before anything is launched: K outside 2 .. 16, rows < 0, D < 1, ld < D or head_stride < 0 -> DM_E_SHAPE;
 * NULL means or reward -> DM_E_NULL; rows == 0 -> DM_OK with nothing launched. */
int dm_disag_reward(int K, int rows, int D, const float* means, int64_t head_stride, int ld, float scale, float* reward,
                    void* stream);
/* The heads' training loss against one target row each, -log Normal(y; m_k, 1) up to its constant:
 *   loss[k][r] = 0.5 * sum_d (m_k[r][d] - y[r][d])^2 (dense, K * rows floats);  dmeans = scale * (m_k - y), optional.
 * target (rows, D) with leading dimension ldt >= D: read in place out of a wider matrix (the feature rows' stochastic part).
 * skip (rows) uint8 or NULL: a row with skip[r] != 0 gets loss 0 and a zero dmeans row, and neither its means nor its target
 * are read.  One wave per (head, row).  Checked on the host as above, and ldt < D -> DM_E_SHAPE, NULL means, target or loss ->
 * DM_E_NULL. */
int dm_ensemble_mse(int K, int rows, int D, const float* means, int64_t head_stride, int ld, const float* target, int ldt,
                    const uint8_t* skip, float scale, float* loss, float* dmeans, void* stream);

/* Per-cell categorical losses over a (C, H, W) logit block (csrc/cat_image.hip): the map probe's CatImageDecoder
 * (decoders.py:183-254, probes.py:32-86).  A logit row is class-major as nn.Unflatten(-1, (C,H,W)) lays it out: class c of
 * cell p at c*cells + p, cells = H*W.  fp32 arithmetic whatever the precision of the products around it; no float atomics
 * (the same inputs give the same bits).  Arguments are checked on the host before anything is launched.
 * idx[r][p] = argmax_c onehot[r][c][p], the lowest class on equal values (decoders.py:221 / probes.py:75 target.argmax(dim=-3)):
 * onehot (rows, C, cells) -> idx (rows, cells) int32. */
int dm_cat_target_index(int rows, int C, int cells, const float* onehot, int32_t* idx, void* stream);
/* F.nll_loss(F.log_softmax(output, 1), target).sum([-1, -2]) (decoders.py:227,234): logits (rows, C*cells) with leading
 * dimension ld >= C*cells, target (rows / I, cells) int32 - row r reads target row r / I (decoders.py:241 insert_dim), rows % I == 0.
 * loss[r] = sum_p (logsumexp_c x[c][p] - x[target[p]][p]); dlogits (rows, C*cells), optional: softmax_c - onehot, unscaled. */
int dm_cat_image_loss(int rows, int I, int C, int cells, const float* logits, int ld, const int32_t* target, float* loss,
                      float* dlogits, void* stream);
/* The decoded map and its accuracy for `groups` frames of I rows each (logits (groups*I, C*cells), leading dimension ld).
 * logp (groups, C, cells), optional: log_softmax over C per row, logsumexp over the I rows, normalised over C again
 * (decoders.py:247-251).  acc[g] = fraction of cells with argmax_c logp == target (probes.py:79-81; lowest class on a tie).
 * seen (groups, cells) int32 mask and acc_seen, optional: acc_seen[g] = sum(hit * seen) / sum(seen), NaN for a frame without
 * a seen cell (probes.py:84; the caller's nanmean skips it).  I <= 256. */
int dm_cat_image_pred(int groups, int I, int C, int cells, const float* logits, int ld, const int32_t* target,
                      const int32_t* seen, float* logp, float* acc, float* acc_seen, void* stream);
/* out (rows, F + E) = [ x[r][0..F) (leading dimension ldx) | extra[r / I][0..E) ]: torch.cat((features, insert_dim(map_coord, 2, I)), -1)
 * of probes.py:54-55. */
int dm_cat_concat_rows(int rows, int I, int F, int E, const float* x, int ldx, const float* extra, float* out, void* stream);

/* The dense categorical image path (csrc/dense_image.hip): image_encoder = image_decoder = 'dense' on a categorical image, the
 * `minigrid` section of defaults.yaml.  DenseEncoder (encoders.py:99-125) is dm_dense_image_rows -> dm_mlp_head_fwd ->
 * dm_elu_rows_fwd, CatImageDecoder (decoders.py:183-254) is dm_mlp_head_fwd -> dm_cat_image_loss(_mix) / dm_cat_image_pred.
 * fp32 arithmetic, no float atomics (the same inputs give the same bits).  Checked on the host before any launch: a NULL
 * required pointer -> DM_E_NULL; rows < 0, any other size < 1 or a leading dimension below the row width -> DM_E_SHAPE;
 * rows == 0 -> DM_OK with nothing launched (as the dm_cat_image_ entries).
 * The encoder's input rows (encoders.py:50-61 followed by nn.Flatten, encoders.py:106):
 *   out[r] (leading dimension ldo) = [ image, class-major C*cells | reward[r] x cells | terminal[r] x cells ].
 * Exactly one of image_f32 (rows, C, cells) and class_i32 (rows, cells) is non-null: a float image is copied as it is (a
 * non-one-hot float image then gives the reference's result), a class map is expanded to 0/1 - a class outside [0, C) gives a
 * zero column and reads nothing out of bounds.  reward and terminal (rows,) come together or not at all (reward_input,
 * encoders.py:52-59); without them a row is C*cells wide.  Columns of `out` past the row width are not touched. */
int dm_dense_image_rows(int rows, int C, int cells, const float* image_f32, const int32_t* class_i32, const float* reward,
                        const float* terminal, float* out, int ldo, void* stream);
/* The activation() behind DenseEncoder's last Linear (encoders.py:116-118; dm_mlp_head_fwd ends in a bare Linear):
 * y = ELU(x) over (rows, n) with leading dimensions; dx = dy * ELU'(x) with the derivative taken from y (1 for y > 0, else
 * y + 1).  In place is allowed (x == y, dy == dx). */
int dm_elu_rows_fwd(int rows, int n, const float* x, int ldx, float* y, int ldy, void* stream);
int dm_elu_rows_bwd(int rows, int n, const float* y, int ldy, const float* dy, int lddy, float* dx, int lddx, void* stream);
/* CatImageDecoder.loss with 0 < min_prob < 1 (decoders.py:229-231): per cell s = softmax_c, p = (1 - m) s + m / C,
 * loss[r] = -sum_cells log p_target; dlogits (rows, C*cells), optional: -(1 - m) s_t (delta_ct - s_c) / p_t, unscaled.
 * logits, ld, target and I as in dm_cat_image_loss.  p_t >= m / C: loss and gradient stay finite when s_t underflows; a target
 * outside [0, C) contributes -log(m / C) and a zero gradient.  min_prob == 0 is dm_cat_image_loss (DM_E_SHAPE here). */
int dm_cat_image_loss_mix(int rows, int I, int C, int cells, const float* logits, int ld, const int32_t* target, float min_prob,
                          float* loss, float* dlogits, void* stream);

/* The goals probe's metrics (csrc/goals.hip; probes.py:113-135) over `rows` frames and G goals, one call, no host read:
 * goals, pred (rows, 2G) fp32 - coordinates (2g, 2g+1) belong to goal g, pred is the decoded mean already averaged over I;
 * visage (rows, G) fp32 or NULL.  out (8 floats, e.g. a slice of the step's metric buffer):
 *   out[0] mse_goals = mean over rows and goals of dx^2 + dy^2;
 *   out[1] var_goals = (1/G) * sum over the 2G coordinates of their unbiased (N - 1) variance over the rows, two-pass
 *          (mean, then sum (x - mean)^2); rows == 1 gives NaN as torch's var() does;
 *   out[2..7] mse_goal_age{0,5,10,50,200,1000}, written only when visage is given: the mean of dx^2 + dy^2 over the
 *          (row, goal) entries with vmin <= visage <= vmax, float compares against [0,0] [1,5] [6,10] [11,50] [51,200]
 *          [201,1000]; an empty bucket is 0 / 0 = NaN (the reference's nanmean(x * mask / mask)).
 * ws: dm_goals_stats_ws_floats(rows, G) floats of scratch.  No float atomics: the same inputs give the same bits.
 * Checked on the host before any launch: NULL goals / pred / out (or ws with rows > 0) -> DM_E_NULL, rows < 0 or G < 1 ->
 * DM_E_SHAPE, rows == 0 -> DM_OK with nothing launched. */
size_t dm_goals_stats_ws_floats(int rows, int G);
int dm_goals_stats(int rows, int G, const float* goals, const float* pred, const float* visage, float* out, void* ws,
                   size_t ws_bytes, void* stream);

/* uint8 ingest (preprocessing.py:21-29 to_image): src (n, h*w, c) uint8 HWC -> dst (n, c, h*w) float32,
 * x/255 - 0.5.  Lets the trainer hand the replay's native uint8 frames to training_step(). */
int dm_preprocess_image_u8(int64_t n, int hw, int c, const uint8_t* src, float* dst, void* stream);

/* ConvEncoder (encoders.py:72-96): 4 x (Conv2d k4 s2 + ELU), Flatten.  w[i]: (Cout,Cin,4,4) torch layout. */
typedef struct dm_conv_params { const float* w[5]; const float* b[5]; } dm_conv_params;
typedef struct dm_conv_grads { float* w[5]; float* b[5]; } dm_conv_grads;
size_t dm_conv_encoder_acts_floats(const dm_shape* shp);
int dm_conv_encoder_fwd(const dm_shape* shp, const float* image /* (N,ch,64,64) */, const dm_conv_params* p,
                        float* acts, float* embed /* (N,E) torch (c,y,x) order */, void* ws, size_t ws_bytes, void* stream);
int dm_conv_encoder_bwd(const dm_shape* shp, const float* image, const dm_conv_params* p, const float* acts,
                        const float* dembed, const dm_conv_grads* g, void* ws, size_t ws_bytes, void* stream);
/* The encoder with a leading dimension on embed / dembed (encoders.py:64-68: the vecobs encoder's output sits behind the image
 * embedding in the same buffer), and with reward_input when reward and terminal are both non-null (both null: the plain
 * 3-channel first layer).
 * reward_input (encoders.py:52-59): the reward and the terminal flag, reward / terminal (N,), enter the encoder as two more
 * input planes, each constant over its frame; w[0] is (d,5,4,4).  The first Conv2d has no padding, so a plane adds
 * r_n * sum_taps W[o,3] + t_n * sum_taps W[o,4] to every output pixel of frame n: the 5-channel image is never written, the
 * direct layer-1 kernels keep reading the 3-channel frame (float or uint8) and start from a per-frame bias table; the planes'
 * weight gradient, the same for all 16 taps, and the bias gradient come from one frame-weighted column sum over the layer's
 * output gradient.  cnn_depth in {8,16,32,48,64}, img_ch = 3.  ld_embed / ld_dembed >= 32 * cnn_depth: leading dimension
 * of embed / dembed (encoders.py:64-68 concatenates other encoders' outputs behind the image embedding); shp->E is not read. */
int dm_conv_encoder_fwd_planes(const dm_shape* shp, const float* image, const dm_conv_params* p, const float* reward,
                               const float* terminal, float* acts, float* embed, int ld_embed, void* ws, size_t ws_bytes,
                               void* stream);
int dm_conv_encoder_bwd_planes(const dm_shape* shp, const float* image, const dm_conv_params* p, const float* reward,
                               const float* terminal, const float* acts, const float* dembed, int ld_dembed,
                               const dm_conv_grads* g, void* ws, size_t ws_bytes, void* stream);

/* ConvDecoder + MSE (decoders.py:111-180): Linear F->32d, 4 x ConvTranspose2d (k 5,5,6,6; s2), ELU x3.
 * w[0],b[0] = Linear; w[1..4]: (Cin,Cout,k,k) torch layout.  loss_image[n] = 0.5*sum (pred-target)^2. */
size_t dm_conv_decoder_acts_floats(const dm_shape* shp);
/* float offset of the prediction (N, img, img, ch) NHWC inside `acts`: image_rec (decoders.py:177) is materialised by the
 * caller only when somebody reads it (pass image_rec = NULL to the forward) */
size_t dm_conv_decoder_pred_offset(const dm_shape* shp);
int dm_conv_decoder_mse_fwd(const dm_shape* shp, const float* feat, int ldf, const float* target,
                            const dm_conv_params* p, float* acts, float* loss_image, float* image_rec /* nullable, NCHW */,
                            void* ws, size_t ws_bytes, void* stream);
/* dfeat (N,F) accumulated (+=) ; scale = image_weight / (T*B).  _rows: an optional per-frame factor on top (IWAE weights). */
int dm_conv_decoder_mse_bwd_rows(const dm_shape* shp, const float* feat, int ldf, const float* target,
                                 const dm_conv_params* p, const float* acts, float scale, const float* row_scale,
                                 const dm_conv_grads* g, float* dfeat, int lddf, void* ws, size_t ws_bytes, void* stream);
int dm_conv_decoder_mse_bwd(const dm_shape* shp, const float* feat, int ldf, const float* target,
                            const dm_conv_params* p, const float* acts, float scale,
                            const dm_conv_grads* g, float* dfeat, int lddf, void* ws, size_t ws_bytes, void* stream);

/* RSSM posterior sequence (rssm.py:21-78,125-153,186-193; rnn.py:40-67). Parameter order of dm_rssm_params.p[]: */
enum {
  DM_RSSM_Z_W = 0, DM_RSSM_Z_B, DM_RSSM_A_W, DM_RSSM_IN_G, DM_RSSM_IN_B,
  DM_RSSM_GRU_WIH, DM_RSSM_GRU_WHH, DM_RSSM_GRU_BIH, DM_RSSM_GRU_BHH,
  DM_RSSM_PRIOR_H_W, DM_RSSM_PRIOR_H_B, DM_RSSM_PRIOR_G, DM_RSSM_PRIOR_B, DM_RSSM_PRIOR_W, DM_RSSM_PRIOR_OB,
  DM_RSSM_POST_H_W, DM_RSSM_POST_H_B, DM_RSSM_POST_E_W, DM_RSSM_POST_G, DM_RSSM_POST_B, DM_RSSM_POST_W, DM_RSSM_POST_OB,
  /* LayerNorm GRU cells only (NULL for gru; then GRU_BIH / GRU_BHH are NULL instead - these cells have no biases):
   * gru_layernorm: (G0,B0) = ln_reset, (G1,B1) = ln_update, (G2,B2) = ln_newval, D floats each;
   * gru_layernorm_dv2: (G0,B0) = lnorm, 3D floats */
  DM_RSSM_GRU_LN_G0, DM_RSSM_GRU_LN_B0, DM_RSSM_GRU_LN_G1, DM_RSSM_GRU_LN_B1, DM_RSSM_GRU_LN_G2, DM_RSSM_GRU_LN_B2,
  /* GRUCellStack layers 1..3 (rnn.py:40-67, gru_layers > 1, gru_type = gru): weight_ih, weight_hh, bias_ih, bias_hh each;
   * layer 0 is the DM_RSSM_GRU_* group above.  Layer i maps (i == 0 ? hidden : D/L) -> D/L and owns state columns
   * [i*D/L, (i+1)*D/L). */
  DM_RSSM_GRU_L1_WIH, DM_RSSM_GRU_L1_WHH, DM_RSSM_GRU_L1_BIH, DM_RSSM_GRU_L1_BHH,
  DM_RSSM_GRU_L2_WIH, DM_RSSM_GRU_L2_WHH, DM_RSSM_GRU_L2_BIH, DM_RSSM_GRU_L2_BHH,
  DM_RSSM_GRU_L3_WIH, DM_RSSM_GRU_L3_WHH, DM_RSSM_GRU_L3_BIH, DM_RSSM_GRU_L3_BHH,
  /* ... and, for a stack of LayerNorm cells (gru_layers > 1 with gru_layernorm / gru_layernorm_dv2; ABI v6), the LayerNorm
   * parameters of layers 1..3 in the (G0,B0,G1,B1,G2,B2) order of DM_RSSM_GRU_LN_* above, D/L (dv2: 3D/L) floats each. */
  DM_RSSM_GRU_L1_LN_G0, DM_RSSM_GRU_L1_LN_B0, DM_RSSM_GRU_L1_LN_G1, DM_RSSM_GRU_L1_LN_B1, DM_RSSM_GRU_L1_LN_G2, DM_RSSM_GRU_L1_LN_B2,
  DM_RSSM_GRU_L2_LN_G0, DM_RSSM_GRU_L2_LN_B0, DM_RSSM_GRU_L2_LN_G1, DM_RSSM_GRU_L2_LN_B1, DM_RSSM_GRU_L2_LN_G2, DM_RSSM_GRU_L2_LN_B2,
  DM_RSSM_GRU_L3_LN_G0, DM_RSSM_GRU_L3_LN_B0, DM_RSSM_GRU_L3_LN_G1, DM_RSSM_GRU_L3_LN_B1, DM_RSSM_GRU_L3_LN_G2, DM_RSSM_GRU_L3_LN_B2,
  DM_RSSM_NPARAMS
};
typedef struct dm_rssm_params { const float* p[DM_RSSM_NPARAMS]; } dm_rssm_params;
typedef struct dm_rssm_grads { float* p[DM_RSSM_NPARAMS]; } dm_rssm_grads;
size_t dm_rssm_acts_floats(const dm_shape* shp);
/* feat (N,F): [h | z]; post, prior (N,Z) logits; idx (N,S).  u (N,S) uniforms; forced_idx nullable. */
int dm_rssm_sequence_fwd(const dm_shape* shp, const float* embed, const float* action, const uint8_t* reset,
                         const float* h0, const float* z0, const float* u, const int32_t* forced_idx,
                         const dm_rssm_params* p, float* acts, float* feat, float* post, float* prior, int32_t* idx,
                         void* ws, size_t ws_bytes, void* stream);
/* dfeat (N,F) from decoders/heads (consumed, overwritten as scratch), dpost/dprior (N,Z) from the KL term.
 * Produces parameter grads and dembed (N,E). */
int dm_rssm_sequence_bwd(const dm_shape* shp, const float* embed, const float* action, const uint8_t* reset,
                         const dm_rssm_params* p, const float* acts, const float* feat, const float* post,
                         float* dfeat, float* dpost, float* dprior,
                         const dm_rssm_grads* g, float* dembed, void* ws, size_t ws_bytes, void* stream);

/* Schedule of this thread's most recent call: which = 0 dm_rssm_sequence_fwd, 1 dm_rssm_sequence_bwd, 2 dm_dream_rollout
 * (-1 for any other `which`, 0 before the first call).  The three entry points pick their launch schedule from the shape, the
 * switches above and the workspace size alone (csrc/rssm.hip plan()); this word is what they decided, stored once per call.
 * Read-only diagnostic: a parity test asserts with it that the schedule it is about is the one that ran. */
#define DM_SCHED_FWD_FUSE_LN 1          /* LayerNorm+ELU in the consuming product's prologue / in the z_embed gather */
#define DM_SCHED_FWD_FUSE_SAMPLE 2      /* the sampler in the posterior-logits product's epilogue */
#define DM_SCHED_FWD_FRAG 4             /* fragment-major operand copies taken */
#define DM_SCHED_FWD_WZT 8              /* z_mlp of the sampled latent as a gather-sum over z_mlp^T */
#define DM_SCHED_FWD_PSYNC 16           /* steps 1.. as the persistent LDS kernel */
#define DM_SCHED_BWD_FUSE_B 1           /* LayerNorm backward in prologues (or folded), gates backward in an epilogue */
#define DM_SCHED_BWD_FOLD 2             /* ... in folded form */
#define DM_SCHED_BWD_FOLD_SM 4          /* ... with the straight-through softmax backward in the closing pair's epilogue */
#define DM_SCHED_BWD_FRAG 8             /* fragment-major operand copies taken */
#define DM_SCHED_BWD_NCHUNK_SHIFT 8     /* bits 8-11: time chunks of the batched weight gradients (1, 2 or 4) */
#define DM_SCHED_BWD_NCHUNK_MASK (15 << DM_SCHED_BWD_NCHUNK_SHIFT)
#define DM_SCHED_ROLL_WZT 1             /* z_mlp (+ in_norm + ELU) as a gather-sum from the prior sampler's indices */
#define DM_SCHED_ROLL_WAT 2             /* a_mlp(action) as a row of a_mlp^T */
#define DM_SCHED_ROLL_ACTOR_WPACK 4     /* the actor on the whole-MLP kernel */
#define DM_SCHED_ROLL_ACTOR_ADD0 8      /* ... its first layer's z columns as a gathered sum */
#define DM_SCHED_ROLL_FUSE_ACT 16       /* the one-hot action draw in that kernel's output stage */
#define DM_SCHED_ROLL_TW_ON 32          /* bf16 twins of the cell's operands */
int dm_rssm_last_schedule(int which);

/* Plain GRU over a sequence (csrc/gru_seq.hip): the recurrent core of the `gru_probe` baseline, torch.nn.GRU(In, D), one
 * layer, time-major (baselines.py:322 self.rnn = nn.GRU(...), :339-341 the [squeezed embedding | action_next] input, :352
 * self.rnn(input, in_state)).  Gate order r, z, n as in torch's GRU: w_ih (3D, In), w_hh (3D, D), b_ih (3D), b_hh (3D), rows
 * [0, D) reset, [D, 2D) update, [2D, 3D) new:
 *   GI = X w_ih^T + b_ih (all T*B rows, one product);  per step GH_t = h_{t-1} w_hh^T + b_hh,
 *   r = sig(GI_r + GH_r), z = sig(GI_z + GH_z), n = tanh(GI_n + r GH_n), h_t = (h_{t-1} - n) z + n.
 * fp32 throughout, whatever other calls of the thread run in.  T, B, In, D >= 1 and D % 4 == 0, else DM_E_SHAPE.
 * x (T*B, In; leading dimension ldx), h0 (B, D), reset0 (B) bytes or NULL: h_0 = reset0[b] ? 0 : h0[b].  Resets of later
 * steps are not an input (nn.GRU has none).  H (T*B, D; leading dimension ldh) receives h_1 .. h_T; the final state is
 * its last B rows.  acts (dm_gru_sequence_acts_floats floats) keeps GI, GH and h_0 for dm_gru_sequence_bwd; acts == NULL:
 * forward only, nothing is kept and H has the same bits.  ws: dm_gru_sequence_ws_bytes bytes of scratch for either call.
 * Launch schedule of the forward step (dm_gru_sequence_last_schedule: that of this thread's last forward call):
 *   1  B <= 64, 3*D*D < 65536 (D <= 144) and H, w_hh, acts and ws 16-byte aligned with ldh % 4 == 0: ONE launch per step - a workgroup
 *      owns 4 hidden units, their r, z, n rows of w_hh share one v_mfma_f32_16x16x4_f32 tile, the gate arithmetic is that
 *      launch's epilogue;
 *   0  otherwise: the h w_hh^T product through the GEMM entry, then the dm_gru_gates_fwd kernel (measured faster than the
 *      one-launch step at D 600 / 1024 / 2048).
 * No atomics, no persistent kernel; every launch on `stream`; the same inputs give the same bits.
 * Backward: dH (T*B, D; leading dimension lddh, read-only) is dL/dH of every step.  Gradient buffers are OVERWRITTEN, as
 * dm_rssm_sequence_bwd and dm_mlp_head_bwd overwrite theirs: g->w_ih, g->w_hh, g->b_ih, g->b_hh and dx (T*B, In; leading
 * dimension lddx; nullable) hold this call's gradients alone afterwards, so a second call into the same buffers leaves the
 * same bits and a caller that accumulates over several calls adds them up itself.  No gradient goes to h0.  x, H and acts
 * must be those of the forward call. */
typedef struct dm_gru_params { const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh; } dm_gru_params;
typedef struct dm_gru_grads { float* w_ih; float* w_hh; float* b_ih; float* b_hh; } dm_gru_grads;
size_t dm_gru_sequence_acts_floats(int T, int B, int In, int D);
size_t dm_gru_sequence_ws_bytes(int T, int B, int In, int D);
int dm_gru_sequence_fwd(int T, int B, int In, int D, const float* x, int ldx, const float* h0, const uint8_t* reset0,
                        const dm_gru_params* p, float* acts, float* H, int ldh, void* ws, size_t ws_bytes, void* stream);
int dm_gru_sequence_bwd(int T, int B, int In, int D, const float* x, int ldx, const dm_gru_params* p, const float* acts,
                        const float* H, int ldh, const float* dH, int lddh, const dm_gru_grads* g, float* dx, int lddx,
                        void* ws, size_t ws_bytes, void* stream);
int dm_gru_sequence_last_schedule(void);
/* Which forward calls take schedule 1: 1 (default) = B <= 64 with 3*D*D < 65536; 0 = none; 2 = every B <= 64 call, whatever the
 * width (how scripts/gru_probe_bench.py regenerates the comparison of DESIGN 4.10 and how the tests reach the one-launch kernel
 * at wide states); -1 queries.  Process-wide; returns the state.  Alignment still applies: an unaligned call runs schedule 0. */
int dm_gru_sequence_fuse_enable(int on);

/* Progress marks for the NEXT dm_dream_rollout call of the calling thread (n <= 4; cleared by that call): events[i] - a
 * hipEvent_t owned by the caller - is recorded on the rollout's stream when horizon step steps[i] (0-based) has been
 * enqueued, i.e. when feature rows [0, (steps[i] + 2) * M) are final; marks that cannot be placed inside the loop (step out
 * of range, chain-graph replay) are recorded behind the call.  Lets the caller start per-row work on the first horizon
 * steps on another stream while the rollout continues.  No reference counterpart. */
int dm_dream_rollout_marks(int n, const int* steps, void* const* events);

/* Imagination rollout (dreamer.py:188-216, rssm.py:155-184, a2c.py:43-55), no autograd graph (actor_grad=reinforce).
 * start (M,F) = [h|z] rows; feats (H+1,M,F); actions (H,M,A) one-hot (or continuous); act_idx (H,M) (onehot only);
 * u_act: (H,M) uniforms for the one-hot actor, or (H,M,A) standard-normal noise for continuous actors (shp->flags);
 * u_prior (H,M,S).
 * actor_acts (dm_mlp_acts_floats(H*M, hidden, layers) floats) + actor_logits (H*M, A): optional (both or neither);
 * when given, the actor activations of all H steps are kept for dm_mlp_head_bwd (rows = H*M). */
int dm_dream_rollout(const dm_shape* shp, int M, const float* start, const dm_rssm_params* cell,
                     const dm_mlp_params* actor, const float* u_act, const float* u_prior,
                     float* feats, float* actions, int32_t* act_idx, float* actor_acts, float* actor_logits,
                     void* ws, size_t ws_bytes, void* stream);

/* GAE + reality weight (a2c.py:81-108). All (J,M)/(H,M) row-major with J=H+1. */
int dm_gae_losses(int H, int M, float gamma, float lambda, const float* reward, const float* terminal,
                  const float* value_t, float* advantage, float* advantage_gae, float* value_target, float* weight,
                  void* stream);
/* actor (reinforce, onehot) loss rows (a2c.py:119-130): loss[r] = (-logpi(a)*adv - ent_w*H[pi])*w;
 * dlogits = scale * dloss/dlogits. */
int dm_actor_loss(int rows, int A, const float* logits, const int32_t* act_idx, const float* adv_gae,
                  const float* weight, float ent_w, float scale, float* loss, float* entropy, float* dlogits, void* stream);
/* Continuous actors (functions.py:59-78; a2c.py:43-55,119-130): kind 1 = tanh_normal, kind 2 = normal_tanh.
 * params (rows,2A) = [mean_raw | std_raw]; eps (rows,A) standard-normal noise (torch.normal restated);
 * action = tanh(mean + std*eps) (kind 1) or mean + std*eps (kind 2). */
int dm_sample_continuous(int kind, int rows, int A, const float* params, const float* eps, float* action, void* stream);
/* reinforce rows: loss[r] = (-log pi(a)*adv - ent_w*H)*w with TransformedDistribution(Normal, Tanh) log-prob (kind 1) and the
 * base Normal's entropy; dparams (rows,2A) = scale * dloss/dparams. */
int dm_actor_loss_continuous(int kind, int rows, int A, const float* params, const float* actions, const float* adv_gae,
                             const float* weight, float ent_w, float scale, float* loss, float* entropy, float* dparams,
                             void* stream);
/* The acting path's draw (csrc/act.hip; generator.py:317-331 for `rows` environments): action, log-probability, entropy and the
 * generator's three logged means from the actor's output rows, explicit noise and the critic's outputs.  kind follows
 * dm_shape.flags bits 0-1: 0 = onehot, 1 = tanh_normal, 2 = normal_tanh.
 *   params   (rows, A) logits for kind 0, (rows, 2A) [mean_raw | std_raw] for kinds 1, 2; leading dimension ldp
 *   noise    kind 0: (rows) uniforms in [0,1); kinds 1, 2: (rows, A) standard normals
 *   value    (rows) critic outputs, or NULL
 *   action   (rows, A), leading dimension lda: the one-hot row (kind 0) or the continuous action
 *   act_idx  (rows) the drawn class (kind 0), zero-filled for kinds 1, 2; or NULL
 *   log_prob, entropy  (rows) each, or NULL
 *   stats    4 floats: mean value (0 with value == NULL), mean exp(log_prob), mean entropy, 0
 *   ws       dm_policy_draw_ws_floats(rows) floats of scratch
 * kind 0: the index is the one dm_sample_onehot(rows, 1, A, ...) gives for the same logits and uniforms, bit for bit (softmax,
 *   sequential fp32 cumsum in class order, idx = #{k : cdf_k <= u cdf_last} clamped to A - 1); log_prob = log_softmax[idx],
 *   entropy = -sum p log p.
 * kinds 1, 2: the action is the one dm_sample_continuous gives for the same params and noise, bit for bit; entropy is the base
 *   Normal's summed over A for both kinds (functions.py:77); log_prob is the Normal's at the draw x = mean + std eps, for kind 1
 *   plus sum_a -2 (log 2 - x_a - softplus(-2 x_a)), computed from the pre-tanh x - not from atanh of the (saturating) action.
 * Two launches, no float atomics: the same inputs give the same bits.  Checked on the host before any launch: NULL params,
 * noise, action, stats or ws -> DM_E_NULL; rows < 1, A < 1, kind outside {0, 1, 2}, ldp below the row width or lda < A ->
 * DM_E_SHAPE; ws_bytes below the scratch size -> DM_E_WORKSPACE. */
size_t dm_policy_draw_ws_floats(int rows);
int dm_policy_draw(int kind, int rows, int A, const float* params, int ldp, const float* noise, const float* value, float* action,
                   int lda, int32_t* act_idx, float* log_prob, float* entropy, float* stats, void* ws, size_t ws_bytes,
                   void* stream);
/* dm_policy_draw with a draw mode (csrc/act.hip; generator.py:317-331 acts, DreamerV2's behaviour policy adds the noise).  kind,
 * params, value, the outputs, stats and ws are dm_policy_draw's; the same two launches, no float atomics, the same bits for the same
 * inputs.
 *   mode 0   sample: dm_policy_draw for the same arguments, bit for bit on every output; noise2 and amount are not read
 *   mode 1   the distribution's mode, for evaluation; noise and noise2 are not read and may be NULL
 *            kind 0: idx = the lowest k with x_k == max_k x_k, the action its one-hot row, log_prob = (x_idx - max) - log(sum) with
 *              the sample path's sequential sum, the entropy unchanged
 *            kinds 1, 2: every output is what mode 0 gives for an all-zero noise array, bit for bit: action = tanh(5 tanh(m / 5))
 *              (tanh_normal) or tanh(m) (normal_tanh).  This is the mode of the BASE Normal pushed through the transform - not the
 *              sample-based mode (the best of a number of draws under log_prob) some Dreamer code uses.
 *   mode 2   sample, then action noise of size amount >= 0 (DreamerV2's rule for its behaviour policy)
 *            kind 0: noise2 (rows, 2) uniforms in [0,1).  idx is drawn from noise as in mode 0; where noise2[r][0] < amount (strict,
 *              fp32) it is replaced by min(A - 1, (int)floorf(noise2[r][1] * A)): the executed index is distributed as
 *              amount / A + (1 - amount) onehot(idx).  log_prob is the POLICY's log-probability of the executed index, not the
 *              mixture's.
 *            kinds 1, 2: noise2 (rows, A) standard normals.  action = clamp(a + amount noise2, -1, 1) with a the mode 0 action;
 *              the clamp is applied only with amount > 0.  log_prob and entropy stay those of the policy's own draw.
 *            amount == 0 gives the mode 0 outputs bit for bit for every kind, and noise2 is not read.
 * Checked on the host before any launch, beyond dm_policy_draw's checks: mode outside {0, 1, 2}, amount < 0 or NaN -> DM_E_SHAPE;
 * NULL noise with mode 0 or 2, NULL noise2 with mode 2 and amount > 0 -> DM_E_NULL. */
int dm_policy_draw_mode(int kind, int mode, float amount, int rows, int A, const float* params, int ldp, const float* noise,
                        const float* noise2, const float* value, float* action, int lda, int32_t* act_idx, float* log_prob,
                        float* entropy, float* stats, void* ws, size_t ws_bytes, void* stream);
/* Latent-space planning by the cross-entropy method (csrc/cem.hip; PlaNet's planner - the reference has no counterpart): the
 * candidate draw and the per-environment update between two open-loop rollouts.  B environments, J candidates each, Hp steps;
 * M = B J rows, row m = b J + j; (Hp, M, ...) arrays are time-major, as dm_rssm_sequence_fwd reads them.  kind follows
 * dm_shape.flags bits 0-1 (0 onehot, 1 tanh_normal, 2 normal_tanh; 1 and 2 behave the same here).
 * dm_cem_draw, one launch:
 *   kind 0      prop (B, Hp, A) probabilities, noise (Hp, M) uniforms in [0,1).  The index follows dm_sample_onehot's inverse-CDF
 *               rule on the probabilities themselves: sequential fp32 cumsum in class order, idx = #{k : cdf_k <= u cdf_last}
 *               clamped to A - 1.  actions (Hp, M, A) the one-hot rows, act_idx (Hp, M).
 *   kinds 1, 2  prop (B, Hp, 2A) = [mean | std], noise (Hp, M, A) standard normals; action = clamp(fl(mean + fl(std eps)), -1, 1)
 *               (product and sum rounded separately).  act_idx may be NULL and is not written.
 * dm_cem_update, one launch, one workgroup per environment:
 *   reward, terminal (Hp, M): the heads' means on the imagined states s_1 .. s_Hp; value (M): the critic on s_Hp, or NULL
 *   ret (M)     sum_t gamma^(t-1) w_t r_t (+ gamma^Hp w_(Hp+1) v), w_1 = 1, w_(t+1) = w_t (1 - terminal_t), accumulated in t order in
 *               fp32; written as computed.  For ranking a non-finite return counts as -FLT_MAX.
 *   elite (B, K) int32: the candidates j of rank < K in rank order, rank_j = #{i : r_i > r_j or (r_i = r_j and i < j)} - an exact
 *               comparison count, a function of the fp32 returns alone
 *   prop_out    kind 0: (1 - floor) (alpha prop_in + (1 - alpha) freq) + floor / A with freq[t][a] the elites' integer class counts
 *               over K; kinds 1, 2: mean_out = alpha mean_in + (1 - alpha) mean_e, std_out = max(alpha std_in + (1 - alpha) std_e,
 *               floor) with the elite mean and population std taken in two passes, each summed in rank order.  May alias prop_in.
 *   first_action (B, A): the t = 0 action of the rank-0 candidate
 *   stats (B, 4): best return, mean elite return (both over the ranking values), the entropy of prop_out at t = 0 (kind 0) or
 *               sum_a log std_out at t = 0 (kinds 1, 2), prop_out's probability of the executed class (kind 0) or 0
 * No float atomics, fixed summation orders: the same inputs give the same bits.  Neither entry takes scratch memory, so neither
 * returns DM_E_WORKSPACE.  Checked on the host before any launch: kind outside {0, 1, 2}, B < 1, J outside 1 .. 1024, Hp outside
 * 1 .. 64, A outside 1 .. 64, B J above INT_MAX / 64, K outside 1 .. J, alpha outside [0, 1], floor < 0 (kind 0: or > 1), a
 * non-finite gamma -> DM_E_SHAPE; a NULL required pointer (act_idx with kind 0 included; value is optional) -> DM_E_NULL. */
int dm_cem_draw(int kind, int B, int J, int Hp, int A, const float* prop, const float* noise, float* actions, int32_t* act_idx,
                void* stream);
int dm_cem_update(int kind, int B, int J, int K, int Hp, int A, float gamma, const float* reward, const float* terminal,
                  const float* value, const float* actions, const int32_t* act_idx, const float* prop_in, float alpha, float floor,
                  float* prop_out, float* ret, int32_t* elite, float* first_action, float* stats, void* stream);
/* The two-hot symlog critic and the percentile return normalisation (csrc/twohot.hip; DreamerV3's critic head and advantage
 * scaling - the reference has no counterpart).  fp32 throughout, compiled with floating-point contraction off: every product and
 * sum below is rounded on its own, in the order written.  No float atomics, no scratch memory (none of the three returns
 * DM_E_WORKSPACE): the same inputs give the same bits.  symlog(t) = copysign(log1pf(|t|), t), symexp(m) = copysign(expm1f(|m|), m).
 * logits (rows, K; leading dimension ld), bins: K strictly increasing floats in symlog space (any increasing support), 2 <= K <= 256.
 * One lane group per row: KP = the power of two >= K up to 64 lanes, E = 1, 2 or 4 elements per lane (element j = lane + e KP);
 * a sum over j is lane-local over e ascending, then an xor-butterfly over the KP lanes.
 * dm_twohot_decode, one launch:
 *   m = max_j logit_j;  e_j = expf(logit_j - m);  s = sum_j e_j;  p_j = e_j / s;  mu = sum_j p_j bins_j;  value[r] = symexp(mu)
 * dm_twohot_loss, one launch, for the rows r < rows:
 *   x = min(max(symlog(target[r]), bins[0]), bins[K-1]);  k = min(max(#{i : bins[i] <= x} - 1, 0), K - 2)
 *   w_hi = (x - bins[k]) / (bins[k+1] - bins[k]);  w_lo = 1 - w_hi;  lse = m + logf(s)
 *   loss[r] = weight[r] * ((lse - w_lo logit_k) - w_hi logit_{k+1})
 *   dlogits[r][j] = (scale * weight[r]) * (p_j - y_j),  y_k = w_lo, y_{k+1} = w_hi, 0 elsewhere      (dlogits: (rows_total, K) dense)
 *   rows [rows, rows_total) of dlogits are written as exact zeros (a2c.py's "value[-1] gets no gradient"); value (optional): the
 *   decoded value of the same logits, rows r < rows; dlogits may be NULL (the loss-only form; rows_total is then not used).
 * dm_return_norm, two launches (one when n_adv == 0): the q_lo and q_hi percentiles of the n values x by linear interpolation
 * between exact order statistics s_0 <= ... <= s_{n-1} (a radix select over the order-preserving integer image of the float in
 * one workgroup; -0 sorts below +0):
 *   pos = fl(q fl(n - 1));  i = floor(pos);  fr = fl(pos - i);  p = fl(s_i + fl(fr fl(s_{i+1} - s_i))),  s_n read as s_{n-1}
 *   update != 0:  state[c] = fl(fl(decay state[c]) + fl(fl(1 - decay) p_c)) for c = 0 (lo), 1 (hi); update == 0: state is read only
 *   scale = max(limit, fl(state[1] - state[0]));  adv[i] = fl(adv[i] / scale) for i < n_adv;  out[0..5) = [p_lo, p_hi, lo, hi, scale]
 *   Inputs are finite by contract; a non-finite one gives an unspecified result, the walk still ends and stays inside the arrays.
 * Checked on the host before any launch: K outside 2 .. 256, rows < 0, rows_total < rows, ld < K; n < 1, n_adv < 0, q outside
 * 0 <= q_lo <= q_hi <= 1, decay outside [0, 1), limit <= 0 or not finite -> DM_E_SHAPE; a NULL required pointer (logits, bins, value
 * for the decode; target, weight, loss for the loss; x, state, out, and adv with n_adv > 0) -> DM_E_NULL; rows == 0 -> DM_OK with
 * nothing launched. */
int dm_twohot_decode(int rows, int K, const float* logits, int ld, const float* bins, float* value, void* stream);
int dm_twohot_loss(int rows, int rows_total, int K, const float* logits, int ld, const float* bins, const float* target,
                   const float* weight, float scale, float* loss, float* dlogits, float* value, void* stream);
int dm_return_norm(int n, const float* x, float q_lo, float q_hi, float decay, float limit, int update, float* state, float* out,
                   float* adv, int n_adv, void* stream);
/* The head form of dm_twohot_loss (the symlog two-hot reward head): the same kernel instances, one launch.  rows = (t, b, i) rows
 * under iwae_samples = I; row r reads target[r / I]; there is no weight array.  With m, s, p_j, mu, x, k, w_hi, w_lo as above:
 *   lse = m + logf(s);  loss[r] = (lse - w_lo logit_k) - w_hi logit_{k+1};  dlogits[r][j] = scale * (p_j - y_j)   ((rows, K) dense)
 *   mean[r] = symexp(mu)
 * For I = 1 these are the bits of dm_twohot_loss with weight = 1 and rows_total = rows.  loss, dlogits and mean are each optional
 * (at least one is given); target == NULL is the mean-only form, the bits of dm_twohot_decode, and then loss and dlogits are NULL.
 * Checked on the host before the launch: K outside 2 .. 256, rows < 0, ld < K, I < 1, rows not a multiple of I -> DM_E_SHAPE; a
 * NULL logits or bins, no output at all, loss or dlogits without a target -> DM_E_NULL; rows == 0 -> DM_OK, nothing launched. */
int dm_twohot_head_loss(int rows, int I, int K, const float* logits, int ld, const float* bins, const float* target, float scale,
                        float* loss, float* dlogits, float* mean, void* stream);
/* critic loss rows (a2c.py:112-115): loss[r] = 0.5*(vt-v)^2*w ; dvalue = scale * -(vt-v)*w. */
int dm_critic_loss(int rows, const float* value, const float* value_target, const float* weight, float scale,
                   float* loss, float* dvalue, void* stream);

/* out[i] = scale[i] * sum(x_i[0..n_i)) for up to 32 arrays in one launch (losses / metrics, dreamer.py:362-379, a2c.py:133-147). */
typedef struct dm_reduce_item {
  const float* x; int64_t n; float scale;
  int32_t mode;            /* 0: sum x ; 1: sum (x - *center)^2 ; 2: sqrt(scale * sum (x - *center)^2)  (reward1.std(), a2c.py:140) */
  const float* center;     /* device scalar, mode 1 only */
} dm_reduce_item;
/* `out` is caller-provided: a step's losses and metrics are written side by side into ONE device buffer (Dreamer.metric_buffer),
 * so the trainer's ~20 per-metric .item() syncs (train.py:204-214) become one copy. */
int dm_multi_sum(int count, const dm_reduce_item* items /* host array */, float* out, void* stream);
/* out[0] = sum_i w[i] * x[i]  (x device, w host; count <= 16): loss_model from its weighted terms (dreamer.py:362-365). */
int dm_combine(int count, const float* x, const float* w, float* out, void* stream);

/* Optimizer (dreamer.py:60-87; torch.optim.AdamW defaults, clip_grad_norm_). */
/* norm_out[0] = ||g||_2 ; norm_out[1] = min(1, max_norm/(norm+1e-6)). */
int dm_multi_tensor_norm_clip(const float* grad, int64_t n, float max_norm, float* norm_out,
                              void* ws, size_t ws_bytes, void* stream);
/* x *= coef[0] (device scalar): the in-place gradient scaling of clip_grad_norm_. */
int dm_scale_inplace(float* x, int64_t n, const float* coef, void* stream);
/* AdamW step with the clip coefficient read from device memory (clip_coef may be NULL = 1): the same bits as
 * dm_scale_inplace(grad, n, clip_coef) followed by the NULL form. */
int dm_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  const float* clip_coef, void* stream);
int dm_copy_params(float* dst, const float* src, int64_t n, void* stream);   /* critic_target <- critic, a2c.py:151-152 */
/* Row threshold from which the 400-wide MLP heads run their whole forward as ONE launch (csrc/mlp_chain.hip; default 256,
 * below it the per-layer launches are faster).  rows >= 1 sets it; returns the previous value (rows < 1: query only). */
int dm_mlp_chain_min_rows(int rows);
/* The imagination rollout's one-hot action draw (dreamer.py:198-200) rides in the output stage of the whole-MLP actor kernel
 * (1, default) or runs as its own sampler launch (0); same rule and operation order: bit-identical draws.  -1 queries. */
int dm_rollout_fuse_act_enable(int on);
/* Optional per-launch timing of the GEMM kernel with HIP events on the launch stream (bench.py's roofline line).
 * dm_prof_begin arms up to max_launches slots; dm_prof_end synchronises on the events, fills
 * out[kind*4+{0,1,2,3}] = {launches, algorithmic flops (2MNK), milliseconds, algorithmic bytes 4(MK+NK+MN)} for
 * kind = tile*4 + a_layout*2 + b_layout with tile 0..4 = 128x128 / 128x64 / 64x64 / 128x96 / 96x128, kind 20 = row-panel
 * Linear+LayerNorm+ELU forward, 21 = row-panel backward, 22 = whole-MLP forward chain, 24 + kind = the same tile / layouts on the LDS-DMA
 * loop gemm_dma_kernel (44 kinds; nkinds >= 44; `out` holds 4*nkinds doubles) and returns the number of launches recorded.  (The <= 64-row skinny products are not in this set.) */
int dm_prof_begin(int max_launches);
int dm_prof_end(double* out, int nkinds);
/* Per-launch rows of the armed region (call before dm_prof_end): rows[i*8 + {0..7}] = {kind, M, N, K, split count, flags
 * (1 gathered A, 2 gathered B, 4 scatter epilogue, 8 bf16 operands, 32 bf16-storage operands), flops, milliseconds};
 * returns the row count. */
int dm_prof_rows(double* rows, int max_rows);
/* Device-resident replay (csrc/replay_gather.hip; pydreamer_amd/replay.py DeviceReplay): assembles the (T, B, ...) batch of up to
 * 16 fields in ONE launch out of episodes that live in device memory.  Batch column b is one or two pieces of episodes:
 *   pieces  device int32 (B, 2, 3) = {start row, length, mark}; the two lengths of a column add up to T (a single-piece column
 *           has length 0 in its second piece);
 *   src     device pointers (B, 2, nfields): the base of each field in the episode of that piece (an unused second piece may
 *           repeat the first one's);
 *   fields  HOST array: destination base, bytes per row, and whether the field is the reset column (one byte per row).
 * For t in piece p at offset t' :  dst_f[(t*B + b) * row_bytes ...] = src[b][p][f][(start + t') * row_bytes ...], and a piece with
 * mark != 0 writes 1 into the reset column at its first row (an artificial reset, data.py:280-300).  The access width per field
 * follows row_bytes: 16 B per lane if divisible by 16, else 4 B if divisible by 4, else bytes; destinations and source bases
 * must be 16-byte aligned (destinations are checked here, the device tables by whoever uploads them).  No atomics, no
 * workspace; the tables are read by the kernel, so they must stay valid until the launch has run. */
#define DM_REPLAY_MAX_FIELDS 16
typedef struct dm_replay_field {
  void* dst; int64_t row_bytes; int32_t is_reset; int32_t reserved_;
} dm_replay_field;
int dm_replay_gather(int T, int B, int nfields, const dm_replay_field* fields /* host array */, const int32_t* pieces,
                     const void* const* src, void* stream);
/* y = a*x + b*y */
int dm_axpby(int64_t n, float a, const float* x, float b, float* y, void* stream);

/* ---- the trainer loop's device-side logging (csrc/logging.hip; pydreamer_amd/train.py) ----
 * One launch each, nothing waits; no float atomics; reductions accumulate in fp64 in a fixed order (thread-strided partials, then
 * a fixed LDS tree) and round to fp32 once: the same inputs give the same bits.  Arguments are checked on the host first. */
/* Folds one step's scalars into running accumulators (train.py:204-214, 346-347, 387-389 without the .item() calls).  vals: n
 * floats (the model's metric buffer, or any device floats), n <= 256; rules: n device bytes; sum, maxv: n doubles; count: n int64.
 *   rule 0  the slot is left alone              rule 1  counted iff not NaN (inf is counted)
 *   rule 2  counted iff finite, and the max over the counted values is tracked
 *   rule 3  always counted                      rule 4  the max only (a NaN stays, as in numpy's max)
 * counted: sum += (double)v, count += 1 - in call order, so sum is what a Python float sum of the same values gives, exactly.
 * A max slot starts at -inf (the caller fills it).  A rule byte above 4 is treated as 0; the Python wrapper refuses it. */
int dm_metric_accum(int n, const float* vals, const uint8_t* rules, double* sum, double* maxv, int64_t* count, void* stream);
/* out4 = [mean reward, mean reset, mean terminal, max reward] over n = T*B elements (train.py:211-214).  reset: bool bytes,
 * counted in integers - its mean is fl32(count) / fl32(n); terminal may be NULL (gives 0); a NaN reward gives NaN in the mean
 * and in the max, as torch.max propagates it.  n <= 2^24. */
int dm_batch_stats(int n, const float* reward, const uint8_t* reset, const float* terminal, float* out4, void* stream);
/* out[0] = the mean of x[t][b] (row-major, leading dimension ldx) over t < min(take_rows, T) and the columns with col_keep[b] != 0
 * (col_keep NULL: all).  skip_nan = 1 leaves NaN elements out - nanmean(logprobs[:5] * mask / mask), train.py:365-372 -, skip_nan
 * = 0 is the plain IEEE mean - (loss_map.mean(0) * reset).sum() / reset.sum(), train.py:346.  The empty set gives NaN.  One
 * deliberate difference from the reference with skip_nan = 0: a non-finite value in a column that is NOT kept does not reach the
 * result here; there it poisons it through NaN * 0. */
int dm_masked_mean(int T, int B, const float* x, int ldx, int take_rows, const uint8_t* col_keep, int skip_nan, float* out,
                   void* stream);
/* A logged float image tensor (T,B,C,H,W) -> the npz layout (min(take_b,B), T, H, W, C) in uint8 (train.py:427, 447, 452, 462 in
 * one pass): fl32(fl32(x + 0.5f) * 255.0f) without contraction, clamped to [0, 255], truncated toward zero.  NaN gives 0 (numpy's
 * own cast of NaN to uint8 is undefined).  C is 1 or 3 and H == W, as the reference asserts. */
int dm_export_image_u8(int T, int B, int take_b, int C, int H, int W, const float* src, uint8_t* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DREAMER_HIP_H */
