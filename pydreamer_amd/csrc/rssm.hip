// RSSM posterior sequence with BPTT, batched prior, and the imagination rollout.
// Reference: RSSMCore.forward (rssm.py:21-78), RSSMCell.forward / forward_prior / batch_prior (rssm.py:125-193),
// nn.GRUCell via GRUCellStack (rnn.py:40-67), Dreamer.dream (dreamer.py:188-216), ActorCritic.forward_actor (a2c.py:43-55).
//
// Host code only: this file decides which launches a step makes.  Each entry point reads validate -> dimensions -> carve ->
// plan (a context struct: the buffers, the optional buffers it obtained, the schedule) -> a loop that calls one step
// function per iteration -> tail.
//  * Loop-invariant projections (a_mlp(action), post_mlp_e(embed), the batched prior) are hoisted out of the T loop as
//    (T*B)-row GEMMs.  h and z of every step are written straight into the (T*B, D+Z) feature matrix (h at column 0, z at
//    column D), so to_feature()'s concat (rssm.py:83-84) never materialises; consumers read sub-matrices through leading dims.
//  * T loop: post_step_fused (LayerNorm+ELU in the consuming product's prologue or in the z_embed gather, the sampler in the
//    logits product's epilogue) or post_step_plain; <= 32-row batches hand steps 1.. over to ONE persistent kernel (rssm_lds.hip).
//  * BPTT loop: bptt_step_fused (LayerNorm backward in prologues, or FOLDED over the producing product's epilogue and a plain
//    consumer; gates backward in an epilogue), bptt_step_single, bptt_step_stacked.  Only data-path products are in the loop:
//    the weight gradients are one ordered list, launched on the side stream in time chunks beside the loop (single-layer
//    cells) or in the tail (stacks); every bias / LayerNorm-parameter gradient is one column pass in the tail.
//  * Rollout: rollout_actor (actor + action draw), rollout_cell (prior cell, prior head, latent draw) per horizon step.
//  * Reset masks (rssm.py:41,134-135) are applied forward by the kernels that produce the next step's h and z (step 0: a
//    stand-alone mask kernel; the masked states are saved for backward) and backward through the products' row_zero option.
#include "common.h"

static inline int rssm_gru_kind(const dm_shape* s) { return (s->flags & DM_FLAG_GRU_MASK) >> DM_FLAG_GRU_SHIFT; }
static inline int rssm_gru_layers(const dm_shape* s) {
  return 1 + ((s->flags & DM_FLAG_GRU_LAYERS_MASK) >> DM_FLAG_GRU_LAYERS_SHIFT);
}
// Z: width of z (S one-hot groups of C, or S Gaussian dimensions when C = 0); ZP: width of the posterior / prior parameters
// (logits, or mean | raw std - rssm.py:112,117); F: width of a feature row [h | z]; N = T*B; kind: 0 nn.GRUCell, 1 / 2 the
// LayerNorm cells
struct RssmDims {
  int T, B, N, D, Hd, S, C, Z, ZP, F, E, A, kind, layers;
  bool gauss;
};
static void rssm_dims(const dm_shape* s, RssmDims* d) {
  d->T = s->T; d->B = s->B; d->N = s->T * s->B; d->D = s->D; d->Hd = s->Hd; d->S = s->S; d->C = s->C;
  d->Z = s->S * (s->C ? s->C : 1); d->ZP = s->S * (s->C ? s->C : 2); d->F = d->D + d->Z; d->E = s->E; d->A = s->A;
  d->gauss = s->C == 0; d->kind = rssm_gru_kind(s); d->layers = rssm_gru_layers(s);
}

struct RssmActs {
  float *ea, *ee, *hin, *zin, *x1, *st1, *za, *gi, *gh, *x2, *st2, *pin, *x3, *st3, *prin;
  float *gs, *gst;      // LayerNorm GRU cells: pre-LayerNorm gate sums (N,3D) and their statistics (N,6 per stack layer)
};
static size_t rssm_carve(const RssmDims& d, float* base, RssmActs* a) {
  const size_t N = (size_t)d.T * d.B, Hd = d.Hd, D = d.D, Z = d.Z;
  DmArena ar(base, (size_t)1 << 62);
  RssmActs t;
  t.ea = ar.take(N * Hd); t.ee = ar.take(N * Hd);
  t.hin = ar.take(N * D); t.zin = ar.take(N * Z);
  t.x1 = ar.take(N * Hd); t.st1 = ar.take(N * 2); t.za = ar.take(N * Hd);
  t.gi = ar.take(N * 3 * D); t.gh = ar.take(N * 3 * D);
  t.x2 = ar.take(N * Hd); t.st2 = ar.take(N * 2); t.pin = ar.take(N * Hd);
  t.x3 = ar.take(N * Hd); t.st3 = ar.take(N * 2); t.prin = ar.take(N * Hd);
  t.gs = ar.take(d.kind ? N * 3 * D : 0); t.gst = ar.take(d.kind ? N * 6 * d.layers : 0);
  if (a) *a = t;
  return ar.off;
}
extern "C" size_t dm_rssm_acts_floats(const dm_shape* shp) {
  if (!shp) return 0;
  RssmDims d;
  rssm_dims(shp, &d);
  return rssm_carve(d, nullptr, nullptr);
}

static int rssm_check(const dm_shape* s) {
  DM_REQUIRE(s->I == 1, DM_E_SHAPE, "rssm: iwae_samples=%d unsupported (only 1)", s->I);
  DM_REQUIRE(s->T >= 1 && s->B >= 1 && s->D >= 4 && s->Hd >= 4 && s->S >= 1 && (s->C >= 2 || s->C == 0) && s->A >= 1 && s->E >= 1,
             DM_E_SHAPE, "rssm: bad shape");
  DM_REQUIRE((s->D & 3) == 0, DM_E_SHAPE, "rssm: deter_dim must be a multiple of 4 (got %d)", s->D);
  DM_REQUIRE(rssm_gru_kind(s) <= 2, DM_E_SHAPE, "rssm: unknown recurrent cell kind %d", rssm_gru_kind(s));
  const int GL = rssm_gru_layers(s);
  DM_REQUIRE(s->D % (4 * GL) == 0, DM_E_SHAPE, "rssm: deter_dim=%d must be a multiple of 4*gru_layers (%d)", s->D, 4 * GL);
  return DM_OK;
}

// GRUCellStack (rnn.py:40-67): L cells (nn.GRUCell, or one of the two LayerNorm cells) of width ls = D/L.  Layer i reads x_i (x_0 = the cell input, x_i = the NEW
// state of layer i-1) and its own slice [i*ls, (i+1)*ls) of the incoming state, and writes the same slice of the new
// state.  The gate products of layer i live at columns [3*ls*i, 3*ls*(i+1)) of the (rows, 3D) gi / gh matrices (and of
// gs / dg for the LayerNorm cells, whose statistics of layer i are columns [6i, 6i+6) of the (rows, 6L) gst matrix).
struct GruStack {
  int L, ls, kind;
  const float *wih[4], *whh[4], *bih[4], *bhh[4];
  float *g_wih[4], *g_whh[4], *g_bih[4], *g_bhh[4];
  const float *lng[4][3], *lnb[4][3];      // LayerNorm cells: (reset, update, newval) or slot 0 = the one 3*ls-wide LayerNorm
  float *g_lng[4][3], *g_lnb[4][3];
};
static int gru_stack(const dm_shape* s, const float* const* p, float* const* g, GruStack* k) {
  k->L = rssm_gru_layers(s);
  k->ls = s->D / k->L;
  k->kind = rssm_gru_kind(s);
  for (int i = 0; i < k->L; ++i) {
    const int lb = i == 0 ? DM_RSSM_GRU_LN_G0 : DM_RSSM_GRU_L1_LN_G0 + 6 * (i - 1);
    for (int q = 0; q < 3; ++q) {
      k->lng[i][q] = p[lb + 2 * q]; k->lnb[i][q] = p[lb + 2 * q + 1];
      k->g_lng[i][q] = g ? g[lb + 2 * q] : nullptr; k->g_lnb[i][q] = g ? g[lb + 2 * q + 1] : nullptr;
      const bool need = k->kind == 1 || (k->kind == 2 && q == 0);
      DM_REQUIRE(!need || (k->lng[i][q] && k->lnb[i][q]), DM_E_NULL, "rssm: LayerNorm GRU layer %d without LayerNorm parameter %d",
                 i, q);
      DM_REQUIRE(!need || !g || (k->g_lng[i][q] && k->g_lnb[i][q]), DM_E_NULL,
                 "rssm: LayerNorm GRU layer %d without LayerNorm gradient slot %d", i, q);
    }
    const int b = i == 0 ? DM_RSSM_GRU_WIH : DM_RSSM_GRU_L1_WIH + 4 * (i - 1);
    k->wih[i] = p[b]; k->whh[i] = p[b + 1]; k->bih[i] = p[b + 2]; k->bhh[i] = p[b + 3];
    const bool biased = rssm_gru_kind(s) == 0;      // the LayerNorm cells have no gate biases (rnn.py:99-100)
    DM_REQUIRE(k->wih[i] && k->whh[i] && (!biased || (k->bih[i] && k->bhh[i])), DM_E_NULL,
               "rssm: GRU layer %d has a null parameter", i);
    if (g) {
      k->g_wih[i] = g[b]; k->g_whh[i] = g[b + 1]; k->g_bih[i] = g[b + 2]; k->g_bhh[i] = g[b + 3];
      DM_REQUIRE(k->g_wih[i] && k->g_whh[i] && (!biased || (k->g_bih[i] && k->g_bhh[i])), DM_E_NULL,
                 "rssm: GRU layer %d has a null gradient slot", i);
    }
  }
  return DM_OK;
}

// The cell's three norms (rssm.py:103-116) are nn.LayerNorm(eps 1e-3) or, with layer_norm=False, NoNorm (common.py:68-74:
// identity, no parameters): a null gain selects the activation alone, and no statistics / parameter gradients exist.
static int norm_elu_fwd(int rows, int n, const float* x, int ldx, const float* gamma, const float* beta, float eps, float* y,
                        int ldy, float* stats, hipStream_t st) {
  if (gamma) return dm_ln_elu_fwd_launch(rows, n, x, ldx, gamma, beta, eps, y, ldy, stats, st);
  return dm_elu_fwd_launch(rows, n, x, ldx, y, ldy, st);
}
static int norm_elu_bwd_dx(int rows, int n, const float* x, int ldx, const float* y, int ldy, const float* stats,
                           const float* gamma, const float* dy, int lddy, float* dx, int lddx, hipStream_t st) {
  if (gamma) return dm_ln_elu_bwd_dx_launch(rows, n, x, ldx, y, ldy, stats, gamma, dy, lddy, dx, lddx, st);
  return dm_elu_bwd_launch(rows, n, y, ldy, dy, lddy, dx, lddx, st);
}
static int norm_elu_bwd_params(int rows, int n, const float* x, int ldx, const float* y, int ldy, const float* stats,
                               const float* dy, int lddy, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                               hipStream_t st) {
  if (!dgamma && !dbeta) return DM_OK;
  return dm_ln_elu_bwd_params_launch(rows, n, x, ldx, y, ldy, stats, dy, lddy, dgamma, dbeta, ws, ws_bytes, st);
}

// y = x @ W^T (+ bias) (+ add): the descriptor (the chain steps add prologues, epilogues and fragment copies), and the launch
static DmGemm linear_q(int rows, int nout, int kin, const float* x, int ldx, const float* W, const float* bias,
                       const float* add, int ldadd, float* y, int ldy) {
  DmGemm q;
  q.M = rows; q.N = nout; q.K = kin;
  q.A = x; q.lda = ldx;
  q.B = W; q.ldb = kin;
  q.C = y; q.ldc = ldy;
  q.bias = bias; q.add = add; q.ldadd = ldadd;
  return q;
}
static int linear(hipStream_t st, void* sk, size_t skb, int rows, int nout, int kin, const float* x, int ldx,
                  const float* W, const float* bias, const float* add, int ldadd, float* y, int ldy) {
  return dm_gemm_launch(linear_q(rows, nout, kin, x, ldx, W, bias, add, ldadd, y, ldy), sk, skb, st);
}
// dW[o][i] = sum_r dy[r][o] x[r][i]
static int wgrad(hipStream_t st, void* sk, size_t skb, int rows, int nout, int kin, const float* dy, int lddy,
                 const float* x, int ldx, float* dW, int accum = 0) {
  DmGemm q;
  q.a_layout = 1; q.b_layout = 1;
  q.M = nout; q.N = kin; q.K = rows;
  q.A = dy; q.lda = lddy;
  q.B = x; q.ldb = ldx;
  q.C = dW; q.ldc = kin;
  q.flags = accum ? DM_GEMM_ACCUM : 0;
  return dm_gemm_launch(q, sk, skb, st);
}
// dx[r][i] (+)= mask_r * sum_o dy[r][o] W[o][i]
static int dgrad(hipStream_t st, void* sk, size_t skb, int rows, int nout, int kin, const float* dy, int lddy,
                 const float* W, float* dx, int lddx, int accum, const uint8_t* row_zero) {
  DmGemm q;
  q.a_layout = 0; q.b_layout = 1;
  q.M = rows; q.N = kin; q.K = nout;
  q.A = dy; q.lda = lddy;
  q.B = W; q.ldb = kin;
  q.C = dx; q.ldc = lddx;
  q.flags = accum ? DM_GEMM_ACCUM : 0;
  q.row_zero = row_zero;
  return dm_gemm_launch(q, sk, skb, st);
}

// dx[r][i] (+)= mask_r * sum_o dy[r][o] Wt[i][o]   (Wt = W^T materialised once per backward pass: the B-row chain
// products of the BPTT loop then read their weights k-contiguous, the layout the skinny kernel streams fastest)
static DmGemm dgrad_t_q(int rows, int nout, int kin, const float* dy, int lddy, const float* Wt, float* dx, int lddx,
                        int accum, const uint8_t* row_zero) {
  DmGemm q;
  q.M = rows; q.N = kin; q.K = nout;
  q.A = dy; q.lda = lddy;
  q.B = Wt; q.ldb = nout;
  q.C = dx; q.ldc = lddx;
  q.flags = accum ? DM_GEMM_ACCUM : 0;
  q.row_zero = row_zero;
  return q;
}
static int dgrad_t(hipStream_t st, void* sk, size_t skb, int rows, int nout, int kin, const float* dy, int lddy,
                   const float* Wt, float* dx, int lddx, int accum, const uint8_t* row_zero) {
  return dm_gemm_launch(dgrad_t_q(rows, nout, kin, dy, lddy, Wt, dx, lddx, accum, row_zero), sk, skb, st);
}
static int transpose(hipStream_t st, const float* W, float* Wt, int rows, int cols) {
  return dm_permute4_launch(W, Wt, 1, 1, rows, cols, 0, 1, 3, 2, st);
}

// One step of the stack, forward: 3 launches per layer.  `hout` may alias nothing of `hin`.
static int gru_stack_fwd(hipStream_t st, void* sk, size_t skb, const GruStack& k, int rows, int Hd, int D, const float* x0,
                         const float* hin, int ldh, float* gi, float* gh, float* hout, int ldo, float* h_next,
                         const uint8_t* next_reset, float* gs, float* gst) {
  const int ls = k.ls;
  for (int i = 0; i < k.L; ++i) {
    const float* x = i == 0 ? x0 : hout + (size_t)(i - 1) * ls;
    const int ldx = i == 0 ? Hd : ldo, kin = i == 0 ? Hd : ls;
    DM_TRY(linear(st, sk, skb, rows, 3 * ls, kin, x, ldx, k.wih[i], k.bih[i], nullptr, 0, gi + 3 * ls * i, 3 * D));
    DM_TRY(linear(st, sk, skb, rows, 3 * ls, ls, hin + i * ls, ldh, k.whh[i], k.bhh[i], nullptr, 0, gh + 3 * ls * i, 3 * D));
    if (k.kind == 0)
      DM_TRY(dm_gru_gates_fwd_launch(rows, ls, gi + 3 * ls * i, gh + 3 * ls * i, hin + i * ls, ldh, hout + i * ls, ldo,
                                     h_next ? h_next + i * ls : nullptr, next_reset, nullptr, nullptr, st, 3 * D, D));
    else
      DM_TRY(dm_gru_norm_fwd_launch(k.kind, rows, ls, gi + 3 * ls * i, gh + 3 * ls * i, hin + i * ls, ldh, k.lng[i], k.lnb[i],
                                    hout + i * ls, ldo, gs + 3 * ls * i, gst + 6 * i, h_next ? h_next + i * ls : nullptr,
                                    next_reset, st, 3 * D, 6 * k.L, D));
  }
  return DM_OK;
}

// Schedule of this thread's most recent call of each entry point (include/dreamer_hip.h dm_rssm_last_schedule): one store
// per call, right after plan() - a report of what plan() decided, read by tests; nothing in the library reads it back.
static thread_local int tl_last_schedule[3] = {0, 0, 0};
extern "C" int dm_rssm_last_schedule(int which) { return which >= 0 && which < 3 ? tl_last_schedule[which] : -1; }

// ---------------------------------------------------------------- posterior T loop --------------
// The chain's workspace: [split-K | optional blocks], each block taken if the schedule wants it (PostCtx::plan) and it fits -
// a small workspace keeps the schedule without it, its pointers null.  On an arena without a base it sizes.
struct PostWs {
  // z_mlp of the sampled (one-hot) latent as a gather-sum over rows of z_mlp^T (dm_z_embed_launch): every step after the
  // first takes its z from the sampler, whose indices are at hand; the first step's z comes from the caller as a dense
  // vector and keeps the product.
  float* wzt;
  // Fragment-major copies of the chain's <= 64-row operands (common.h dm_frag_off), written by the kernel that produces
  // each operand next to its ordinary copy and read by the product that consumes it: z_in -> x1 -> (gi | gh from h_in)
  // -> h -> x2 -> z.  One buffer per operand is enough (producer and consumer alternate in stream order).
  float *zinf, *x1f, *hinf, *hf, *x2f;
  // The fused schedule's steps after the first as ONE persistent kernel with the cell's weights stationary in
  // LDS (rssm_lds.hip): the first step runs as launches (its z is a dense vector from the caller) and leaves h, the masked
  // inputs and the indices the kernel's first step continues from.  Needs wzt.
  float* psync; size_t psync_floats;
};
static size_t post_layout(DmArena ar, const RssmDims& d, bool want_wzt, bool want_frag, bool want_psync, PostWs* w) {
  *w = {};
  ar.take(DM_SPLITK_FLOATS);
  if (want_wzt) {
    const size_t mark = ar.off;
    w->wzt = ar.take((size_t)d.Z * d.Hd);
    if (!ar.fits()) { w->wzt = nullptr; want_psync = false; ar.give_back(mark); }
  }
  if (want_frag) {
    w->zinf = ar.take(dm_frag_floats(d.Z)); w->x1f = ar.take(dm_frag_floats(d.Hd)); w->hinf = ar.take(dm_frag_floats(d.D));
    w->hf = ar.take(dm_frag_floats(d.D)); w->x2f = ar.take(dm_frag_floats(d.Hd));
    if (!ar.fits()) w->zinf = w->x1f = w->hinf = w->hf = w->x2f = nullptr;      // (not given back: nothing behind them fits either)
  }
  if (want_wzt && want_psync) {
    w->psync_floats = dm_rssm_lds_ws_floats(d.B, d.D, d.Hd, d.S, d.C, d.T - 1);
    w->psync = ar.take(w->psync_floats);
    if (!ar.fits()) w->psync = nullptr;
  }
  return ar.off;
}

struct PostCtx : RssmDims, PostWs {
  RssmActs a; GruStack gk;
  const float* const* p; hipStream_t st; void* ws; size_t skb;      // ws: the split-K scratch at the head of the workspace
  const uint8_t* reset; const float* u; const int32_t* forced; float *feat, *post; int32_t* idx;
  // Fused schedule (5 launches per step instead of 8) when the <= 64-row products qualify: the two LayerNorm+ELU stages
  // ride in the PROLOGUE of the product that consumes them (each workgroup recomputes the row statistics of its <= 64
  // rows from L2) and the straight-through sampler rides in the EPILOGUE of the posterior-logits product (one 32-logit
  // group per workgroup).  The post-LayerNorm activations `za` / `pin` that only the backward pass needs (weight
  // gradients, ELU') are then produced for ALL rows by two batched launches after the loop.
  bool fuse_ln, fuse_sample;

  // Decides the schedule and takes the optional buffers (PostWs) it wants; no launches.
  int plan(size_t ws_bytes) {
    const bool stacked = gk.L > 1;      // GRUCellStack with several layers: the unfused schedule, 3 launches per layer
    const bool normed = p[DM_RSSM_IN_G] != nullptr;      // layer_norm=False: all three norms are NoNorm (null parameters)
    DM_REQUIRE((p[DM_RSSM_POST_G] != nullptr) == normed && (p[DM_RSSM_PRIOR_G] != nullptr) == normed, DM_E_NULL,
               "rssm: the cell's three norms must be all LayerNorm or all NoNorm");
    fuse_ln = normed && !stacked && !gauss && dm_skinny_ln_ok(B, 3 * D, Hd) && dm_skinny_ln_ok(B, ZP, Hd) &&
              (ZP >= 64 * 1024 / Hd);
    fuse_sample = fuse_ln && C == 32 && (Z & 31) == 0 && (F & 3) == 0 && (D & 3) == 0 &&
                  (((uintptr_t)feat | (uintptr_t)a.zin) & 15) == 0;
    const bool want_wzt = !gauss && idx && T > 1 && dm_z_embed_ok(Hd);
    post_layout(DmArena(ws, ws_bytes), *this, want_wzt, fuse_sample && kind == 0 && B <= 64,
                normed && !stacked && !gauss && kind == 0 && want_wzt && idx && (F & 3) == 0 && T >= 3 && dm_rssm_lds_ok(B, D, Hd, S, C),
                this);
    return DM_OK;
  }

  // step t+1's masked inputs and reset flags: written / read by the kernels that produce h_t and z_t (null at the last step)
  float* hin_next(int t) const { return t + 1 < T ? a.hin + (size_t)(t + 1) * B * D : nullptr; }
  float* zin_next(int t) const { return t + 1 < T ? a.zin + (size_t)(t + 1) * B * Z : nullptr; }
  const uint8_t* reset_next(int t) const { return t + 1 < T ? reset + (size_t)(t + 1) * B : nullptr; }

  // x1 = z_mlp(z) + a_mlp(a) (rssm.py:138-139): the gather-sum from the indices step t-1 drew, else the product.
  // ln_z: the gather kernel owns complete rows, so it also writes za = ELU(in_norm(x1)) (rssm.py:140) and the statistics.
  int post_x1(int t, bool ln_z) const {
    const size_t r0 = (size_t)t * B;
    if (ln_z)
      return dm_z_embed_launch(B, Hd, S, C, idx + (r0 - B) * S, reset + r0, wzt, p[DM_RSSM_Z_B], a.ea + r0 * Hd, Hd, nullptr,
                               nullptr, a.x1 + r0 * Hd, Hd, nullptr, p[DM_RSSM_IN_G], p[DM_RSSM_IN_B], 1e-3f, a.za + r0 * Hd, Hd,
                               st, x1f, a.st1 + r0 * 2);
    if (wzt && t > 0)
      return dm_z_embed_launch(B, Hd, S, C, idx + (r0 - B) * S, reset + r0, wzt, p[DM_RSSM_Z_B], a.ea + r0 * Hd, Hd, nullptr,
                               nullptr, a.x1 + r0 * Hd, Hd, x1f, nullptr, nullptr, 0.f, nullptr, 0, st);
    DmGemm q = linear_q(B, Hd, Z, a.zin + r0 * Z, Z, p[DM_RSSM_Z_W], p[DM_RSSM_Z_B], a.ea + r0 * Hd, Hd, a.x1 + r0 * Hd, Hd);
    q.A_frag = zinf; q.C_frag = x1f;
    return dm_gemm_launch(q, ws, skb, st);
  }
  // h = GRUCell(za, h_in) (rssm.py:141), single layer: the two gate products in one launch, then the gates.
  // prologue: the first product reads x1 and applies in_norm + ELU itself (else za holds ELU(in_norm(x1)) already).
  int post_cell(int t, bool prologue) const {
    const size_t r0 = (size_t)t * B;
    const float* hin = a.hin + r0 * D;
    DmGemm gi_q = linear_q(B, 3 * D, Hd, (prologue ? a.x1 : a.za) + r0 * Hd, Hd, p[DM_RSSM_GRU_WIH], p[DM_RSSM_GRU_BIH], nullptr, 0,
                           a.gi + r0 * 3 * D, 3 * D);
    if (prologue) { gi_q.ln_g = p[DM_RSSM_IN_G]; gi_q.ln_b = p[DM_RSSM_IN_B]; gi_q.ln_eps = 1e-3f; }
    gi_q.A_frag = x1f;      // (fused schedule: the copy of whichever operand this form reads)
    DmGemm gh_q = linear_q(B, 3 * D, D, hin, D, p[DM_RSSM_GRU_WHH], p[DM_RSSM_GRU_BHH], nullptr, 0, a.gh + r0 * 3 * D, 3 * D);
    gh_q.A_frag = hinf;
    DM_TRY(dm_gemm_pair_launch(gi_q, gh_q, ws, skb, st));
    if (kind == 0)
      return dm_gru_gates_fwd_launch(B, D, a.gi + r0 * 3 * D, a.gh + r0 * 3 * D, hin, D, feat + r0 * F, F, hin_next(t),
                                     reset_next(t), hf, t + 1 < T ? hinf : nullptr, st);
    return dm_gru_norm_fwd_launch(kind, B, D, a.gi + r0 * 3 * D, a.gh + r0 * 3 * D, hin, D, gk.lng[0], gk.lnb[0], feat + r0 * F, F,
                                  a.gs + r0 * 3 * D, a.gst + r0 * 6, hin_next(t), reset_next(t), st);
  }
  // x2 = post_mlp_h(h) + post_mlp_e(embed)                                              rssm.py:143-144
  int post_x2(int t) const {
    const size_t r0 = (size_t)t * B;
    DmGemm q = linear_q(B, Hd, D, feat + r0 * F, F, p[DM_RSSM_POST_H_W], p[DM_RSSM_POST_H_B], a.ee + r0 * Hd, Hd, a.x2 + r0 * Hd, Hd);
    q.A_frag = hf; q.C_frag = x2f;
    return dm_gemm_launch(q, ws, skb, st);
  }
  // z ~ OneHotCategoricalStraightThrough(post) as its own launch                        rssm.py:147-148
  int post_sample(int t) const {
    const size_t r0 = (size_t)t * B;
    return dm_sample_onehot_launch(B, S, C, post + r0 * ZP, ZP, u ? u + r0 * S : nullptr, forced ? forced + r0 * S : nullptr,
                                   feat + r0 * F + D, F, idx ? idx + r0 * S : nullptr, zin_next(t), reset_next(t), st);
  }

  // 5 launches (one plain or LayerNorm cell, categorical latents, the three norms LayerNorm).
  int post_step_fused(int t) const {
    const size_t r0 = (size_t)t * B;
    // in_norm + ELU in the gather (the prologue form makes each of the gate product's 226 workgroups redo the LayerNorm + ELU
    // of the whole operand); the row-per-workgroup form holds <= 32 groups (stoch_dim 64 / 96 take the prologue)
    const bool ln_z = wzt && t > 0 && x1f && S <= 32;
    DM_TRY(post_x1(t, ln_z));
    DM_TRY(post_cell(t, !ln_z));
    DM_TRY(post_x2(t));
    // post = post_mlp(ELU(post_norm(x2))), LayerNorm in the prologue                             rssm.py:145-146
    DmGemm pq = linear_q(B, ZP, Hd, a.x2 + r0 * Hd, Hd, p[DM_RSSM_POST_W], p[DM_RSSM_POST_OB], nullptr, 0, post + r0 * ZP, ZP);
    pq.ln_g = p[DM_RSSM_POST_G]; pq.ln_b = p[DM_RSSM_POST_B]; pq.ln_eps = 1e-3f;
    pq.A_frag = x2f;
    if (!fuse_sample) {
      DM_TRY(dm_gemm_launch(pq, ws, skb, st));
      return post_sample(t);
    }
    DmSample sm;      // ... and z ~ OneHotCategoricalStraightThrough(post) in the epilogue        rssm.py:147-148
    sm.u = u ? u + r0 * S : nullptr; sm.forced = forced ? forced + r0 * S : nullptr;
    sm.onehot = feat + r0 * F + D; sm.ldo = F; sm.idx = idx ? idx + r0 * S : nullptr;
    sm.z_next = zin_next(t); sm.next_reset = reset_next(t); sm.z_next_frag = zinf;
    return dm_gemm_sample_launch(pq, sm, st);
  }
  // 8 launches (3 per layer for a cell stack): the reset masks of step t+1 are applied by the kernels that produce h_t and
  // z_t, and a single cell's two gate products share one launch.
  int post_step_plain(int t) const {
    const size_t r0 = (size_t)t * B;
    DM_TRY(post_x1(t, false));
    DM_TRY(norm_elu_fwd(B, Hd, a.x1 + r0 * Hd, Hd, p[DM_RSSM_IN_G], p[DM_RSSM_IN_B], 1e-3f, a.za + r0 * Hd, Hd, a.st1 + r0 * 2, st));
    if (gk.L > 1)
      DM_TRY(gru_stack_fwd(st, ws, skb, gk, B, Hd, D, a.za + r0 * Hd, a.hin + r0 * D, D, a.gi + r0 * 3 * D, a.gh + r0 * 3 * D,
                           feat + r0 * F, F, hin_next(t), reset_next(t), kind ? a.gs + r0 * 3 * D : nullptr,
                           kind ? a.gst + r0 * 6 * gk.L : nullptr));
    else
      DM_TRY(post_cell(t, false));
    DM_TRY(post_x2(t));
    // post = post_mlp(ELU(post_norm(x2)))                                                 rssm.py:145-146
    DM_TRY(norm_elu_fwd(B, Hd, a.x2 + r0 * Hd, Hd, p[DM_RSSM_POST_G], p[DM_RSSM_POST_B], 1e-3f, a.pin + r0 * Hd, Hd,
                        a.st2 + r0 * 2, st));
    DM_TRY(linear(st, ws, skb, B, ZP, Hd, a.pin + r0 * Hd, Hd, p[DM_RSSM_POST_W], p[DM_RSSM_POST_OB], nullptr, 0, post + r0 * ZP,
                  ZP));
    return post_sample(t);
  }
};

extern "C" int dm_rssm_sequence_fwd(const dm_shape* s, const float* embed, const float* action, const uint8_t* reset,
                                    const float* h0, const float* z0, const float* u, const int32_t* forced_idx,
                                    const dm_rssm_params* P, float* acts, float* feat, float* post, float* prior,
                                    int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(s && embed && action && reset && h0 && z0 && P && acts && feat && post && prior && ws, DM_E_NULL,
             "rssm_sequence_fwd: null pointer");
  DM_REQUIRE(u || forced_idx, DM_E_NULL, "rssm_sequence_fwd: need uniforms or forced indices");
  DmPrecisionScope prec(s->flags & DM_FLAG_BF16);
  DM_TRY(rssm_check(s));
  DM_REQUIRE(ws_bytes >= DM_SPLITK_FLOATS * sizeof(float), DM_E_WORKSPACE, "rssm_sequence_fwd: workspace too small");
  PostCtx c = {};
  rssm_dims(s, &c);
  rssm_carve(c, acts, &c.a);
  c.p = P->p; c.st = (hipStream_t)stream; c.ws = ws; c.skb = DM_SPLITK_FLOATS * sizeof(float);
  c.reset = reset; c.u = u; c.forced = forced_idx; c.feat = feat; c.post = post; c.idx = idx;
  DM_TRY(gru_stack(s, c.p, nullptr, &c.gk));
  DM_TRY(c.plan(ws_bytes));
  tl_last_schedule[0] = (c.fuse_ln ? DM_SCHED_FWD_FUSE_LN : 0) | (c.fuse_sample ? DM_SCHED_FWD_FUSE_SAMPLE : 0) |
                        (c.zinf ? DM_SCHED_FWD_FRAG : 0) | (c.wzt ? DM_SCHED_FWD_WZT : 0) | (c.psync ? DM_SCHED_FWD_PSYNC : 0);
  const RssmActs& a = c.a;
  const float* const* p = c.p;
  const int N = c.N, D = c.D, Hd = c.Hd, Z = c.Z, ZP = c.ZP;
  hipStream_t st = c.st;
  const size_t skb = c.skb;

  DM_TRY(linear(st, ws, skb, N, Hd, c.A, action, c.A, p[DM_RSSM_A_W], nullptr, nullptr, 0, a.ea, Hd));
  DM_TRY(linear(st, ws, skb, N, Hd, c.E, embed, c.E, p[DM_RSSM_POST_E_W], nullptr, nullptr, 0, a.ee, Hd));
  if (c.wzt) DM_TRY(transpose(st, p[DM_RSSM_Z_W], c.wzt, Hd, Z));
  // step 0's inputs: the caller's state under the first reset mask (every later step's are written by the step before it)
  DM_TRY(dm_mask_rows2_launch(c.B, D, h0, D, a.hin, D, Z, z0, Z, a.zin, Z, reset, st));
  if (c.zinf) {
    DM_TRY(dm_frag_pack_launch(c.B, D, a.hin, D, c.hinf, st));
    DM_TRY(dm_frag_pack_launch(c.B, Z, a.zin, Z, c.zinf, st));
  }
  const int t_launch_end = c.psync ? 1 : c.T;
  for (int t = 0; t < t_launch_end; ++t) DM_TRY(c.fuse_ln ? c.post_step_fused(t) : c.post_step_plain(t));
  if (c.psync) {
    DmRssmLds pq;
    pq.B = c.B; pq.D = D; pq.Hd = Hd; pq.S = c.S; pq.C = c.C; pq.F = c.F; pq.t_begin = 1; pq.t_end = c.T;
    pq.wzt = c.wzt; pq.zb = p[DM_RSSM_Z_B];
    pq.wih = p[DM_RSSM_GRU_WIH]; pq.bih = p[DM_RSSM_GRU_BIH]; pq.whh = p[DM_RSSM_GRU_WHH]; pq.bhh = p[DM_RSSM_GRU_BHH];
    pq.wph = p[DM_RSSM_POST_H_W]; pq.bph = p[DM_RSSM_POST_H_B]; pq.wpo = p[DM_RSSM_POST_W]; pq.bpo = p[DM_RSSM_POST_OB];
    pq.in_g = p[DM_RSSM_IN_G]; pq.in_b = p[DM_RSSM_IN_B]; pq.post_g = p[DM_RSSM_POST_G]; pq.post_b = p[DM_RSSM_POST_B];
    pq.ea = a.ea; pq.ee = a.ee; pq.reset = reset; pq.u = u; pq.forced = forced_idx;
    pq.x1 = a.x1; pq.gi = a.gi; pq.gh = a.gh; pq.hin = a.hin; pq.zin = a.zin; pq.feat = feat; pq.x2 = a.x2; pq.post = post;
    pq.idx = idx; pq.ws = c.psync; pq.ws_floats = c.psync_floats;
    DM_TRY(dm_rssm_lds_launch(pq, st));
  }
  if (c.fuse_ln || c.psync) {     // what only the backward pass reads: post-LayerNorm activations + statistics of every row
    DM_TRY(norm_elu_fwd(N, Hd, a.x1, Hd, p[DM_RSSM_IN_G], p[DM_RSSM_IN_B], 1e-3f, a.za, Hd, a.st1, st));
    DM_TRY(norm_elu_fwd(N, Hd, a.x2, Hd, p[DM_RSSM_POST_G], p[DM_RSSM_POST_B], 1e-3f, a.pin, Hd, a.st2, st));
  }
  // batch_prior over all (T*B) rows                                                    rssm.py:61,186-193
  DM_TRY(linear(st, ws, skb, N, Hd, D, feat, c.F, p[DM_RSSM_PRIOR_H_W], p[DM_RSSM_PRIOR_H_B], nullptr, 0, a.x3, Hd));
  DM_TRY(norm_elu_fwd(N, Hd, a.x3, Hd, p[DM_RSSM_PRIOR_G], p[DM_RSSM_PRIOR_B], 1e-3f, a.prin, Hd, a.st3, st));
  DM_TRY(linear(st, ws, skb, N, ZP, Hd, a.prin, Hd, p[DM_RSSM_PRIOR_W], p[DM_RSSM_PRIOR_OB], nullptr, 0, prior, ZP));
  return DM_OK;
}

// ---------------------------------------------------------------- BPTT --------------------------
// A/B switch of the BPTT launch schedule's folded LayerNorm backward (include/dreamer_hip.h dm_bptt_fold_enable)
static int g_bptt_fold = 1;
extern "C" int dm_bptt_fold_enable(int on) {
  const int was = g_bptt_fold;
  if (on >= 0) g_bptt_fold = on ? 1 : 0;
  return was;
}

// The backward's workspace: what every schedule needs (`must` floats), then the folded schedule's buffers and the fragment-major
// copies, each taken if wanted (BpttCtx::plan) and it fits - a small caller workspace keeps the prologue form / the row-major
// operands, the pointers null.  On an arena without a base it sizes.
struct BpttWs {
  float *sk, *sk_w;      // split-K scratch of the chain and of the parameter gradients' stream
  float *dprin, *dx3, *dpin, *dx2, *dgi, *dgh, *dza, *dx1;
  float *wt_post, *wt_post_h, *wt_ih, *wt_hh, *wt_z;      // W^T of the five backward-data products of a step
  float *dgl, *lnpg, *lnpb;      // LayerNorm GRU cells: gradients w.r.t. the LayerNorm outputs; column sums for their parameters
  // the side stream's own dx2 / dx1 (fused schedule: the LayerNorm backward of a chunk of rows is redone there instead of
  // being shared with the chain)
  float *dx2_w, *dx1_w;
  size_t must;
  // folded form: x2 W_post_h and x1 W_z for all rows, the weights' column sums, the per-strip row sums of g2 / g1
  float *xw2, *xwz, *cs2, *csz, *eps2, *eps1;
  // fragment-major copies (common.h dm_frag_off) of the two K = 3D operands of a step, dgi and dgh (written by the gates
  // backward epilogue, read by the two products that follow it), and of dpin, dza (written by the product that makes them)
  float *dgif, *dghf, *dpinf, *dzaf;
};
static size_t bptt_layout(DmArena ar, const RssmDims& d, bool want_fold, bool want_frag, BpttWs* w) {
  const size_t rows = d.N, D = d.D, Hd = d.Hd, Z = d.Z, ZP = d.ZP;
  *w = {};
  w->sk = ar.take(DM_SPLITK_FLOATS);
  w->dprin = ar.take(rows * Hd); w->dx3 = ar.take(rows * Hd); w->dpin = ar.take(rows * Hd); w->dx2 = ar.take(rows * Hd);
  w->dgi = ar.take(rows * 3 * D); w->dgh = ar.take(rows * 3 * D); w->dza = ar.take(rows * Hd); w->dx1 = ar.take(rows * Hd);
  w->wt_post = ar.take(ZP * Hd); w->wt_post_h = ar.take(Hd * D);
  w->wt_ih = ar.take(3 * D * Hd); w->wt_hh = ar.take(3 * D * D); w->wt_z = ar.take(Hd * Z);
  w->dgl = ar.take(d.kind ? rows * 3 * D : 0); w->lnpg = ar.take(d.kind ? 3 * D : 0); w->lnpb = ar.take(d.kind ? 3 * D : 0);
  w->sk_w = ar.take(DM_SPLITK_FLOATS); w->dx2_w = ar.take(rows * Hd); w->dx1_w = ar.take(rows * Hd);
  w->must = ar.off;
  if (want_fold) {
    const size_t mark = ar.off, nstrip = (Hd + 15) / 16;
    w->xw2 = ar.take(rows * D); w->xwz = ar.take(rows * Z); w->cs2 = ar.take(D); w->csz = ar.take(Z);
    w->eps2 = ar.take(nstrip * 128); w->eps1 = ar.take(nstrip * 128);
    if (!ar.fits()) { w->xw2 = w->xwz = w->cs2 = w->csz = w->eps2 = w->eps1 = nullptr; ar.give_back(mark); }
  }
  if (want_frag) {
    w->dgif = ar.take(dm_frag_floats(3 * d.D)); w->dghf = ar.take(dm_frag_floats(3 * d.D));
    w->dpinf = ar.take(dm_frag_floats(d.Hd)); w->dzaf = ar.take(dm_frag_floats(d.Hd));
    if (!ar.fits()) w->dgif = w->dghf = w->dpinf = w->dzaf = nullptr;
  }
  return ar.off;
}

struct BpttCtx : RssmDims, BpttWs {
  RssmActs a; GruStack gk;
  const float* const* p; float* const* g;
  // Parameter gradients are leaves of this pass: nothing reads them before the gradient clip.  They go to `sw` - the
  // library's weight-gradient side stream when the calling thread is armed (include/dreamer_hip.h dm_wgrad_side_arm), else
  // `st` itself - with a split-K scratch of their own.
  hipStream_t st, sw;
  size_t skb;
  const float *embed, *action, *feat, *post; const uint8_t* reset; float *dfeat, *dpost;
  const float *dx2s, *dx1s;      // whichever of dx2 / dx2_w (dx1 / dx1_w) the side stream reads
  // Fused schedule (5 launches per step instead of 8), mirror of the forward T loop: both LayerNorm+ELU BACKWARD stages
  // ride in the prologue of the <= 64-row product that consumes their result, and the GRU gates backward rides in the
  // epilogue of the product that completes dh'.  dx1 / dx2 (needed by the batched weight gradients) are then produced for
  // all rows by batched launches.
  bool fuse_b;
  // ... in FOLDED form (common.h DmGemm::eg_x): the product that makes dpin (dza) also turns it into g = dy ELU'(pre) gamma in
  // its epilogue - once, by the workgroup that owns the element, instead of once per consuming workgroup in a prologue - and
  // the consuming product is a plain one whose epilogue applies the two row-mean terms.  That needs x2 W_post_h and x1 W_z for
  // all rows (xw2, xwz: two batched products before the loop) and the weights' column sums (cs2, csz).
  // fold_sm (32 classes): step t-1's straight-through softmax backward rides in the epilogue of the product that completes its dz'.
  bool fold, fold_sm;
  int nstrip;
  // time chunks of the batched weight gradients (single-layer cells): chunk k = steps [T*k/nchunk, T*(k+1)/nchunk); the loop
  // runs t downwards, so the LAST chunk completes first - it overwrites the gradient, the others accumulate
  int nchunk, next_chunk;
  // The RSSM's weight gradients dW = dy^T x, in launch order: [0, 3) post_mlp, post_mlp_h, post_mlp_e; [3, 3 + 2L) W_ih, W_hh
  // of each cell layer (layer 0 reads za, layer i the new state of layer i-1); then z_mlp, a_mlp.
  struct Wgrad { const float* dy; int lddy, nout; const float* x; int ldx, kin; float* dW; } wg[3 + 2 * 4 + 2];
  int nwg;

  // Carves the workspace, decides the schedule and lists the weight gradients; no launches.
  int plan(void* ws, size_t ws_bytes) {
    const bool stacked = gk.L > 1;
    skb = DM_SPLITK_FLOATS * sizeof(float);
    // (the step's closing pair launch carries the LayerNorm backward on its second product: its first, dgh W_hh, must be on the
    // skinny kernel too - 3D x D over that kernel's 64K floor, i.e. deter_dim >= 148)
    fuse_b = p[DM_RSSM_IN_G] != nullptr && !stacked && !gauss && kind == 0 && dm_skinny_ln_ok(B, D, Hd) &&
             dm_skinny_ln_ok(B, Z, Hd) && (int64_t)3 * D * D >= (int64_t)64 * 1024 && (F & 3) == 0;
    fold = fuse_b && g_bptt_fold && B <= 64 && (int64_t)Hd * ZP >= (int64_t)64 * 1024 &&
           (int64_t)Hd * 3 * D >= (int64_t)64 * 1024 && (ZP & 3) == 0 && ((3 * D) & 3) == 0 && ZP >= 16;
    nstrip = (Hd + 15) / 16;
    bptt_layout(DmArena(ws, ws_bytes), *this, fold, fuse_b && B <= 64, this);
    DM_REQUIRE(must <= ws_bytes / sizeof(float), DM_E_WORKSPACE, "rssm_sequence_bwd: workspace too small (need %zu floats)", must);
    fold = fold && xw2;       // a small caller workspace keeps the prologue form
    fold_sm = fold && !gauss && C == 32 && Z == ZP;
    nchunk = (stacked || B < 16) ? 1 : (T >= 16 ? 4 : T >= 8 ? 2 : 1);      // (a few-column shard: the chunks' extra launches cost more than they hide)
    next_chunk = nchunk - 1;
    dx2s = fuse_b ? dx2_w : dx2;
    dx1s = fuse_b ? dx1_w : dx1;
    const int ls = gk.ls;
    int n = 0;
    wg[n++] = {dpost, ZP, ZP, a.pin, Hd, Hd, g[DM_RSSM_POST_W]};
    wg[n++] = {dx2s, Hd, Hd, feat, F, D, g[DM_RSSM_POST_H_W]};
    wg[n++] = {dx2s, Hd, Hd, embed, E, E, g[DM_RSSM_POST_E_W]};
    for (int i = 0; i < gk.L; ++i) {
      wg[n++] = {dgi + 3 * ls * i, 3 * D, 3 * ls, i == 0 ? a.za : feat + (size_t)(i - 1) * ls, i == 0 ? Hd : F, i == 0 ? Hd : ls,
                 gk.g_wih[i]};
      wg[n++] = {dgh + 3 * ls * i, 3 * D, 3 * ls, a.hin + i * ls, D, ls, gk.g_whh[i]};
    }
    wg[n++] = {dx1s, Hd, Hd, a.zin, Z, Z, g[DM_RSSM_Z_W]};
    wg[n++] = {dx1s, Hd, Hd, action, A, A, g[DM_RSSM_A_W]};
    nwg = n;
    return DM_OK;
  }
  // entries [first, first + count) of the list over rows [c0, c0 + rows), on the side stream
  int wgrads(int first, int count, size_t c0, int rows, int accum) const {
    for (const Wgrad* w = wg + first; w < wg + first + count; ++w)
      DM_TRY(wgrad(sw, sk_w, skb, rows, w->nout, w->kin, w->dy + c0 * w->lddy, w->lddy, w->x + c0 * w->ldx, w->ldx, w->dW, accum));
    return DM_OK;
  }
  // Single-layer cells: the weight gradients of a time chunk, launched as soon as the loop has finished the chunk's rows, so
  // they run BESIDE the loop (a B-row latency chain that leaves most CUs idle) instead of behind it.  The chunk boundaries,
  // and with them every sum, are the same whether or not a side stream is used.
  int side_chunk(int t) {
    if (gk.L > 1 || next_chunk < 0 || t != (int)((long long)T * next_chunk / nchunk)) return DM_OK;
    const int k = next_chunk--;
    const int t0 = (int)((long long)T * k / nchunk), t1 = (int)((long long)T * (k + 1) / nchunk);
    const size_t c0 = (size_t)t0 * B;
    const int rows = (t1 - t0) * B;
    DM_TRY(dm_wgrad_side_fork(st, sw));            // rows [c0, c0 + rows) of dpost, dpin, dgi, dgh, dza (dx2, dx1) are final
    if (fuse_b) {
      DM_TRY(post_norm_bwd(c0, rows, dx2_w, sw));
      DM_TRY(in_norm_bwd(c0, rows, dx1_w, sw));
    }
    return wgrads(0, nwg, c0, rows, k != nchunk - 1);
  }
  // dx2 / dx1 = the post_norm / in_norm + ELU backward of dpin / dza, rows [c0, c0 + rows)
  int post_norm_bwd(size_t c0, int rows, float* dx, hipStream_t s) const {
    return norm_elu_bwd_dx(rows, Hd, a.x2 + c0 * Hd, Hd, a.pin + c0 * Hd, Hd, a.st2 + c0 * 2, p[DM_RSSM_POST_G], dpin + c0 * Hd, Hd,
                           dx + c0 * Hd, Hd, s);
  }
  int in_norm_bwd(size_t c0, int rows, float* dx, hipStream_t s) const {
    return norm_elu_bwd_dx(rows, Hd, a.x1 + c0 * Hd, Hd, a.za + c0 * Hd, Hd, a.st1 + c0 * 2, p[DM_RSSM_IN_G], dza + c0 * Hd, Hd,
                           dx + c0 * Hd, Hd, s);
  }

  // Step t: [dh' | dz'] of step t (complete when the step starts), its dpost rows, step t-1's [dh' | dz'] (null at t = 0)
  struct Rows { size_t r0; float *dft, *dpt, *dprev; const uint8_t* rz; };
  Rows rows_of(int t) const {
    const size_t r0 = (size_t)t * B;
    return {r0, dfeat + r0 * F, dpost + r0 * ZP, t > 0 ? dfeat + (r0 - B) * F : nullptr, reset + r0};
  }
  // dprev[:, :D] += mask * dgh W_hh: the first product of the pair launch that closes a single-layer step
  DmGemm dprev_h(const Rows& r) const {
    DmGemm q = dgrad_t_q(B, 3 * D, D, dgh + r.r0 * 3 * D, 3 * D, wt_hh, r.dprev, F, 1, r.rz);
    q.A_frag = dghf;
    return q;
  }
  // One LayerNorm+ELU stage of step t as the fused schedule's products see it.
  struct Ln {
    const float *x, *stats, *gamma, *beta;      // pre-activations, (mean, rstd), parameters
    float *dy, *gx, *frag, *ps;                 // gradient w.r.t. the output; folded: gx = dy ELU'(pre) gamma and its per-strip row sums; frag: copy of dy (folded: of gx)
    const float *xw, *cs; int ldxw;             // folded: x W of these rows and W's column sums, W = the consuming product's weight
  };
  // C = dy of the stage = A Wt^T (K = lda = ldb).  Prologue form: + its fragment-major copy; folded: + gx and its row sums.
  DmGemm make_dy(const Ln& n, bool folded, int K, const float* A_, const float* A_frag, const float* Wt) const {
    DmGemm q = dgrad_t_q(B, K, Hd, A_, K, Wt, n.dy, Hd, 0, nullptr);
    q.A_frag = A_frag;
    if (folded) {
      q.eg_x = n.x; q.eg_ldx = Hd; q.eg_stats = n.stats; q.eg_gamma = n.gamma; q.eg_beta = n.beta;
      q.eg_G = n.gx; q.eg_ldg = Hd; q.eg_Gf = n.frag; q.eg_ps = n.ps;
    } else {
      q.C_frag = n.frag;
    }
    return q;
  }
  // C_ (ldc = F) += mask * dx Wt^T, dx = the gradient w.r.t. the stage's input.  Prologue form: A = dy, the LayerNorm+ELU
  // backward in the prologue; folded: a plain product on gx whose epilogue applies the two row-mean terms.
  DmGemm use_dx(const Ln& n, bool folded, int N_, const float* Wt, float* C_, const uint8_t* rz) const {
    DmGemm q = dgrad_t_q(B, Hd, N_, folded ? n.gx : n.dy, Hd, Wt, C_, F, 1, rz);
    q.A_frag = n.frag;
    if (folded) {
      q.lnf_ps = n.ps; q.lnf_nps = nstrip; q.lnf_stats = n.stats; q.lnf_xw = n.xw; q.lnf_ldxw = n.ldxw; q.lnf_cs = n.cs;
    } else {
      q.ln_g = n.gamma; q.ln_b = n.beta; q.lnb_x = n.x; q.lnb_ldx = Hd; q.lnb_stats = n.stats;
    }
    return q;
  }

  // 4 launches: dpin, dh' + gates backward, dza, the dprev pair - and the sample backward in front, unless fold_sm has moved it
  // into the pair of step t+1.
  int bptt_step_fused(int t) const {
    const Rows r = rows_of(t);
    const size_t r0 = r.r0;
    const Ln post_n = {a.x2 + r0 * Hd, a.st2 + r0 * 2, p[DM_RSSM_POST_G], p[DM_RSSM_POST_B], dpin + r0 * Hd, dx2 + r0 * Hd, dpinf,
                       eps2, fold ? xw2 + r0 * D : nullptr, cs2, D};
    const Ln in_n = {a.x1 + r0 * Hd, a.st1 + r0 * 2, p[DM_RSSM_IN_G], p[DM_RSSM_IN_B], dza + r0 * Hd, dx1 + r0 * Hd, dzaf,
                     eps1, fold ? xwz + r0 * Z : nullptr, csz, Z};
    // straight-through sample: dpost += softmax'(post)^T dz'   (fold_sm: done by the pair launch of step t+1)
    if (!(fold_sm && t < T - 1)) DM_TRY(dm_st_softmax_bwd_launch(B, S, C, post + r0 * ZP, ZP, r.dft + D, F, r.dpt, ZP, 1, st));
    // dpin = dpost Wpost   (folded: g2 goes row-major into the dx2 rows - re-made in batch after the loop - and fragment-major)
    DM_TRY(dm_gemm_launch(make_dy(post_n, fold, ZP, r.dpt, nullptr, wt_post), sk, skb, st));
    // dh' += LNbwd(dpin) Wph ; then the GRU gates backward on the completed dh' (the direct path dh'*u goes, masked, into dprev)
    DmGatesBwd gb;
    gb.gi = a.gi + r0 * 3 * D; gb.gh = a.gh + r0 * 3 * D; gb.h_in = a.hin + r0 * D; gb.ldh = D; gb.D = D;
    gb.dgi = dgi + r0 * 3 * D; gb.dgh = dgh + r0 * 3 * D; gb.dprev = r.dprev; gb.ldp = F; gb.row_zero = r.rz;
    gb.dgi_frag = dgif; gb.dgh_frag = dghf;
    DmGemm q4 = use_dx(post_n, fold, D, wt_post_h, r.dft, nullptr);
    q4.gates = &gb;
    DM_TRY(dm_gemm_launch(q4, sk, skb, st));
    // dza = dgi Wih
    DM_TRY(dm_gemm_launch(make_dy(in_n, fold, 3 * D, dgi + r0 * 3 * D, dgif, wt_ih), sk, skb, st));
    if (t == 0) return DM_OK;
    // both products into step t-1's [dh' | dz']; the second one consumes LNbwd(dza)
    DmGemm qz = use_dx(in_n, fold, Z, wt_z, r.dprev + D, r.rz);
    if (fold_sm) { qz.sm_logits = post + (r0 - B) * ZP; qz.sm_ld = ZP; qz.sm_dlogits = dpost + (r0 - B) * ZP; qz.sm_ldd = ZP; }
    return dm_gemm_pair_launch(dprev_h(r), qz, sk, skb, st);
  }

  // The head of an unfused step (4 launches): sample backward, post_mlp, post_norm+ELU, post_mlp_h.
  int post_branch(const Rows& r) const {
    const size_t r0 = r.r0;
    // straight-through sample: dpost += softmax'(post)^T dz'   (Gaussian: the reparameterised sample's (dmean, draw std))
    if (gauss) DM_TRY(dm_gauss_sample_bwd_launch(B, S, post + r0 * ZP, ZP, feat + r0 * F + D, F, r.dft + D, F, r.dpt, ZP, 1, st));
    else DM_TRY(dm_st_softmax_bwd_launch(B, S, C, post + r0 * ZP, ZP, r.dft + D, F, r.dpt, ZP, 1, st));
    DM_TRY(dgrad_t(st, sk, skb, B, ZP, Hd, r.dpt, ZP, wt_post, dpin + r0 * Hd, Hd, 0, nullptr));
    DM_TRY(post_norm_bwd(r0, B, dx2, st));
    return dgrad_t(st, sk, skb, B, Hd, D, dx2 + r0 * Hd, Hd, wt_post_h, r.dft, F, 1, nullptr);
  }
  // 8 launches: the head, the gates (the direct path dh'*u goes, masked, straight into step t-1's dh'), dza, in_norm, the pair.
  int bptt_step_single(int t) const {
    const Rows r = rows_of(t);
    const size_t r0 = r.r0;
    DM_TRY(post_branch(r));
    if (kind == 0)
      DM_TRY(dm_gru_gates_bwd_launch(B, D, a.gi + r0 * 3 * D, a.gh + r0 * 3 * D, a.hin + r0 * D, D, r.dft, F, dgi + r0 * 3 * D,
                                     dgh + r0 * 3 * D, r.dprev, F, 1, r.rz, st));
    else
      DM_TRY(dm_gru_norm_bwd_launch(kind, B, D, a.gh + r0 * 3 * D, a.hin + r0 * D, D, a.gs + r0 * 3 * D, a.gst + r0 * 6, gk.lng[0],
                                    gk.lnb[0], r.dft, F, dgi + r0 * 3 * D, dgh + r0 * 3 * D, dgl + r0 * 3 * D, r.dprev, F, r.rz, st));
    DM_TRY(dgrad_t(st, sk, skb, B, 3 * D, Hd, dgi + r0 * 3 * D, 3 * D, wt_ih, dza + r0 * Hd, Hd, 0, nullptr));
    DM_TRY(in_norm_bwd(r0, B, dx1, st));
    if (t == 0) return DM_OK;
    // both products into step t-1's [dh' | dz'], one launch
    return dm_gemm_pair_launch(dprev_h(r), dgrad_t_q(B, Hd, Z, dx1 + r0 * Hd, Hd, wt_z, r.dprev + D, F, 1, r.rz), sk, skb, st);
  }
  // The head, then the layers in reverse: layer i's input gradient lands in the new-state gradient of layer i-1 before that
  // layer's own gates run; its recurrent-input gradient goes (masked) into step t-1's dh' slice.
  int bptt_step_stacked(int t) const {
    const Rows r = rows_of(t);
    const size_t r0 = r.r0;
    const int ls = gk.ls;
    float* dprev = r.dprev;
    DM_TRY(post_branch(r));
    for (int i = gk.L - 1; i >= 0; --i) {
      float* dgi_i = dgi + r0 * 3 * D + 3 * ls * i;
      float* dgh_i = dgh + r0 * 3 * D + 3 * ls * i;
      if (kind == 0)
        DM_TRY(dm_gru_gates_bwd_launch(B, ls, a.gi + r0 * 3 * D + 3 * ls * i, a.gh + r0 * 3 * D + 3 * ls * i,
                                       a.hin + r0 * D + i * ls, D, r.dft + i * ls, F, dgi_i, dgh_i,
                                       dprev ? dprev + i * ls : nullptr, F, 1, r.rz, st, 3 * D));
      else
        DM_TRY(dm_gru_norm_bwd_launch(kind, B, ls, a.gh + r0 * 3 * D + 3 * ls * i, a.hin + r0 * D + i * ls, D,
                                      a.gs + r0 * 3 * D + 3 * ls * i, a.gst + r0 * 6 * gk.L + 6 * i, gk.lng[i], gk.lnb[i],
                                      r.dft + i * ls, F, dgi_i, dgh_i, dgl + r0 * 3 * D + 3 * ls * i,
                                      dprev ? dprev + i * ls : nullptr, F, r.rz, st, 3 * D, 6 * gk.L));
      if (i > 0) DM_TRY(dgrad(st, sk, skb, B, 3 * ls, ls, dgi_i, 3 * D, gk.wih[i], r.dft + (i - 1) * ls, F, 1, nullptr));
      else DM_TRY(dgrad(st, sk, skb, B, 3 * ls, Hd, dgi_i, 3 * D, gk.wih[0], dza + r0 * Hd, Hd, 0, nullptr));
      if (dprev) DM_TRY(dgrad(st, sk, skb, B, 3 * ls, ls, dgh_i, 3 * D, gk.whh[i], dprev + i * ls, F, 1, r.rz));
    }
    DM_TRY(in_norm_bwd(r0, B, dx1, st));
    if (dprev) DM_TRY(dgrad_t(st, sk, skb, B, Hd, Z, dx1 + r0 * Hd, Hd, wt_z, dprev + D, F, 1, r.rz));
    return DM_OK;
  }

  // Gate-bias (nn.GRUCell) or LayerNorm-parameter (the LayerNorm cells) gradients of cell layer i: column passes over the
  // layer's 3*ls gate columns of all rows; the latter are then split into the cell's (reset, update, newval) parameter slots.
  int cell_param_grads(int i) const {
    const int ls = gk.ls;
    if (kind == 0) {
      DM_TRY(dm_colsum_launch(N, 3 * ls, dgi + 3 * ls * i, 3 * D, gk.g_bih[i], sk_w, skb, sw));
      return dm_colsum_launch(N, 3 * ls, dgh + 3 * ls * i, 3 * D, gk.g_bhh[i], sk_w, skb, sw);
    }
    DM_TRY(dm_gru_norm_param_grads_launch(kind, N, ls, a.gs + 3 * ls * i, a.gst + 6 * i, dgl + 3 * ls * i, lnpg, lnpb, sw, 3 * D,
                                          6 * gk.L));
    const int parts = kind == 1 ? 3 : 1;
    const size_t len = (size_t)(kind == 1 ? ls : 3 * ls) * sizeof(float);
    for (int q = 0; q < parts; ++q)
      if (hipMemcpyAsync(gk.g_lng[i][q], lnpg + (size_t)q * ls, len, hipMemcpyDeviceToDevice, sw) != hipSuccess ||
          hipMemcpyAsync(gk.g_lnb[i][q], lnpb + (size_t)q * ls, len, hipMemcpyDeviceToDevice, sw) != hipSuccess)
        return dm_fail(DM_E_HIP, "rssm_sequence_bwd: gradient copy failed");
    return DM_OK;
  }
  // Bias / LayerNorm-parameter gradients (column passes over all rows) and, for cell stacks, the weight gradients: on sw.
  int param_tail() const {
    const int L = gk.L;
    const bool stacked = L > 1;
    if (stacked) DM_TRY(dm_wgrad_side_fork(st, sw));      // (single-layer cells forked at their last chunk)
    DM_TRY(dm_colsum_launch(N, ZP, dpost, ZP, g[DM_RSSM_POST_OB], sk_w, skb, sw));
    DM_TRY(norm_elu_bwd_params(N, Hd, a.x2, Hd, a.pin, Hd, a.st2, dpin, Hd, g[DM_RSSM_POST_G], g[DM_RSSM_POST_B], sk_w, skb, sw));
    DM_TRY(dm_colsum_launch(N, Hd, dx2s, Hd, g[DM_RSSM_POST_H_B], sk_w, skb, sw));
    if (stacked) DM_TRY(wgrads(0, 3, 0, N, 0));
    for (int i = 0; i < L; ++i) {
      if (stacked) DM_TRY(wgrads(3 + 2 * i, 2, 0, N, 0));
      DM_TRY(cell_param_grads(i));
    }
    DM_TRY(norm_elu_bwd_params(N, Hd, a.x1, Hd, a.za, Hd, a.st1, dza, Hd, g[DM_RSSM_IN_G], g[DM_RSSM_IN_B], sk_w, skb, sw));
    DM_TRY(dm_colsum_launch(N, Hd, dx1s, Hd, g[DM_RSSM_Z_B], sk_w, skb, sw));
    if (stacked) DM_TRY(wgrads(3 + 2 * L, 2, 0, N, 0));
    return dm_wgrad_side_mark(sw, st);
  }
};

extern "C" int dm_rssm_sequence_bwd(const dm_shape* s, const float* embed, const float* action, const uint8_t* reset,
                                    const dm_rssm_params* P, const float* acts, const float* feat, const float* post,
                                    float* dfeat, float* dpost, float* dprior, const dm_rssm_grads* G, float* dembed,
                                    void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(s && embed && action && reset && P && acts && feat && post && dfeat && dpost && dprior && G && ws, DM_E_NULL,
             "rssm_sequence_bwd: null pointer");
  DmPrecisionScope prec(s->flags & DM_FLAG_BF16);
  DM_TRY(rssm_check(s));
  BpttCtx c = {};
  rssm_dims(s, &c);
  rssm_carve(c, const_cast<float*>(acts), &c.a);
  c.p = P->p; c.g = G->p; c.st = (hipStream_t)stream; c.sw = dm_wgrad_side_stream(c.st);
  c.embed = embed; c.action = action; c.feat = feat; c.post = post; c.reset = reset; c.dfeat = dfeat; c.dpost = dpost;
  DM_TRY(gru_stack(s, c.p, c.g, &c.gk));
  DM_TRY(c.plan(ws, ws_bytes));
  tl_last_schedule[1] = (c.fuse_b ? DM_SCHED_BWD_FUSE_B : 0) | (c.fold ? DM_SCHED_BWD_FOLD : 0) | (c.fold_sm ? DM_SCHED_BWD_FOLD_SM : 0) |
                        (c.dgif ? DM_SCHED_BWD_FRAG : 0) | (c.nchunk << DM_SCHED_BWD_NCHUNK_SHIFT);
  const RssmActs& a = c.a;
  const float* const* p = c.p;
  float* const* g = c.g;
  const int N = c.N, D = c.D, Hd = c.Hd, Z = c.Z, ZP = c.ZP, F = c.F;
  hipStream_t st = c.st, sw = c.sw;
  float *sk = c.sk, *sk_w = c.sk_w;
  const size_t skb = c.skb;

  // ---- prior branch, batched over all rows: the data gradient on st ...
  DM_TRY(dgrad(st, sk, skb, N, ZP, Hd, dprior, ZP, p[DM_RSSM_PRIOR_W], c.dprin, Hd, 0, nullptr));
  DM_TRY(norm_elu_bwd_dx(N, Hd, a.x3, Hd, a.prin, Hd, a.st3, p[DM_RSSM_PRIOR_G], c.dprin, Hd, c.dx3, Hd, st));
  DM_TRY(dgrad(st, sk, skb, N, Hd, D, c.dx3, Hd, p[DM_RSSM_PRIOR_H_W], dfeat, F, 1, nullptr));
  // ... its parameter gradients on sw
  DM_TRY(dm_wgrad_side_fork(st, sw));
  DM_TRY(wgrad(sw, sk_w, skb, N, ZP, Hd, dprior, ZP, a.prin, Hd, g[DM_RSSM_PRIOR_W]));
  DM_TRY(dm_colsum_launch(N, ZP, dprior, ZP, g[DM_RSSM_PRIOR_OB], sk_w, skb, sw));
  DM_TRY(norm_elu_bwd_params(N, Hd, a.x3, Hd, a.prin, Hd, a.st3, c.dprin, Hd, g[DM_RSSM_PRIOR_G], g[DM_RSSM_PRIOR_B], sk_w, skb, sw));
  DM_TRY(wgrad(sw, sk_w, skb, N, Hd, D, c.dx3, Hd, feat, F, g[DM_RSSM_PRIOR_H_W]));
  DM_TRY(dm_colsum_launch(N, Hd, c.dx3, Hd, g[DM_RSSM_PRIOR_H_B], sk_w, skb, sw));

  // ---- BPTT as launches.  The five backward-data products of a step multiply a B-row block by W (not W^T); transposing the
  // weights once here (22 MB, ~20 us) lets all 5*T of them stream k-contiguous rows.  (The loop as a persistent
  // LDS-weight-stationary kernel is 1.6x faster alone and slower INSIDE the multi-stream step, because it needs every CU at
  // once while the decoder backward wants them too: profiles/r04_ab_bptt.txt.)
  DM_TRY(transpose(st, p[DM_RSSM_POST_W], c.wt_post, ZP, Hd));
  DM_TRY(transpose(st, p[DM_RSSM_POST_H_W], c.wt_post_h, Hd, D));
  if (c.gk.L == 1) {
    DM_TRY(transpose(st, p[DM_RSSM_GRU_WIH], c.wt_ih, 3 * D, Hd));
    DM_TRY(transpose(st, p[DM_RSSM_GRU_WHH], c.wt_hh, 3 * D, D));
  }
  DM_TRY(transpose(st, p[DM_RSSM_Z_W], c.wt_z, Hd, Z));
  if (c.fold) {
    DM_TRY(dgrad(st, sk, skb, N, Hd, D, a.x2, Hd, p[DM_RSSM_POST_H_W], c.xw2, D, 0, nullptr));      // x2 W_post_h
    DM_TRY(dgrad(st, sk, skb, N, Hd, Z, a.x1, Hd, p[DM_RSSM_Z_W], c.xwz, Z, 0, nullptr));           // x1 W_z
    DM_TRY(dm_colsum_launch(Hd, D, p[DM_RSSM_POST_H_W], D, c.cs2, sk, skb, st));
    DM_TRY(dm_colsum_launch(Hd, Z, p[DM_RSSM_Z_W], Z, c.csz, sk, skb, st));
  }
  for (int t = c.T - 1; t >= 0; --t) {
    DM_TRY(c.fuse_b ? c.bptt_step_fused(t) : c.gk.L > 1 ? c.bptt_step_stacked(t) : c.bptt_step_single(t));
    DM_TRY(c.side_chunk(t));
  }
  // ---- the one data gradient left: dembed, for the encoder backward that follows on st
  if (c.fuse_b) DM_TRY(c.post_norm_bwd(0, N, c.dx2, st));
  if (dembed) DM_TRY(dgrad(st, sk, skb, N, Hd, c.E, c.dx2, Hd, p[DM_RSSM_POST_E_W], dembed, c.E, 0, nullptr));
  return c.param_tail();
}

// ---------------------------------------------------------------- imagination -------------------
// Progress marks of the NEXT dm_dream_rollout call of this thread (include/dreamer_hip.h): events[i] is recorded on the
// rollout's stream once horizon step steps[i] has been enqueued, i.e. when feature rows [0, (steps[i] + 2) * M) are final.
static thread_local int tl_marks_n = 0;
static thread_local int tl_mark_step[4];
static thread_local hipEvent_t tl_mark_ev[4];
extern "C" int dm_dream_rollout_marks(int n, const int* steps, void* const* events) {
  DM_REQUIRE(n >= 0 && n <= 4 && (n == 0 || (steps && events)), DM_E_SHAPE, "dream_rollout_marks: n=%d (0..4)", n);
  for (int i = 0; i < n; ++i) {
    DM_REQUIRE(events[i], DM_E_NULL, "dream_rollout_marks: null event %d", i);
    tl_mark_step[i] = steps[i];
    tl_mark_ev[i] = (hipEvent_t)events[i];
  }
  tl_marks_n = n;
  return DM_OK;
}
// every mark not recorded inside the loop (step out of range, or the chain ran as a captured / replayed graph) is recorded
// behind the whole call, so a waiter is never left with a stale event
struct DmRolloutMarks {
  int n;
  bool done[4] = {false, false, false, false};
  hipStream_t caller;
  explicit DmRolloutMarks(hipStream_t st) : n(tl_marks_n), caller(st) { tl_marks_n = 0; }
  void at_step(int i, hipStream_t st, bool eager) {
    if (!eager) return;
    for (int k = 0; k < n; ++k)
      if (!done[k] && tl_mark_step[k] == i) { (void)hipEventRecord(tl_mark_ev[k], st); done[k] = true; }
  }
  ~DmRolloutMarks() {
    for (int k = 0; k < n; ++k)
      if (!done[k]) (void)hipEventRecord(tl_mark_ev[k], caller);
  }
};

static int g_rollout_fuse_act = 1;
// 1 / 0: the rollout's one-hot action draw in the output stage of the whole-MLP actor kernel / as its own launch; -1 queries.
extern "C" int dm_rollout_fuse_act_enable(int on) {
  if (on >= 0) g_rollout_fuse_act = on ? 1 : 0;
  return g_rollout_fuse_act;
}

struct RolloutDims : RssmDims {
  int M, H, Hm, L, adist, AO;      // rows, horizon; the actor MLP's width and depth, its distribution (0 onehot, 1 tanh_normal, 2 normal_tanh) and output width (a2c.py:35)
};
// The rollout's workspace: what every schedule needs (`must` floats; keep_acts: the caller keeps the actor's activations and
// outputs, tw_on: the bf16 twins), then three optional blocks, each taken if wanted (RolloutCtx::plan) and it fits - the
// product path needs none of them, their pointers stay null.  On an arena without a base it sizes.
struct RolloutWs {
  float *sk, *macts, *logits_ws, *ea, *x1, *za, *stats, *gi, *gh, *prior, *gsw, *gstw;
  // bf16 mode, plain single-layer GRU with LayerNorm: the cell's four 2 500-row products read bf16 twins (common.h DmTwinScope) -
  // per-call copies of their weights, za (written by the z_embed / LayerNorm kernels that produce it) and the h columns of
  // `feats` (written by the gates kernel; one range per step, so step 0's h, copied from `start`, stays on the fp32 path)
  unsigned short *wih_h, *whh_h, *wph_h, *wp_h, *za_h, *feats_h;
  size_t must;
  // steps 1.. of the rollout read the z the prior sampler of the step before drew (pidx): z_mlp + in_norm + ELU become one
  // gather-sum launch over z_mlp^T (dm_z_embed_launch) instead of a (M x Hd x Z) product and a LayerNorm launch; with one-hot
  // actions a_mlp(action) is a row of a_mlp^T too (wat; aidx: scratch for the action's index if the caller wants none)
  float *wzt, *wat; int32_t *pidx, *aidx;
  // the actor's weights, fragment-major for the whole-MLP kernel: packed once for all H steps.  The actor's first layer
  // sees [h | one-hot z]: its z columns are a gathered sum of W0^T rows into actor_add0 (indices from the prior sampler;
  // step 0's z is a dense vector: its non-zeros are found by ballot), the MFMA product runs over h only.  Needs pidx.
  float *actor_wpack, *actor_w0t, *actor_add0;
};
static size_t rollout_layout(DmArena ar, const RolloutDims& d, bool keep_acts, bool tw_on, bool want_z, bool want_pack,
                             bool want_add0, RolloutWs* w) {
  const size_t M = d.M, D = d.D, Hd = d.Hd, ZP = d.ZP, F = d.F;
  *w = {};
  w->sk = ar.take(DM_SPLITK_FLOATS);
  w->macts = ar.take(keep_acts ? 0 : dm_mlp_acts_floats(d.M, d.Hm, d.L)); w->logits_ws = ar.take(keep_acts ? 0 : M * d.AO);
  w->ea = ar.take(M * Hd); w->x1 = ar.take(M * Hd); w->za = ar.take(M * Hd); w->stats = ar.take(M * 2);
  w->gi = ar.take(M * 3 * D); w->gh = ar.take(M * 3 * D); w->prior = ar.take(M * ZP);
  w->gsw = ar.take(d.kind ? M * 3 * D : 0); w->gstw = ar.take(d.kind ? M * 6 * d.layers : 0);
  w->wih_h = (unsigned short*)ar.take(tw_on ? dm_half_floats(3 * D * Hd) : 0);
  w->whh_h = (unsigned short*)ar.take(tw_on ? dm_half_floats(3 * D * D) : 0);
  w->wph_h = (unsigned short*)ar.take(tw_on ? dm_half_floats(Hd * D) : 0);
  w->wp_h = (unsigned short*)ar.take(tw_on ? dm_half_floats(ZP * Hd) : 0);
  w->za_h = (unsigned short*)ar.take(tw_on ? dm_half_floats(M * Hd) : 0);
  w->feats_h = (unsigned short*)ar.take(tw_on ? dm_half_floats((size_t)(d.H + 1) * M * F) : 0);
  w->must = ar.off;
  if (want_z) {
    const size_t mark = ar.off;
    w->wzt = ar.take((size_t)d.Z * Hd);
    w->wat = ar.take((size_t)d.A * Hd);
    w->pidx = reinterpret_cast<int32_t*>(ar.take(M * d.S));
    w->aidx = reinterpret_cast<int32_t*>(ar.take(M));
    want_z = ar.fits();
    if (!want_z) { w->wzt = nullptr; w->pidx = nullptr; ar.give_back(mark); }
    if (!want_z || d.adist != 0) { w->wat = nullptr; w->aidx = nullptr; }
  }
  if (want_pack) {
    w->actor_wpack = ar.take(dm_mlp_chain_pack_floats(d.F, d.L));
    if (ar.fits() && want_z && want_add0) {
      const size_t mark = ar.off;
      w->actor_w0t = ar.take(F * d.Hm);
      w->actor_add0 = ar.take(M * d.Hm);
      if (!ar.fits()) { w->actor_w0t = w->actor_add0 = nullptr; ar.give_back(mark); }
    }
  }
  return ar.off;
}

struct RolloutCtx : RolloutDims, RolloutWs {
  GruStack gk;
  const float* const* p; const dm_mlp_params* actor; hipStream_t st; size_t skb;
  const float *u_act, *u_prior; float *feats, *actions; int32_t* act_idx; float *actor_acts, *actor_logits;
  bool tw_on;
  // one-hot actors on the whole-MLP kernel: the action draw rides in that kernel's output stage (dm_rollout_fuse_act_enable(0)
  // keeps the stand-alone sampler launch - same rule, same operation order, bit-identical draws)
  bool fuse_act;

  // Decides the schedule and takes the workspace (RolloutWs) with the optional buffers it wants; no launches.
  int plan(void* ws, size_t ws_bytes) {
    tw_on = dm_twins_on() && kind == 0 && layers == 1 && p[DM_RSSM_IN_G] && p[DM_RSSM_PRIOR_G] && (F & 7) == 0;
    skb = DM_SPLITK_FLOATS * sizeof(float);
    // the actor's call as every step issues it: mlp.hip's plan says whether it runs on the whole-MLP kernel (weights packed once
    // for all H steps) and whether that kernel then takes the z columns' contribution from here
    const bool chain = dm_mlp_fwd_path(actor_call(0)) == DM_MLP_CHAIN;
    rollout_layout(DmArena(ws, ws_bytes), *this, actor_acts != nullptr, tw_on, C != 0 && H > 1 && dm_z_embed_ok(Hd), chain,
                   C != 0 && dm_z_embed_ok(Hm), this);
    DM_REQUIRE(must <= ws_bytes / sizeof(float), DM_E_WORKSPACE, "dream_rollout: workspace too small (need %zu floats)", must);
    if (actor_add0) {
      int k0 = F;
      dm_mlp_fwd_path(actor_call(0), &k0);
      if (k0 == F) actor_w0t = actor_add0 = nullptr;
    }
    fuse_act = adist == 0 && actor_wpack && g_rollout_fuse_act;
    return DM_OK;
  }

  // the sampled action's index of step i (scratch if the caller wants none; null when there is neither)
  int32_t* act_idx_of(int i) const { return act_idx ? act_idx + (size_t)i * M : aidx; }

  // the actor's forward of step i, without the fused sampler
  DmMlpFwd actor_call(int i) const {
    const bool keep = actor_acts != nullptr;
    DmMlpFwd q;
    q.rows = M; q.in_dim = F; q.hidden = Hm; q.layers = L; q.out_dim = AO;
    q.x = feats + (size_t)i * M * F; q.ldx = F; q.p = actor;
    q.acts = keep ? actor_acts : macts; q.acts_total_rows = keep ? H * M : M; q.acts_row_off = keep ? i * M : 0;
    q.out = keep ? actor_logits + (size_t)i * M * AO : logits_ws; q.ldout = AO;
    q.wpack = actor_wpack; q.add0 = actor_add0; q.sparse_cols = actor_add0 ? Z : 0;
    return q;
  }
  // action ~ OneHotCategorical(actor(feature))                                          dreamer.py:195-200
  // with actor_acts the activations of all H steps are kept (rows i*M..) so ActorCritic's policy-gradient backward
  // reuses them instead of recomputing forward_actor(features[:-1]) (the reference's own TODO, a2c.py:119)
  int rollout_actor(int i) const {
    const float* cur = feats + (size_t)i * M * F;
    float* act = actions + (size_t)i * M * A;
    if (actor_add0) {
      if (i == 0) DM_TRY(dm_sparse_rows_launch(M, Hm, Z, cur + D, F, actor_w0t + (size_t)D * Hm, actor_add0, Hm, st));
      else DM_TRY(dm_z_embed_launch(M, Hm, S, C, pidx, nullptr, actor_w0t + (size_t)D * Hm, nullptr, nullptr, 0, nullptr, nullptr,
                                    actor_add0, Hm, nullptr, nullptr, nullptr, 0.f, nullptr, 0, st));
    }
    int32_t* ai = act_idx_of(i);
    const DmChainSample samp = {u_act + (size_t)i * M, act, A, ai};
    DmMlpFwd q = actor_call(i);
    if (fuse_act) q.sample = &samp;
    const float* logits = q.out;
    DM_TRY(dm_mlp_fwd_launch(q, sk, skb, st));
    if (fuse_act) return DM_OK;
    if (adist == 0)
      return dm_sample_onehot_launch(M, 1, A, logits, A, u_act + (size_t)i * M, nullptr, act, A, ai, nullptr, nullptr, st);
    return dm_sample_continuous_launch(adist, M, A, logits, u_act + (size_t)i * M * A, act, st);
  }
  // cell.forward_prior(action, None, (h, z)) and z ~ prior                              rssm.py:155-184
  int rollout_cell(int i) const {
    const float* cur = feats + (size_t)i * M * F;
    float* nxt = feats + (size_t)(i + 1) * M * F;
    const float* act = actions + (size_t)i * M * A;
    const int32_t* ai = act_idx_of(i);
    const bool embed = wzt && i > 0, embed_a = embed && wat && ai;
    if (!embed_a) DM_TRY(linear(st, sk, skb, M, Hd, A, act, A, p[DM_RSSM_A_W], nullptr, nullptr, 0, ea, Hd));
    if (embed) {
      DM_TRY(dm_z_embed_launch(M, Hd, S, C, pidx, nullptr, wzt, p[DM_RSSM_Z_B], embed_a ? nullptr : ea, Hd,
                               embed_a ? ai : nullptr, wat, nullptr, Hd, nullptr, p[DM_RSSM_IN_G], p[DM_RSSM_IN_B], 1e-3f,
                               za, Hd, st));
    } else {
      DM_TRY(linear(st, sk, skb, M, Hd, Z, cur + D, F, p[DM_RSSM_Z_W], p[DM_RSSM_Z_B], ea, Hd, x1, Hd));
      DM_TRY(norm_elu_fwd(M, Hd, x1, Hd, p[DM_RSSM_IN_G], p[DM_RSSM_IN_B], 1e-3f, za, Hd, stats, st));
    }
    if (gk.L > 1) {
      DM_TRY(gru_stack_fwd(st, sk, skb, gk, M, Hd, D, za, cur, F, gi, gh, nxt, F, nullptr, nullptr, gsw, gstw));
    } else {
      DM_TRY(linear(st, sk, skb, M, 3 * D, Hd, za, Hd, p[DM_RSSM_GRU_WIH], p[DM_RSSM_GRU_BIH], nullptr, 0, gi, 3 * D));
      DM_TRY(linear(st, sk, skb, M, 3 * D, D, cur, F, p[DM_RSSM_GRU_WHH], p[DM_RSSM_GRU_BHH], nullptr, 0, gh, 3 * D));
      if (kind == 0) DM_TRY(dm_gru_gates_fwd_launch(M, D, gi, gh, cur, F, nxt, F, nullptr, nullptr, nullptr, nullptr, st));
      else DM_TRY(dm_gru_norm_fwd_launch(kind, M, D, gi, gh, cur, F, gk.lng[0], gk.lnb[0], nxt, F, gsw, gstw, nullptr, nullptr, st));
    }
    DM_TRY(linear(st, sk, skb, M, Hd, D, nxt, F, p[DM_RSSM_PRIOR_H_W], p[DM_RSSM_PRIOR_H_B], nullptr, 0, x1, Hd));
    DM_TRY(norm_elu_fwd(M, Hd, x1, Hd, p[DM_RSSM_PRIOR_G], p[DM_RSSM_PRIOR_B], 1e-3f, za, Hd, stats, st));
    DM_TRY(linear(st, sk, skb, M, ZP, Hd, za, Hd, p[DM_RSSM_PRIOR_W], p[DM_RSSM_PRIOR_OB], nullptr, 0, prior, ZP));
    return dm_sample_onehot_launch(M, S, C, prior, ZP, u_prior + (size_t)i * M * S, nullptr, nxt + D, F, pidx, nullptr, nullptr, st);
  }
};

extern "C" int dm_dream_rollout(const dm_shape* s, int M, const float* start, const dm_rssm_params* P,
                                const dm_mlp_params* actor, const float* u_act, const float* u_prior, float* feats,
                                float* actions, int32_t* act_idx, float* actor_acts, float* actor_logits, void* ws,
                                size_t ws_bytes, void* stream) {
  DM_REQUIRE(s && start && P && actor && u_act && u_prior && feats && actions && ws, DM_E_NULL,
             "dream_rollout: null pointer");
  DmPrecisionScope prec(s->flags & DM_FLAG_BF16);
  DM_TRY(rssm_check(s));
  DM_REQUIRE(M >= 1 && s->H >= 1, DM_E_SHAPE, "dream_rollout: M=%d H=%d", M, s->H);
  RolloutCtx c = {};
  rssm_dims(s, &c);
  c.M = M; c.H = s->H; c.Hm = s->mlp_hidden; c.L = s->mlp_layers; c.adist = s->flags & 3;
  DM_REQUIRE(c.adist <= 2, DM_E_SHAPE, "dream_rollout: unknown actor distribution %d", c.adist);
  c.AO = c.adist == 0 ? c.A : 2 * c.A;
  DM_REQUIRE((actor_acts == nullptr) == (actor_logits == nullptr), DM_E_NULL,
             "dream_rollout: actor_acts and actor_logits must be given together");
  c.p = P->p; c.actor = actor; c.st = (hipStream_t)stream;
  c.u_act = u_act; c.u_prior = u_prior; c.feats = feats; c.actions = actions; c.act_idx = act_idx;
  c.actor_acts = actor_acts; c.actor_logits = actor_logits;
  DmTwinScope tw((s->flags & DM_FLAG_BF16) != 0);
  DM_TRY(c.plan(ws, ws_bytes));
  tl_last_schedule[2] = (c.wzt ? DM_SCHED_ROLL_WZT : 0) | (c.wat ? DM_SCHED_ROLL_WAT : 0) | (c.actor_wpack ? DM_SCHED_ROLL_ACTOR_WPACK : 0) |
                        (c.actor_add0 ? DM_SCHED_ROLL_ACTOR_ADD0 : 0) | (c.fuse_act ? DM_SCHED_ROLL_FUSE_ACT : 0) |
                        (c.tw_on ? DM_SCHED_ROLL_TW_ON : 0);
  const float* const* p = c.p;
  const int H = c.H, D = c.D, Hd = c.Hd, Z = c.Z, ZP = c.ZP, F = c.F;
  hipStream_t st = c.st;
  DmRolloutMarks marks(st);
  const bool marks_eager = st == (hipStream_t)stream;
  DM_TRY(gru_stack(s, p, nullptr, &c.gk));

  if (c.tw_on) {
    const DmCvtSeg sg[4] = {{p[DM_RSSM_GRU_WIH], c.wih_h, (size_t)3 * D * Hd}, {p[DM_RSSM_GRU_WHH], c.whh_h, (size_t)3 * D * D},
                            {p[DM_RSSM_PRIOR_H_W], c.wph_h, (size_t)Hd * D}, {p[DM_RSSM_PRIOR_W], c.wp_h, (size_t)ZP * Hd}};
    DM_TRY(dm_to_bf16_multi_launch(sg, 4, st));
    for (int i = 0; i < 4; ++i) dm_twin_add(sg[i].src, sg[i].n, sg[i].dst, true);
    dm_twin_add(c.za, (size_t)M * Hd, c.za_h, false);
    for (int i = 1; i <= H && i < 40; ++i)
      dm_twin_add(feats + (size_t)i * M * F, (size_t)M * F, c.feats_h + (size_t)i * M * F, false);
  }
  if (c.wzt) DM_TRY(transpose(st, p[DM_RSSM_Z_W], c.wzt, Hd, Z));
  if (c.wat) DM_TRY(transpose(st, p[DM_RSSM_A_W], c.wat, Hd, c.A));
  if (c.actor_w0t) DM_TRY(transpose(st, actor->w[0], c.actor_w0t, c.Hm, F));
  if (c.actor_wpack) DM_TRY(dm_mlp_chain_pack_launch(F, c.L, actor, c.actor_wpack, st, c.actor_w0t ? D : 0));
  hipError_t e = hipMemcpyAsync(feats, start, (size_t)M * F * sizeof(float), hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return dm_fail(DM_E_HIP, "dream_rollout: %s", hipGetErrorString(e));
  for (int i = 0; i < H; ++i) {
    DM_TRY(c.rollout_actor(i));
    DM_TRY(c.rollout_cell(i));
    marks.at_step(i, st, marks_eager);
  }
  return DM_OK;
}

// ---------------------------------------------------------------- workspace sizing (common.h) ----
// The RSSM calls take an IWAE batch expanded (T, B * I, 1).  Wanted: what the shape alone admits - the caller's pointers are
// taken as aligned and present (idx, the LayerNorm parameters), switches as on, DM_FLAG_BF16 as twins on, the persistent
// kernel by dm_rssm_lds_ws_floats (0 where no plan exists), never by asking the device.
static RolloutDims rollout_dims(const dm_shape* s) {
  dm_shape e = *s;
  e.B = s->B * (s->I > 0 ? s->I : 1); e.I = 1;
  RolloutDims d = {};
  rssm_dims(&e, &d);
  d.M = d.N; d.H = s->H > 0 ? s->H : 1; d.Hm = s->mlp_hidden; d.L = s->mlp_layers; d.adist = s->flags & 3;
  d.AO = d.adist == 0 ? d.A : 2 * d.A;
  return d;
}
size_t dm_rssm_ws_floats(const dm_shape* s, size_t parts[2]) {
  if (!s) return 0;
  const RolloutDims d = rollout_dims(s);
  const bool chain64 = !d.gauss && d.kind == 0 && d.layers == 1 && d.B <= 64;      // the fused schedules' <= 64-row single plain cell
  const bool wzt = !d.gauss && d.T > 1 && dm_z_embed_ok(d.Hd);
  PostWs pw;
  BpttWs bw;
  const size_t fwd = post_layout(DmArena(nullptr, 0), d, wzt, chain64 && d.C == 32, chain64 && wzt && (d.F & 3) == 0 && d.T >= 3, &pw);
  const size_t bwd = bptt_layout(DmArena(nullptr, 0), d, chain64, chain64, &bw);
  if (parts) { parts[0] = fwd; parts[1] = bwd; }
  return fwd > bwd ? fwd : bwd;
}
// M = every row of the shape; the actor's activations in the workspace (actor_acts == NULL).  All three optional blocks are
// wanted whatever the shape: whether the actor runs on the whole-MLP kernel depends on its pointers and a run-time switch.
size_t dm_rollout_ws_floats(const dm_shape* s) {
  if (!s) return 0;
  const RolloutDims d = rollout_dims(s);
  const bool tw = (s->flags & DM_FLAG_BF16) && d.kind == 0 && d.layers == 1 && (d.F & 7) == 0;
  RolloutWs w;
  return rollout_layout(DmArena(nullptr, 0), d, false, tw, true, true, true, &w);
}
