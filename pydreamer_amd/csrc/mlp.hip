// pydreamer MLP (common.py:37-65): [Linear -> LayerNorm(eps 1e-3) -> ELU] x L, Linear.
// Used by the reward / terminal decoders (decoders.py:257-319) and actor / critic / critic_target (a2c.py:37-39).
// Contractions run on gemm.hip (MFMA); LayerNorm+ELU and the bias / gamma / beta column sums are row kernels.
// Host structure: a pure plan (path, optional pieces, workspace need), one layout function per direction, one function per path.
#include "common.h"

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static const size_t MLP_SKB = DM_SPLITK_FLOATS * sizeof(float);

struct MlpActs {
  float* xpre[DM_MAX_MLP_LAYERS];
  float* stats[DM_MAX_MLP_LAYERS];
  float* y[DM_MAX_MLP_LAYERS];
};
static size_t mlp_carve(int rows, int hidden, int layers, float* base, MlpActs* a) {
  DmArena ar(base, (size_t)1 << 62);
  for (int l = 0; l < layers; ++l) {
    float* xp = ar.take((size_t)rows * hidden);
    float* st = ar.take((size_t)rows * 2);
    float* yy = ar.take((size_t)rows * hidden);
    if (a) { a->xpre[l] = xp; a->stats[l] = st; a->y[l] = yy; }
  }
  return ar.off;
}
extern "C" size_t dm_mlp_acts_floats(int rows, int hidden, int layers) {
  if (rows < 0 || hidden < 0 || layers < 0 || layers > DM_MAX_MLP_LAYERS) return 0;
  return mlp_carve(rows, hidden, layers, nullptr, nullptr);
}

// An UPPER BOUND (floats) of mlp_fwd_layout and mlp_bwd_layout, whatever the plans take: any in_dim <= 4096 (wider inputs
// take no optional piece; there is no in_dim argument, so those terms are sized for 4096), both precisions, any sparse_cols,
// with or without `acts`.  Terms: split-K region, the forward's activation ping-pong (3 x rows x hidden; the backward has 2),
// the panel backward's column partials (they also cover the forward's rows x 2 statistics: 3 x hidden floats per 64 rows and
// layer), then the optional pieces named per line.  tests/test_mlp_plan_cpu.py holds every plan to it and pins its values.
static size_t mlp_ws_floats(int rows, int hidden, int layers) {
  const size_t rh = dm_align_up((size_t)rows * hidden, 64);
  return DM_SPLITK_FLOATS + 3 * rh + dm_align_up((size_t)layers * dm_panel_count(rows) * 3 * hidden, 64) +
         dm_align_up((size_t)hidden * hidden, 64) + 256 +     // + the bf16 panel backward's transposed weights
         dm_align_up((size_t)hidden * 2048 + (size_t)layers * hidden * hidden / 2 + 64, 64) +     // + bf16 weight copies (in_dim <= 4096)
         rh + dm_align_up((size_t)hidden * 4096, 64);       // + sparse-column contribution and W0^T (sparse_cols, in_dim <= 4096)
}
extern "C" size_t dm_mlp_ws_floats(int rows, int hidden, int layers) {
  if (rows < 0 || hidden < 0 || layers < 0 || layers > DM_MAX_MLP_LAYERS) return 0;
  return mlp_ws_floats(rows, hidden, layers);
}

// ---------------------------------------------------------------- forward -----------------------
enum { MLP_ADD_NONE = 0, MLP_ADD_HERE = 1, MLP_ADD_CALLER = 2 };      // who makes the sparse columns' addend
struct MlpFwdPlan {
  int path;             // DM_MLP_PANEL / DM_MLP_CHAIN / DM_MLP_PER_LAYER
  int k0;               // layer-0 columns multiplied densely (in_dim: all of them)
  int addend;           // MLP_ADD_*: the other in_dim - k0 columns enter as a gathered sum of W0^T rows
  bool pack_here;       // whole-MLP kernel: weights packed per call into the split-K region (which it does not use otherwise)
  bool bf16_copies;     // row panels: one bf16 copy of the hidden-layer weights per call (they then stream half the bytes)
  bool fuse_out;        // row panels: the output layer rides in the last panel launch's epilogue
  bool normed;          // layer_norm=False (common.py:68-74 NoNorm): null LayerNorm parameters, Linear -> ELU per layer
  size_t need_floats;   // the workspace floats the call touches
};
// The forward's one workspace layout: [split-K | t0 | t1 | t2 | stats] - the activation ping-pong of a call without `acts` -
// and the optional tail: bf16 weight copies, or the sparse columns' addend g and W0^T.  On an arena without a base it sizes.
struct MlpFwdWs {
  float *splitk, *t0, *t1, *t2, *stats, *g, *w0t;
  unsigned short* wh[DM_MAX_MLP_LAYERS];
};
static size_t mlp_fwd_layout(DmArena ar, const DmMlpFwd& q, bool bf16_copies, bool addend, MlpFwdWs* w) {
  const size_t rh = (size_t)q.rows * q.hidden;
  *w = {};
  w->splitk = ar.take(DM_SPLITK_FLOATS);
  w->t0 = ar.take(rh); w->t1 = ar.take(rh); w->t2 = ar.take(rh); w->stats = ar.take((size_t)q.rows * 2);
  for (int l = 0; l < q.layers && bf16_copies; ++l)
    w->wh[l] = (unsigned short*)ar.take(dm_half_floats((size_t)q.hidden * (l == 0 ? q.in_dim : q.hidden)));
  if (addend) { w->g = ar.take(rh); w->w0t = ar.take((size_t)q.in_dim * q.hidden); }
  return ar.off;
}

// Reads the call's numbers, which pointers are given and how they are aligned - nothing behind them; no launch, and on the way
// to DM_OK no allocation or formatting.  An optional piece is taken only if `ws_bytes` has room: the plan is what the call does.
// Path rule: row panels from dm_panel_ok's rows up (LayerNorm; 16-byte rows of W0 - x may be unaligned, the panels keep a
// scalar-load form), else the whole-MLP kernel where dm_mlp_chain_ok admits it, else GEMM + LayerNorm launches per layer (the
// 64-row panels would leave most CUs idle on small batches).
static int mlp_fwd_plan(const DmMlpFwd& q, const void* ws, size_t ws_bytes, MlpFwdPlan* out) {
  const dm_mlp_params* p = q.p;
  DM_REQUIRE(q.layers >= 1 && q.layers <= DM_MAX_MLP_LAYERS, DM_E_SHAPE, "mlp: layers=%d", q.layers);
  DM_REQUIRE(q.sparse_cols >= 0 && q.sparse_cols < q.in_dim, DM_E_SHAPE, "mlp: sparse_cols=%d of in_dim=%d", q.sparse_cols, q.in_dim);
  DM_REQUIRE(!q.add0 || q.wpack, DM_E_NULL, "mlp_fwd: a caller's sparse addend comes with the weights the caller packed for it");
  DM_REQUIRE(ws_bytes >= MLP_SKB, DM_E_WORKSPACE, "mlp_fwd: workspace too small");
  const size_t cap = ws_bytes / sizeof(float);
  MlpFwdWs sized;
  MlpFwdPlan pl = {};
  pl.need_floats = q.acts ? DM_SPLITK_FLOATS : mlp_fwd_layout(DmArena(nullptr, 0), q, false, false, &sized);
  DM_REQUIRE(pl.need_floats <= cap, DM_E_WORKSPACE,
             "mlp_fwd: workspace too small for the activation ping-pong (need %zu floats)", pl.need_floats);
  pl.normed = p->ln_g[0] != nullptr;
  for (int l = 0; l < q.layers; ++l)
    DM_REQUIRE((p->ln_g[l] != nullptr) == pl.normed && (p->ln_b[l] != nullptr) == pl.normed, DM_E_NULL,
               "mlp: layer %d mixes LayerNorm and NoNorm parameters", l);
  // Sparse trailing columns (the one-hot latent of a feature row): layer 0 multiplies only the dense columns, the others
  // contribute the sum of the weight rows their non-zeros name (x W^T = x_dense W_d^T + sum_e x_e W^T[e]).  For the DreamerV2
  // feature (600 dense + 32 of 1024) that is 63 % of a panel layer's flops replaced by a 32-row gather (40 000 rows: 764 us ->
  // 290 us + 135 us), and 58 % of the whole-MLP kernel's MFMA issue and 36 % of its weight stream.  fp32 only: with bf16
  // operands the product is cheaper than the gather (measured: step +0.4 ms).
  const bool split_ok = dm_mlp_chain_sparse_ok(q.in_dim, q.sparse_cols);
  const int dense = q.in_dim - q.sparse_cols;
  bool want_copies = false, want_addend = false;
  pl.k0 = q.in_dim;
  if (pl.normed && dm_panel_ok(q.rows, q.hidden) && (q.in_dim & 3) == 0 && al16(p->w[0])) {
    pl.path = DM_MLP_PANEL;
    pl.fuse_out = q.out_dim <= 32;
    want_copies = dm_cur_precision() && q.in_dim <= 4096 && (q.in_dim & 7) == 0;
    want_addend = split_ok && (q.ldx & 3) == 0;
  } else if (dm_mlp_chain_ok(q.rows, q.in_dim, q.hidden, q.layers, q.out_dim, q.x, q.ldx, p)) {
    pl.path = DM_MLP_CHAIN;
    if (q.wpack) {      // packed by the caller: for k0 = dense if the addend comes with them
      if (q.add0 && split_ok) { pl.addend = MLP_ADD_CALLER; pl.k0 = dense; }
    } else if (dm_mlp_chain_pack_floats(q.in_dim, q.layers) <= DM_SPLITK_FLOATS && al16(ws)) {
      pl.pack_here = true;      // (otherwise the kernel gathers from the row-major weights)
      want_addend = split_ok;
    }
  } else {
    pl.path = DM_MLP_PER_LAYER;
  }
  DM_REQUIRE(!q.sample || pl.path == DM_MLP_CHAIN, DM_E_SHAPE,
             "mlp_fwd: the fused sampler rides in the whole-MLP kernel only (rows %d)", q.rows);
  if (want_copies || want_addend) {
    const size_t full = mlp_fwd_layout(DmArena(nullptr, 0), q, want_copies, want_addend, &sized);
    if (full <= cap) {
      pl.need_floats = full;
      pl.bf16_copies = want_copies;
      if (want_addend) { pl.addend = MLP_ADD_HERE; pl.k0 = dense; }
    }
  }
  *out = pl;
  return DM_OK;
}

int dm_mlp_fwd_path(const DmMlpFwd& q, int* k0) {
  MlpFwdPlan pl;
  DM_TRY(mlp_fwd_plan(q, nullptr, ~(size_t)0, &pl));
  if (k0) *k0 = pl.k0;
  return pl.path;
}

struct MlpFwdCtx {
  const DmMlpFwd& q;
  MlpFwdPlan pl;
  MlpFwdWs w;
  MlpActs a;
  hipStream_t st;
};

// g = the sparse columns' contribution: W0 (hidden, in) -> W0^T (in, hidden), then the rows the non-zeros name, summed
static int mlp_sparse_addend(const MlpFwdCtx& c) {
  const DmMlpFwd& q = c.q;
  DM_TRY(dm_permute4_launch(q.p->w[0], c.w.w0t, 1, 1, q.hidden, q.in_dim, 0, 1, 3, 2, c.st));
  return dm_sparse_rows_launch(q.rows, q.hidden, q.sparse_cols, q.x + c.pl.k0, q.ldx, c.w.w0t + (size_t)c.pl.k0 * q.hidden,
                               c.w.g, q.hidden, c.st);
}

static int mlp_out_layer(const MlpFwdCtx& c, const float* in) {
  const DmMlpFwd& q = c.q;
  DmGemm g;
  g.M = q.rows; g.N = q.out_dim; g.K = q.hidden;
  g.A = in; g.lda = q.hidden;
  g.B = q.p->w[q.layers]; g.ldb = q.hidden;
  g.C = q.out; g.ldc = q.ldout;
  g.bias = q.p->b[q.layers];
  return dm_gemm_launch(g, c.w.splitk, MLP_SKB, c.st);
}

// all layers + the output layer in ONE launch (mlp_chain.hip)
static int mlp_fwd_chain(const MlpFwdCtx& c) {
  const DmMlpFwd& q = c.q;
  const float* wpack = q.wpack;
  const float* add0 = c.pl.addend == MLP_ADD_CALLER ? q.add0 : nullptr;
  if (c.pl.addend == MLP_ADD_HERE) {
    DM_TRY(mlp_sparse_addend(c));
    add0 = c.w.g;
  }
  if (c.pl.pack_here) {
    DM_TRY(dm_mlp_chain_pack_launch(q.in_dim, q.layers, q.p, c.w.splitk, c.st, c.pl.k0));
    wpack = c.w.splitk;
  }
  return dm_mlp_chain_fwd_launch(q.rows, q.in_dim, q.layers, q.out_dim, q.x, q.ldx, q.p, q.acts ? c.a.xpre : nullptr,
                                 q.acts ? c.a.stats : nullptr, q.acts ? c.a.y : nullptr, q.out, q.ldout, wpack, c.st, c.pl.k0,
                                 add0, q.sample);
}

// each Linear -> LayerNorm -> ELU as ONE row-panel launch (panel.hip), the output layer folded into the last one's epilogue
static int mlp_fwd_panel(const MlpFwdCtx& c) {
  const DmMlpFwd& q = c.q;
  const dm_mlp_params* p = q.p;
  const int layers = q.layers;
  if (c.pl.bf16_copies) {
    const float* src[DM_MAX_MLP_LAYERS];
    int rws[DM_MAX_MLP_LAYERS], cls[DM_MAX_MLP_LAYERS];
    for (int l = 0; l < layers; ++l) { src[l] = p->w[l]; rws[l] = q.hidden; cls[l] = l == 0 ? q.in_dim : q.hidden; }
    DM_TRY(dm_panel_bf16_weights_launch(layers, src, c.w.wh, rws, cls, 0, c.st));
  }
  if (c.pl.addend == MLP_ADD_HERE) DM_TRY(mlp_sparse_addend(c));
  const float* in = q.x;
  int ldin = q.ldx, kin = c.pl.k0;
  for (int l = 0; l < layers; ++l) {
    const bool fo = l == layers - 1 && c.pl.fuse_out;
    DM_TRY(dm_panel_ln_fwd_launch(q.rows, q.hidden, kin, in, ldin, p->w[l], p->b[l], p->ln_g[l], p->ln_b[l], 1e-3f,
                                  q.acts ? c.a.xpre[l] : nullptr, q.acts ? c.a.stats[l] : nullptr,
                                  (fo && !q.acts) ? nullptr : c.a.y[l], fo ? p->w[layers] : nullptr,
                                  fo ? p->b[layers] : nullptr, q.out, q.out_dim, q.ldout, c.st, c.w.wh[l], l == 0 ? q.in_dim : 0,
                                  l == 0 ? c.w.g : nullptr));
    in = c.a.y[l]; ldin = q.hidden; kin = q.hidden;
  }
  return c.pl.fuse_out ? DM_OK : mlp_out_layer(c, in);
}

// GEMM + LayerNorm/ELU (or ELU) launches per layer
static int mlp_fwd_layers(const MlpFwdCtx& c) {
  const DmMlpFwd& q = c.q;
  const dm_mlp_params* p = q.p;
  const float* in = q.x;
  int ldin = q.ldx, kin = q.in_dim;
  for (int l = 0; l < q.layers; ++l) {
    DmGemm g;
    g.M = q.rows; g.N = q.hidden; g.K = kin;
    g.A = in; g.lda = ldin;
    g.B = p->w[l]; g.ldb = kin;
    g.C = c.a.xpre[l]; g.ldc = q.hidden;
    g.bias = p->b[l];
    DM_TRY(dm_gemm_launch(g, c.w.splitk, MLP_SKB, c.st));
    if (c.pl.normed)
      DM_TRY(dm_ln_elu_fwd_launch(q.rows, q.hidden, c.a.xpre[l], q.hidden, p->ln_g[l], p->ln_b[l], 1e-3f, c.a.y[l], q.hidden,
                                  c.a.stats[l], c.st));
    else DM_TRY(dm_elu_fwd_launch(q.rows, q.hidden, c.a.xpre[l], q.hidden, c.a.y[l], q.hidden, c.st));
    in = c.a.y[l]; ldin = q.hidden; kin = q.hidden;
  }
  return mlp_out_layer(c, in);
}

// Plan, carve, switch.  `acts` is carved for acts_total_rows rows, of which this call fills [acts_row_off, acts_row_off + rows);
// without `acts` the activations ping-pong through `ws` and no pre-activation / statistics are kept.
int dm_mlp_fwd_launch(const DmMlpFwd& q, void* ws, size_t ws_bytes, hipStream_t st) {
  MlpFwdCtx c = {q, {}, {}, {}, st};
  DM_TRY(mlp_fwd_plan(q, ws, ws_bytes, &c.pl));
  mlp_fwd_layout(DmArena(ws, ws_bytes), q, c.pl.bf16_copies, c.pl.addend == MLP_ADD_HERE, &c.w);
  if (q.acts) {
    DM_REQUIRE(q.acts_row_off >= 0 && q.acts_row_off + q.rows <= q.acts_total_rows, DM_E_SHAPE, "mlp_fwd: acts row window");
    mlp_carve(q.acts_total_rows, q.hidden, q.layers, q.acts, &c.a);
    for (int l = 0; l < q.layers; ++l) {
      c.a.xpre[l] += (size_t)q.acts_row_off * q.hidden;
      c.a.stats[l] += (size_t)q.acts_row_off * 2;
      c.a.y[l] += (size_t)q.acts_row_off * q.hidden;
    }
  } else {
    for (int l = 0; l < q.layers; ++l) { c.a.xpre[l] = c.w.t2; c.a.stats[l] = c.w.stats; c.a.y[l] = (l & 1) ? c.w.t1 : c.w.t0; }
  }
  switch (c.pl.path) {
    case DM_MLP_PANEL: return mlp_fwd_panel(c);
    case DM_MLP_CHAIN: return mlp_fwd_chain(c);
    default: return mlp_fwd_layers(c);
  }
}

// the call of the three exported forwards: rows [row0, row0 + rows) of x / out / acts, which span rows_total rows
static int mlp_head_fwd(int rows_total, int row0, int rows, int in_dim, int sparse_cols, int hidden, int layers, int out_dim,
                        const float* x, int ldx, const dm_mlp_params* p, float* acts, float* out, void* ws, size_t ws_bytes,
                        void* stream) {
  DmPrecisionScope prec(p->precision);
  DmMlpFwd q;
  q.rows = rows; q.in_dim = in_dim; q.hidden = hidden; q.layers = layers; q.out_dim = out_dim;
  q.x = x + (size_t)row0 * ldx; q.ldx = ldx; q.p = p;
  q.acts = acts; q.acts_total_rows = rows_total; q.acts_row_off = row0;
  q.out = out + (size_t)row0 * out_dim; q.ldout = out_dim;
  q.sparse_cols = sparse_cols;
  return dm_mlp_fwd_launch(q, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int dm_mlp_head_fwd(int rows, int in_dim, int hidden, int layers, int out_dim, const float* x, int ldx,
                               const dm_mlp_params* p, float* acts, float* out, void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(x && p && out && ws, DM_E_NULL, "mlp_head_fwd: null pointer");      // acts may be NULL (no backward)
  return mlp_head_fwd(rows, 0, rows, in_dim, 0, hidden, layers, out_dim, x, ldx, p, acts, out, ws, ws_bytes, stream);
}

extern "C" int dm_mlp_head_fwd_sparse(int rows, int in_dim, int sparse_cols, int hidden, int layers, int out_dim,
                                      const float* x, int ldx, const dm_mlp_params* p, float* acts, float* out, void* ws,
                                      size_t ws_bytes, void* stream) {
  DM_REQUIRE(x && p && out && ws, DM_E_NULL, "mlp_head_fwd_sparse: null pointer");
  return mlp_head_fwd(rows, 0, rows, in_dim, sparse_cols, hidden, layers, out_dim, x, ldx, p, acts, out, ws, ws_bytes, stream);
}

// Rows [row0, row0 + rows) of an MLP forward over rows_total rows: x, out and acts are the FULL arrays (acts carved for
// rows_total rows; may be NULL).  Row results do not depend on the window (no cross-row reduction in the forward).
extern "C" int dm_mlp_head_fwd_rows(int rows_total, int row0, int rows, int in_dim, int sparse_cols, int hidden, int layers,
                                    int out_dim, const float* x, int ldx, const dm_mlp_params* p, float* acts, float* out,
                                    void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(x && p && out && ws, DM_E_NULL, "mlp_head_fwd_rows: null pointer");
  DM_REQUIRE(row0 >= 0 && rows >= 1 && row0 + rows <= rows_total, DM_E_SHAPE, "mlp_head_fwd_rows: window [%d, %d) of %d rows", row0,
             row0 + rows, rows_total);
  return mlp_head_fwd(rows_total, row0, rows, in_dim, sparse_cols, hidden, layers, out_dim, x, ldx, p, acts, out, ws, ws_bytes,
                      stream);
}

// ---------------------------------------------------------------- backward ----------------------
struct MlpBwdPlan {
  int path;             // DM_MLP_PANEL / DM_MLP_PER_LAYER
  bool normed;          // layer_norm=False: no LayerNorm parameters, no gradients for them
  bool bf16;            // row panels with bf16 operands: fp32 scratch for one transposed weight (wt)
  bool bf16_copies;     // ... and, if they fit, bf16 copies of W_l^T (hidden x hidden, l >= 1) for the data-gradient panels
  size_t need_floats;
};
// The backward's one workspace layout: [split-K | dy | dxp | column partials | wt | bf16 W_l^T], the last three for the panels
struct MlpBwdWs {
  float *splitk, *dy, *dxp, *colpart, *wt;
  unsigned short* wth[DM_MAX_MLP_LAYERS];      // [l - 1] for layer l
};
static size_t mlp_bwd_layout(DmArena ar, int rows, int hidden, int layers, const MlpBwdPlan& pl, MlpBwdWs* w) {
  const bool panel = pl.path == DM_MLP_PANEL;
  *w = {};
  w->splitk = ar.take(DM_SPLITK_FLOATS);
  w->dy = ar.take((size_t)rows * hidden); w->dxp = ar.take((size_t)rows * hidden);
  w->colpart = ar.take(panel ? (size_t)layers * dm_panel_count(rows) * 3 * hidden : 0);
  if (pl.bf16) w->wt = ar.take((size_t)hidden * hidden);
  for (int l = 1; l < layers && pl.bf16_copies; ++l) w->wth[l - 1] = (unsigned short*)ar.take(dm_half_floats((size_t)hidden * hidden));
  return ar.off;
}
static int mlp_bwd_plan(int rows, int hidden, int layers, const dm_mlp_params* p, size_t ws_bytes, MlpBwdPlan* out) {
  DM_REQUIRE(layers >= 1 && layers <= DM_MAX_MLP_LAYERS, DM_E_SHAPE, "mlp: layers=%d", layers);
  const size_t cap = ws_bytes / sizeof(float);
  MlpBwdWs sized;
  MlpBwdPlan pl = {};
  pl.normed = p->ln_g[0] != nullptr;
  pl.path = pl.normed && dm_panel_ok(rows, hidden) && al16(p->w[layers]) ? DM_MLP_PANEL : DM_MLP_PER_LAYER;
  pl.bf16 = pl.path == DM_MLP_PANEL && dm_cur_precision();
  pl.need_floats = mlp_bwd_layout(DmArena(nullptr, 0), rows, hidden, layers, pl, &sized);
  DM_REQUIRE(pl.need_floats <= cap, DM_E_WORKSPACE, "mlp_head_bwd: workspace too small (need %zu floats)", pl.need_floats);
  if (pl.bf16 && (hidden & 7) == 0 && layers > 1) {
    pl.bf16_copies = true;
    const size_t full = mlp_bwd_layout(DmArena(nullptr, 0), rows, hidden, layers, pl, &sized);
    if (full <= cap) pl.need_floats = full;
    else pl.bf16_copies = false;
  }
  *out = pl;
  return DM_OK;
}

struct MlpBwdCtx {
  int rows, in_dim, hidden, layers, out_dim;
  const float* x; int ldx;
  const dm_mlp_params* p; const float* dout; const dm_mlp_grads* g;
  float* dx; int lddx, dx_accum;
  hipStream_t st;
  MlpBwdPlan pl;
  MlpBwdWs w;
  MlpActs a;
};
// dW[o][i] = sum_r dy[r][o] in[r][i]
static int mlp_wgrad(const MlpBwdCtx& c, int n_out, int n_in, const float* dy, const float* in, int ldin, float* dW) {
  DmGemm g;
  g.a_layout = 1; g.b_layout = 1;
  g.M = n_out; g.N = n_in; g.K = c.rows;
  g.A = dy; g.lda = n_out;
  g.B = in; g.ldb = ldin;
  g.C = dW; g.ldc = n_in;
  return dm_gemm_launch(g, c.w.splitk, MLP_SKB, c.st);
}
// d(in)[r][i] (+)= sum_o dy[r][o] W[o][i]
static int mlp_dgrad(const MlpBwdCtx& c, int n_out, int n_in, const float* dy, const float* W, float* din, int ldd, int accum = 0) {
  DmGemm g;
  g.a_layout = 0; g.b_layout = 1;
  g.M = c.rows; g.N = n_in; g.K = n_out;
  g.A = dy; g.lda = n_out;
  g.B = W; g.ldb = n_in;
  g.C = din; g.ldc = ldd; g.flags = accum ? DM_GEMM_ACCUM : 0;
  return dm_gemm_launch(g, c.w.splitk, MLP_SKB, c.st);
}
// the output layer's parameters: dW_L[o][h] = sum_r dout[r][o] y[r][h], db_L = column sums of dout
static int mlp_bwd_out_params(const MlpBwdCtx& c) {
  DM_TRY(mlp_wgrad(c, c.out_dim, c.hidden, c.dout, c.a.y[c.layers - 1], c.hidden, c.g->w[c.layers]));
  return dm_colsum_launch(c.rows, c.out_dim, c.dout, c.out_dim, c.g->b[c.layers], c.w.splitk, MLP_SKB, c.st);
}

// Row-panel backward (panel.hip): the data-gradient product of layer l+1 and the LayerNorm/ELU backward of layer l are ONE
// launch that also leaves per-panel column sums for dbias / dgamma / dbeta; one final launch adds them up.
static int mlp_bwd_panel(const MlpBwdCtx& c) {
  const dm_mlp_params* p = c.p;
  const int rows = c.rows, hidden = c.hidden, layers = c.layers, npanels = dm_panel_count(rows);
  const size_t cstride = (size_t)npanels * 3 * hidden;
  if (c.pl.bf16_copies) {      // one launch for all layers; destination (in x out) = W_l^T, W_l is (out x in)
    const float* src[DM_MAX_MLP_LAYERS];
    int rws[DM_MAX_MLP_LAYERS], cls[DM_MAX_MLP_LAYERS];
    for (int l = 1; l < layers; ++l) { src[l - 1] = p->w[l]; rws[l - 1] = hidden; cls[l - 1] = hidden; }
    DM_TRY(dm_panel_bf16_weights_launch(layers - 1, src, c.w.wth, rws, cls, 1, c.st));
  }
  DM_TRY(mlp_bwd_out_params(c));
  float* cur = c.w.dxp;
  float* other = c.w.dy;
  DM_TRY(dm_panel_ln_bwd_launch(rows, hidden, c.out_dim, c.dout, c.out_dim, p->w[layers], c.a.xpre[layers - 1],
                                c.a.stats[layers - 1], p->ln_g[layers - 1], p->ln_b[layers - 1], cur,
                                c.w.colpart + (layers - 1) * cstride, nullptr, c.st));
  for (int l = layers - 1; l >= 0; --l) {
    DM_TRY(mlp_wgrad(c, hidden, l ? hidden : c.in_dim, cur, l ? c.a.y[l - 1] : c.x, l ? hidden : c.ldx, c.g->w[l]));
    if (l > 0) {
      DM_TRY(dm_panel_ln_bwd_launch(rows, hidden, hidden, cur, hidden, p->w[l], c.a.xpre[l - 1], c.a.stats[l - 1],
                                    p->ln_g[l - 1], p->ln_b[l - 1], other, c.w.colpart + (l - 1) * cstride, c.w.wt, c.st,
                                    c.w.wth[l - 1]));
      float* t = cur; cur = other; other = t;
    } else if (c.dx) {
      DM_TRY(mlp_dgrad(c, hidden, c.in_dim, cur, p->w[0], c.dx, c.lddx, c.dx_accum));
    }
  }
  const float* parts[3 * DM_MAX_MLP_LAYERS];
  float* outs[3 * DM_MAX_MLP_LAYERS];
  for (int l = 0; l < layers; ++l) {
    const float* base = c.w.colpart + l * cstride;
    parts[3 * l + 0] = base;              outs[3 * l + 0] = c.g->b[l];
    parts[3 * l + 1] = base + hidden;     outs[3 * l + 1] = c.g->ln_g[l];
    parts[3 * l + 2] = base + 2 * hidden; outs[3 * l + 2] = c.g->ln_b[l];
  }
  return dm_panel_colsum_final_launch(3 * layers, parts, outs, hidden, npanels, 3 * hidden, c.st);
}

// GEMM and row-kernel launches per layer
static int mlp_bwd_layers(const MlpBwdCtx& c) {
  const dm_mlp_params* p = c.p;
  const int rows = c.rows, hidden = c.hidden, layers = c.layers;
  float* dy = c.w.dy;
  float* dxp = c.w.dxp;
  DM_TRY(mlp_bwd_out_params(c));
  DM_TRY(mlp_dgrad(c, c.out_dim, hidden, c.dout, p->w[layers], dy, hidden));
  for (int l = layers - 1; l >= 0; --l) {
    if (c.pl.normed) {
      DM_TRY(dm_ln_elu_bwd_dx_launch(rows, hidden, c.a.xpre[l], hidden, c.a.y[l], hidden, c.a.stats[l], p->ln_g[l], dy, hidden,
                                     dxp, hidden, c.st));
      DM_TRY(dm_ln_elu_bwd_params_launch(rows, hidden, c.a.xpre[l], hidden, c.a.y[l], hidden, c.a.stats[l], dy, hidden,
                                         c.g->ln_g[l], c.g->ln_b[l], c.w.splitk, MLP_SKB, c.st));
    } else {
      DM_TRY(dm_elu_bwd_launch(rows, hidden, c.a.y[l], hidden, dy, hidden, dxp, hidden, c.st));
    }
    DM_TRY(mlp_wgrad(c, hidden, l ? hidden : c.in_dim, dxp, l ? c.a.y[l - 1] : c.x, l ? hidden : c.ldx, c.g->w[l]));
    DM_TRY(dm_colsum_launch(rows, hidden, dxp, hidden, c.g->b[l], c.w.splitk, MLP_SKB, c.st));
    if (l > 0) DM_TRY(mlp_dgrad(c, hidden, hidden, dxp, p->w[l], dy, hidden));
    else if (c.dx) DM_TRY(mlp_dgrad(c, hidden, c.in_dim, dxp, p->w[0], c.dx, c.lddx, c.dx_accum));
  }
  return DM_OK;
}

extern "C" int dm_mlp_head_bwd(int rows, int in_dim, int hidden, int layers, int out_dim, const float* x, int ldx,
                               const dm_mlp_params* p, const float* acts, const float* dout, const dm_mlp_grads* g,
                               float* dx, int lddx, int dx_accum, void* ws, size_t ws_bytes, void* stream) {
  DM_REQUIRE(x && p && acts && dout && g && ws, DM_E_NULL, "mlp_head_bwd: null pointer");
  DmPrecisionScope prec(p->precision);
  MlpBwdCtx c = {rows, in_dim, hidden, layers, out_dim, x, ldx, p, dout, g, dx, lddx, dx_accum, (hipStream_t)stream, {}, {}, {}};
  DM_TRY(mlp_bwd_plan(rows, hidden, layers, p, ws_bytes, &c.pl));
  mlp_bwd_layout(DmArena(ws, ws_bytes), rows, hidden, layers, c.pl, &c.w);
  mlp_carve(rows, hidden, layers, const_cast<float*>(acts), &c.a);
  return c.pl.path == DM_MLP_PANEL ? mlp_bwd_panel(c) : mlp_bwd_layers(c);
}

// ---------------------------------------------------------------- the plans, without a device ----
// include/dreamer_hip.h dm_mlp_plan_query: mlp_fwd_plan (which = 0) / mlp_bwd_plan (1) on placeholder addresses that are never
// dereferenced - x and the weights at base_align, everything else 16-byte aligned.
// out = {path, k0, MLP_ADD_*, pack_here, bf16_copies, fuse_out, need_floats low 32 bits, high 32 bits}
extern "C" int dm_mlp_plan_query(int which, int rows, int in_dim, int hidden, int layers, int out_dim, int ldx, int sparse_cols,
                                 int base_align, int normed, int precision, int has_acts, int has_wpack, int has_add0,
                                 int has_sample, size_t ws_bytes, int32_t out[8]) {
  DM_REQUIRE(out, DM_E_NULL, "mlp_plan_query: null output");
  DM_REQUIRE((unsigned)which <= 1 && base_align >= 4 && base_align <= 4096 && (base_align & (base_align - 1)) == 0, DM_E_SHAPE,
             "mlp_plan_query: which %d, base_align %d", which, base_align);
  for (int i = 0; i < 8; ++i) out[i] = 0;
  float* const aligned = reinterpret_cast<float*>((uintptr_t)1 << 20);
  float* const base = reinterpret_cast<float*>(((uintptr_t)1 << 20) + (uintptr_t)base_align);
  DmPrecisionScope prec(precision != 0);
  dm_mlp_params p = {};
  for (int l = 0; l <= DM_MAX_MLP_LAYERS; ++l) p.w[l] = p.b[l] = base;
  for (int l = 0; l < DM_MAX_MLP_LAYERS && normed; ++l) p.ln_g[l] = p.ln_b[l] = aligned;
  size_t need;
  if (which == 1) {
    MlpBwdPlan pl;
    DM_TRY(mlp_bwd_plan(rows, hidden, layers, &p, ws_bytes, &pl));
    out[0] = pl.path; out[1] = in_dim; out[4] = pl.bf16_copies;
    need = pl.need_floats;
  } else {
    const DmChainSample sample = {};
    DmMlpFwd q;
    q.rows = rows; q.in_dim = in_dim; q.hidden = hidden; q.layers = layers; q.out_dim = out_dim;
    q.x = base; q.ldx = ldx; q.p = &p; q.sparse_cols = sparse_cols;
    q.acts = has_acts ? aligned : nullptr;
    q.wpack = has_wpack ? aligned : nullptr; q.add0 = has_add0 ? aligned : nullptr; q.sample = has_sample ? &sample : nullptr;
    MlpFwdPlan pl;
    DM_TRY(mlp_fwd_plan(q, aligned, ws_bytes, &pl));
    out[0] = pl.path; out[1] = pl.k0; out[2] = pl.addend; out[3] = pl.pack_here; out[4] = pl.bf16_copies; out[5] = pl.fuse_out;
    need = pl.need_floats;
  }
  out[6] = (int32_t)(uint32_t)(need & 0xFFFFFFFFu); out[7] = (int32_t)(uint32_t)((uint64_t)need >> 32);
  return DM_OK;
}
