"""The case table of tests/test_gpu_mlp_backward.py and its references, shared with tests/test_mlp_backward_cases_cpu.py.
Not a test module; importable without a GPU.

dm_mlp_head_bwd (csrc/mlp.hip) is the backward pass of every MLP of the project.  mlp_bwd_plan picks one of two paths - the
row panels of csrc/panel.hip, or GEMM / LayerNorm-ELU / column-sum launches per layer - and every panel launch picks one of four
kernel instantiations in dm_panel_ln_bwd_launch.  Each row of CASES names the answer it expects; branch_of() restates the two
rules, tests/test_mlp_backward_cases_cpu.py holds the table to branch_of and to dm_mlp_plan_query, and the GPU test pins the path
from the profiler rows.  A new head shape gets a row here.
"""
import ctypes
from collections import namedtuple

import torch

HIDDEN_PANEL, PANEL_MIN_ROWS, PANEL_BM, MAX_LAYERS = 400, 16384, 64, 8
PANEL, PER_LAYER = 'panel', 'per-layer'
FP32_VEC, FP32_SCALAR, BF16_COPIES, BF16_WT = 'fp32-vec', 'fp32-scalar', 'bf16-copies', 'bf16-wt'
LDDX_PAD = 8                          # dx mode 'accum': lddx = in_dim + 8
EPS = 1e-3

# rows, in_dim, pad (ldx = in_dim + pad), hidden, layers, out_dim, layer_norm, precision (0 fp32, 1 bf16 operands),
# dx: 'none' (dx = NULL) / 'write' (lddx = in_dim) / 'accum' (dx_accum = 1, lddx = in_dim + 8),
# ws: 'ample' (dm_mlp_ws_floats) / 'no_copies' (cut to what the layout without the bf16 W^T copies needs),
# path: PANEL / PER_LAYER, out_launch / hid_launch: (branch, k-tiles) of the output layer's panel launch and of each
# hidden-to-hidden panel launch (None: no such launch)
Case = namedtuple('Case', 'name rows in_dim pad hidden layers out_dim layer_norm precision dx ws path out_launch hid_launch')

CASES = [
    # ragged last panel of 16 rows; the output layer's 6 columns: scalar loads, one k-tile
    Case('panel-ragged16', 16400, 136, 0, 400, 4, 6, True, 0, 'write', 'ample', PANEL, (FP32_SCALAR, 1), (FP32_VEC, 13)),
    # the two-hot critic's 255 bins: scalar loads over 8 k-tiles, the last of 31; a last panel of ONE row
    Case('panel-twohot255', 16385, 136, 0, 400, 4, 255, True, 0, 'accum', 'ample', PANEL, (FP32_SCALAR, 8), (FP32_VEC, 13)),
    # 16-byte loads over exactly one k-tile; one layer: no hidden-to-hidden panel; rows of x not 16-byte aligned
    Case('panel-out32-L1', 16400, 136, 1, 400, 1, 32, True, 0, 'write', 'ample', PANEL, (FP32_VEC, 1), None),
    # 16-byte loads, two k-tiles, the second of 4
    Case('panel-out36-L2', 16400, 136, 0, 400, 2, 36, True, 0, 'none', 'ample', PANEL, (FP32_VEC, 2), (FP32_VEC, 13)),
    # DM_MAX_MLP_LAYERS: the final column-sum launch adds up its maximum of 24 vectors
    Case('panel-L8', 16384, 136, 0, 400, 8, 1, True, 0, 'write', 'ample', PANEL, (FP32_SCALAR, 1), (FP32_VEC, 13)),
    # in_dim % 4 != 0: the forward runs per layer, the backward on the panels - activations of one path feed the other
    Case('panel-in27', 16400, 27, 0, 400, 2, 6, True, 0, 'write', 'ample', PANEL, (FP32_SCALAR, 1), (FP32_VEC, 13)),
    Case('panel-bf16-copies', 16400, 136, 0, 400, 4, 6, True, 1, 'write', 'ample', PANEL, (FP32_SCALAR, 1), (BF16_COPIES, 13)),
    Case('panel-bf16-nocopies', 16400, 136, 0, 400, 4, 6, True, 1, 'write', 'no_copies', PANEL, (FP32_SCALAR, 1), (BF16_WT, 13)),
    # a bf16 hidden launch behind an fp32 scalar-load output-layer launch of 8 k-tiles
    Case('panel-bf16-out255', 16400, 136, 0, 400, 2, 255, True, 1, 'accum', 'ample', PANEL, (FP32_SCALAR, 8), (BF16_COPIES, 13)),
    # (added) bf16 with one layer: the plan carves the transpose scratch, takes no copies and launches no bf16 panel
    Case('panel-bf16-L1', 16400, 136, 0, 400, 1, 6, True, 1, 'write', 'ample', PANEL, (FP32_SCALAR, 1), None),
    Case('layers-nonorm', 16400, 136, 0, 400, 4, 6, False, 0, 'accum', 'ample', PER_LAYER, None, None),
    Case('layers-h128', 300, 72, 4, 128, 3, 7, True, 0, 'accum', 'ample', PER_LAYER, None, None),
    Case('layers-h1024', 300, 96, 0, 1024, 2, 1134, True, 0, 'write', 'ample', PER_LAYER, None, None),       # the map probe's decoder
    Case('layers-row1', 1, 136, 0, 400, 4, 6, True, 0, 'write', 'ample', PER_LAYER, None, None),
    Case('layers-16383', 16383, 136, 0, 400, 4, 6, True, 0, 'write', 'ample', PER_LAYER, None, None),        # one row under the panels
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def ldx_of(case):
    return case.in_dim + case.pad


def lddx_of(case):
    return case.in_dim + (LDDX_PAD if case.dx == 'accum' else 0)


def path_of(case):
    """mlp_bwd_plan's path rule (the output weight is a tensor of its own: 16-byte aligned)."""
    return PANEL if case.layer_norm and case.hidden == HIDDEN_PANEL and case.rows >= PANEL_MIN_ROWS else PER_LAYER


def copies_of(case):
    """mlp_bwd_plan's bf16_copies, given room for them."""
    return path_of(case) == PANEL and case.precision == 1 and case.hidden % 8 == 0 and case.layers > 1 and case.ws == 'ample'


def _panel_branch(precision, kup, lddup, wt, wth):
    """The if ladder of dm_panel_ln_bwd_launch for a 16-byte aligned incoming gradient: (branch, k-tiles of 32)."""
    avec = kup % 4 == 0 and lddup % 4 == 0
    ktiles = (kup + 31) // 32
    if precision and wth and avec and kup >= 32 and kup % 8 == 0:
        return BF16_COPIES, ktiles
    if precision and wt and avec and kup >= 32:
        return BF16_WT, ktiles
    return (FP32_VEC if avec else FP32_SCALAR), ktiles


def branch_of(case):
    """-> (path, [(branch, k-tiles) of every panel launch of the call, in launch order]).  mlp_bwd_panel: the output layer's
    data gradient first (kup = out_dim, no transpose scratch and no copy handed over: fp32 whatever the precision), then one
    launch per hidden layer l = layers - 1 .. 1 (kup = hidden, the scratch and - if the plan took them - the copies)."""
    if path_of(case) != PANEL:
        return PER_LAYER, []
    launches = [_panel_branch(case.precision, case.out_dim, case.out_dim, False, False)]
    for _ in range(case.layers - 1):
        launches.append(_panel_branch(case.precision, case.hidden, case.hidden, case.precision == 1, copies_of(case)))
    return PANEL, launches


def expected_launches(case):
    """The table's own answer in the form branch_of returns."""
    if case.path != PANEL:
        return case.path, []
    return PANEL, [case.out_launch] + [case.hid_launch] * (case.layers - 1)


# ---------------------------------------------------------------------------------------------- the library's own plan
def plan_query(lib, case, ws_bytes):
    """dm_mlp_plan_query(which = 1): the mlp_bwd_plan a call runs -> (return code, path, copies, need in floats)."""
    out = (ctypes.c_int32 * 8)()
    rc = lib.dm_mlp_plan_query(1, case.rows, case.in_dim, case.hidden, case.layers, case.out_dim, ldx_of(case), 0, 16,
                               int(case.layer_norm), case.precision, 1, 0, 0, 0, ws_bytes, out)
    need = (out[6] & 0xFFFFFFFF) | ((out[7] & 0xFFFFFFFF) << 32)
    return rc, (PANEL, 'chain', PER_LAYER)[out[0]], int(out[4]), need


def ws_bytes_of(lib, case):
    """The workspace bytes the case hands to dm_mlp_head_bwd.  'ample': dm_mlp_ws_floats, which holds every optional piece.
    'no_copies': found the way tests/test_mlp_plan_cpu.py _steps finds it - four bytes under the need the plan reports with
    the copies drop them; the call gets exactly what the plan then reports."""
    full = 4 * int(lib.dm_mlp_ws_floats(case.rows, case.hidden, case.layers))
    if case.ws == 'ample':
        return full
    rc, _, copies, need = plan_query(lib, case, full)
    assert rc == 0 and copies == 1, (case.name, rc, copies)
    rc, _, copies, less = plan_query(lib, case, 4 * need - 4)
    assert rc == 0 and copies == 0 and less < need, (case.name, rc, copies, less, need)
    return 4 * less


# ---------------------------------------------------------------------------------------------- which products are rounded
def gemm_rounds(al, bl, M, N, K, lda, ldb):
    """Does dm_gemm_launch (csrc/gemm.hip) round the operands of this product to bf16 under precision = 1, bases 16-byte
    aligned?  Not on the one-launch skinny kernel (csrc/gemm_skinny.hip skinny_ok / dm_gemm_skinny_takes: A row-major, at most
    512 rows, K >= 16 and a multiple of 4, N * K >= 64 Ki, beyond 64 rows K <= 1024 and N * K <= 1100 Ki), and not where an
    operand cannot take 16-byte loads (gemm_plan a_vec / b_vec: row stride and contiguous extent multiples of 4) - those run
    the scalar-load tile, which has no bf16 variant.  tests/test_gpu_vectorenv.py _bf16_product is the forward's case of it."""
    a_vec = lda % 4 == 0 and (K if al == 0 else M) % 4 == 0
    b_vec = ldb % 4 == 0 and (K if bl == 0 else N) % 4 == 0
    return not gemm_skinny(al, bl, M, N, K, lda, ldb) and a_vec and b_vec


def gemm_skinny(al, bl, M, N, K, lda, ldb):
    """dm_gemm_skinny_takes for a plain product on 16-byte aligned bases.  Such a product leaves no per-launch profiler row."""
    return (al == 0 and 1 <= M <= 512 and K >= 16 and K % 4 == 0 and lda % 4 == 0 and (bl == 1 or ldb % 4 == 0)
            and N * K >= 64 * 1024 and (M <= 64 or (K <= 1024 and N * K <= 1100 * 1024)))


def bf16_touched(case):
    """Names of the outputs that lie behind at least one rounded product.  The others come from the same kernels on the same
    operands at either precision: the same bits."""
    L = case.layers
    r = {(name, l): rounded for name, l, _, _, rounded in backward_products(case)}
    touched = {'dW_out'} if r[('wgrad', L)] else set()
    tainted = r[('dgrad', L)]
    for l in range(L - 1, -1, -1):
        if tainted:
            touched |= {f'db_{l}', f'dgamma_{l}', f'dbeta_{l}'} if case.layer_norm else {f'db_{l}'}
        if tainted or r[('wgrad', l)]:
            touched.add(f'dW_{l}')
        tainted = tainted or r.get(('dgrad', l), False)
    if case.dx != 'none' and tainted:
        touched.add('dx')
    return touched


def backward_products(case):
    """The products of one dm_mlp_head_bwd call in launch order: (name, layer, who, (al, bl, M, N, K, lda, ldb), rounded).
    name 'wgrad' (dW_l = dy^T in) / 'dgrad' (the data gradient INTO layer l - 1, or dx for l = 0); layer = layers for the
    output layer; who 'gemm' or 'panel'; rounded: bf16 operands under the case's precision."""
    L, h, rows, bf = case.layers, case.hidden, case.rows, case.precision == 1
    panel = path_of(case) == PANEL
    _, launches = branch_of(case)
    out = []

    def gemm(name, l, al, bl, M, N, K, lda, ldb):
        out.append((name, l, 'gemm', (al, bl, M, N, K, lda, ldb), bf and gemm_rounds(al, bl, M, N, K, lda, ldb)))

    def wgrad(l):
        n_out = case.out_dim if l == L else h
        n_in = case.in_dim if l == 0 else h
        gemm('wgrad', l, 1, 1, n_out, n_in, rows, n_out, ldx_of(case) if l == 0 else h)

    wgrad(L)
    if panel:
        out.append(('dgrad', L, 'panel', (0, 1, rows, h, case.out_dim, case.out_dim, h), launches[0][0] in (BF16_COPIES, BF16_WT)))
    else:
        gemm('dgrad', L, 0, 1, rows, h, case.out_dim, case.out_dim, h)
    for l in range(L - 1, -1, -1):
        wgrad(l)
        if l > 0 and panel:
            out.append(('dgrad', l, 'panel', (0, 1, rows, h, h, h, h), launches[L - l][0] in (BF16_COPIES, BF16_WT)))
        elif l > 0:
            gemm('dgrad', l, 0, 1, rows, h, h, h, h)
        elif case.dx != 'none':
            gemm('dgrad', 0, 0, 1, rows, case.in_dim, h, h, case.in_dim)
    return out


# ---------------------------------------------------------------------------------------------- model, inputs, reference
def make_model(case, device):
    """The case's MLP with non-trivial LayerNorm parameters (the existing MLP tests' ranges)."""
    from pydreamer_amd.models import MLP
    torch.manual_seed(17 + case.out_dim + 10 * case.layers + case.in_dim)      # by shape: the two bf16 workspace cases share a model
    m = MLP(case.in_dim, case.out_dim, case.hidden, case.layers, layer_norm=case.layer_norm)
    if case.layer_norm:
        with torch.no_grad():
            for i in range(case.layers):
                m.model[3 * i + 1].weight.uniform_(0.5, 1.5)
                m.model[3 * i + 1].bias.uniform_(-0.5, 0.5)
    return m.to(device)


def make_inputs(case, device):
    """x as (rows, ldx) with NaN in the padding columns, dout = randn / rows."""
    g = torch.Generator().manual_seed(7919 * case.rows + 31 * case.in_dim + case.out_dim + case.layers)
    x = torch.full((case.rows, ldx_of(case)), float('nan'))
    x[:, :case.in_dim] = torch.randn(case.rows, case.in_dim, generator=g)
    dout = torch.randn(case.rows, case.out_dim, generator=g) / case.rows
    return x.to(device), dout.to(device)


def split_acts(acts, rows, hidden, layers):
    """csrc/mlp.hip mlp_carve restated: per layer [pre-activations (rows, hidden) | LayerNorm statistics (rows, 2) | activations
    (rows, hidden)], every array rounded up to 64 floats.  -> (list of pre-activation views, list of activation views)."""
    off, xpre, y = 0, [], []
    for _ in range(layers):
        for name, w in (('xpre', hidden), ('stats', 2), ('y', hidden)):
            if name != 'stats':
                (xpre if name == 'xpre' else y).append(acts[off: off + rows * w].view(rows, w))
            off += (rows * w + 63) // 64 * 64
    return xpre, y


def acts_floats(case):
    """dm_mlp_acts_floats restated (split_acts' layout)."""
    return sum((case.rows * w + 63) // 64 * 64 for _ in range(case.layers) for w in (case.hidden, 2, case.hidden))


def grad_names(case):
    """Names of the parameter gradients in MLP.parameters() order (Linear, LayerNorm per layer, then the output Linear)."""
    names = []
    for l in range(case.layers):
        names += [f'dW_{l}', f'db_{l}'] + ([f'dgamma_{l}', f'dbeta_{l}'] if case.layer_norm else [])
    return names + ['dW_out', 'db_out']


def _bf16(t, dtype):
    return t.float().bfloat16().to(dtype)


def reference(case, m, x, dout, dtype, acts=None):
    """The case's MLP and its gradients in torch, on the device of x, in `dtype`, as an EXPLICIT layer-by-layer backward (no
    autograd): {'out', 'dx' (rows, in_dim), 'dW_l', 'db_l', 'dgamma_l', 'dbeta_l', 'dW_out', 'db_out'}.

    precision = 1: both operands of exactly the backward products that the library rounds (backward_products) are rounded to
    bf16 - the incoming gradient, the weights, the activations - and everything else stays in `dtype`.  Which FORWARD products
    a call rounds is the forward plan's business (tests/test_gpu_mlp_windows.py), so such a case hands over `acts`, the
    activation set the library's forward saved: its pre-activations and activations replace the reference's own forward and the
    backward is judged on the inputs it really gets.  acts = None (fp32 cases): the reference runs its own forward."""
    L, h, rows = case.layers, case.hidden, case.rows
    assert case.precision == 0 or acts is not None, 'a bf16 case is judged on the activations its forward saved'
    ws, bs, gs, bes = m.tensors()
    cv = lambda t: t.detach().to(device=x.device, dtype=dtype)
    W, B, G, BE = [cv(t) for t in ws], [cv(t) for t in bs], [cv(t) for t in gs], [cv(t) for t in bes]
    xin = x[:, :case.in_dim].to(dtype)
    dout = dout.to(dtype)
    rounded = {(name, l): r for name, l, _, _, r in backward_products(case)}

    def operands(key, a, b):
        return (_bf16(a, dtype), _bf16(b, dtype)) if rounded[key] else (a, b)

    # ---- forward
    saved = split_acts(acts, rows, h, L) if acts is not None else None
    ins, xhat, rstd, z = [xin], [], [], []
    for l in range(L):
        pre = saved[0][l].to(dtype) if saved else ins[l] @ W[l].t() + B[l]
        if case.layer_norm:
            mean = pre.mean(1, keepdim=True)
            rs = 1.0 / torch.sqrt(((pre - mean) ** 2).mean(1, keepdim=True) + EPS)
            xh = (pre - mean) * rs
            xhat.append(xh)
            rstd.append(rs)
            z.append(xh * G[l] + BE[l])
        else:
            z.append(pre)
        ins.append(saved[1][l].to(dtype) if saved else torch.where(z[l] > 0, z[l], torch.expm1(z[l])))
    res = {'out': ins[L] @ W[L].t() + B[L]}

    # ---- backward
    a, b = operands(('wgrad', L), dout, ins[L])
    res['dW_out'] = a.t() @ b
    res['db_out'] = dout.sum(0)
    a, b = operands(('dgrad', L), dout, W[L])
    dy = a @ b
    for l in range(L - 1, -1, -1):
        gl = dy * torch.where(z[l] > 0, torch.ones_like(z[l]), torch.exp(z[l]))
        if case.layer_norm:
            res[f'dbeta_{l}'] = gl.sum(0)
            res[f'dgamma_{l}'] = (gl * xhat[l]).sum(0)
            g = gl * G[l]
            dpre = rstd[l] * (g - g.mean(1, keepdim=True) - xhat[l] * (g * xhat[l]).mean(1, keepdim=True))
        else:
            dpre = gl
        res[f'db_{l}'] = dpre.sum(0)
        a, b = operands(('wgrad', l), dpre, ins[l])
        res[f'dW_{l}'] = a.t() @ b
        if l > 0 or case.dx != 'none':
            a, b = operands(('dgrad', l), dpre, W[l])
            dy = a @ b
    if case.dx != 'none':
        res['dx'] = dy
    return res
