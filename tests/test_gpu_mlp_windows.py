"""-m gpu: dm_mlp_head_fwd_rows, the windowed MLP forward (ActorCritic.forward_values, heads.dream_fwd), at every dispatch branch.

The gradient step fills ONE activation set window by window and then runs ONE dm_mlp_head_bwd over all rows; the windows of one
forward may be answered by different kernels (row panels from 16 384 rows, the whole-MLP kernel from 256 rows, per-layer GEMM +
LayerNorm launches below that or when the operand loads cannot be 16 bytes wide).  Every case here names the kernel it expects
per window and asserts it from the per-launch profiler rows (tests/gemm_pin.py: kind 20 = row-panel forward, 22 = whole-MLP
kernel, GEMM-tile rows only or none = per-layer launches), fills `out` and `acts` with a sentinel bit pattern first, and compares
with oracle.dreamer_oracle.mlp in fp64 at the bars of test_gpu_training_step.py's MLP tests: forward _close(1e-4, 1e-5), dx and
every parameter gradient _rel_l2 < 1e-4.
"""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import dreamer_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/gemm_pin.py
import gemm_pin as GP                                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HID, LAYERS = 400, 4
DENSE, SP = 72, 64                    # the one-hot variant: 72 dense columns + 8 groups of 8 one-hot columns
IN = DENSE + SP                       # 136, the dense variant's width too
SENT = 0x7FC0DEAD                     # a NaN with a payload no arithmetic produces
DM_E_SHAPE = -1
PANEL, CHAIN, PER_LAYER = 'panel', 'chain', 'per-layer'

# rows_total -> windows (row0, rows, kernel with 16-byte operand loads available)
WINDOWS = {
    16700: [(0, 300, CHAIN), (300, 16400, PANEL)],      # 16 400 = 256 * 64 + 16: ragged last panel; row0 300 = 4 * 75
    700: [(0, 290, CHAIN), (290, 410, CHAIN)],          # ragged 16-row blocks in both
    520: [(0, 250, PER_LAYER), (250, 270, CHAIN)],      # below / above the 256-row threshold of the whole-MLP kernel
    600: [(100, 300, CHAIN)],                           # a middle window alone
}
UNALIGNED_X = {PANEL: PANEL, CHAIN: PER_LAYER, PER_LAYER: PER_LAYER}      # the kernel of such a window at ldx = in_dim + 1


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _close(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bad = ~(err <= atol + rtol * b.abs())
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})'


def _sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _acts_layout(rows):
    """csrc/mlp.hip mlp_carve restated: per layer [pre-activations (rows, 400) | LayerNorm statistics (rows, 2) | activations
    (rows, 400)], each array rounded up to 64 floats.  Returns ([(name, offset, width)], total floats)."""
    off, arrays = 0, []
    for l in range(LAYERS):
        for name, w in (('xpre', HID), ('stats', 2), ('y', HID)):
            arrays.append((f'{name}[{l}]', off, w))
            off += (rows * w + 63) // 64 * 64
    return arrays, off


def _acts_mask(rows_total, windows):
    """bool (acts floats): the elements the given (row0, rows) windows own"""
    arrays, total = _acts_layout(rows_total)
    mask = torch.zeros(total, dtype=torch.bool, device=DEV)
    for _, off, w in arrays:
        for row0, rows in windows:
            mask[off + row0 * w: off + (row0 + rows) * w] = True
    return mask


def _path(pins):
    kinds = [r[0] for r in pins]
    if 20 in kinds:
        assert kinds.count(20) == LAYERS and 22 not in kinds, kinds
        return PANEL
    if 22 in kinds:
        assert kinds.count(22) == 1, kinds
        return CHAIN
    assert all(0 <= k < 20 or 24 <= k < GP.NKINDS for k in kinds), kinds
    return PER_LAYER


def _expected(hip, m, rows, path, pad, sparse):
    """The plan's answer for a window of `rows` rows at ldx = in_dim + pad (dm_mlp_plan_query: the mlp_fwd_plan a call runs;
    tests/test_mlp_plan_cpu.py holds it to the dispatch table).  With 16-byte rows of x that is the kernel WINDOWS names.
    ldx = in_dim + 1: no row of x is 16-byte aligned - the whole-MLP kernel hands over to the per-layer launches, the row panels
    stay and take their scalar-load instantiation (the profiler row does not tell the two apart; the stride does)."""
    out = (ctypes.c_int32 * 8)()
    rc = hip.lib().dm_mlp_plan_query(0, rows, IN, HID, LAYERS, m.out_dim, IN + pad, sparse, 16, 1, m.struct().precision, 1, 0, 0, 0,
                                     512 << 20, out)
    assert rc == 0, hip.lib().dm_last_error()
    want = (PANEL, CHAIN, PER_LAYER)[out[0]]
    pinned = UNALIGNED_X[path] if pad & 3 else path
    assert want == pinned, f'{rows} rows, ldx {IN + pad}: the plan says {want}, the table {pinned}'
    return want


def _ws():
    return torch.empty(512 << 20, dtype=torch.uint8, device=DEV)


_CASES = {}


def _case(rows, variant, out_dim, need_ref=True):
    """Model, input, output gradient and the fp64 reference of one (rows, variant, out_dim); computed once, never modified."""
    from pydreamer_amd.models import MLP
    key = (rows, variant, out_dim)
    c = _CASES.get(key)
    if c is None:
        g = torch.Generator().manual_seed(1000 * out_dim + rows + (7 if variant == 'onehot' else 0))
        torch.manual_seed(17 + out_dim)
        m = MLP(IN, out_dim, HID, LAYERS).to(DEV)
        with torch.no_grad():                      # non-trivial LayerNorm parameters
            for i in range(LAYERS):
                m.model[3 * i + 1].weight.uniform_(0.5, 1.5)
                m.model[3 * i + 1].bias.uniform_(-0.5, 0.5)
        x = torch.randn(rows, IN, generator=g)
        if variant == 'onehot':
            idx = torch.randint(0, 8, (rows, 8), generator=g)
            x[:, DENSE:] = F.one_hot(idx, 8).float().reshape(rows, SP)
        dout = torch.randn(rows, out_dim, generator=g) / rows
        c = dict(m=m, x=x.to(DEV), dout=dout.to(DEV), sparse=SP if variant == 'onehot' else 0)
        _CASES[key] = c
    if need_ref and 'out' not in c:
        p = {f'h.{k}': v.detach().double().cpu().requires_grad_(True) for k, v in c['m'].model.state_dict().items()}
        xr = c['x'].double().cpu().requires_grad_(True)
        ref = O.mlp(p, 'h', xr, LAYERS)
        ref.backward(c['dout'].double().cpu().reshape(ref.shape))
        c.update(out=ref.detach().reshape(rows, out_dim), dx=xr.grad, grads={k: v.grad for k, v in p.items()})
    return c


def _strided(x, pad):
    """x in rows of in_dim + pad floats, NaN in the padding columns (never read)"""
    xs = torch.full((x.shape[0], IN + pad), float('nan'), device=DEV)
    xs[:, :IN] = x
    return xs


def _check_whole_equals_window(hip, c, xs, ld, row0, rows, want, out, acts, rows_total, ws):
    """The same rows as a WHOLE call (their own contiguous copy, their own activation set) on the same kernel: same bits in
    `out` and in every activation array."""
    m = c['m']
    sub = xs[row0:row0 + rows].clone()
    acts_w = _sentinel(m.acts_floats(rows))
    res = []
    pins = GP.profiled_rows(hip, lambda: res.append(m.fwd(sub, ld, rows, ws, acts=acts_w, sparse_cols=c['sparse'])[0]))
    assert _path(pins) == want, f'whole call over {rows} rows: {_path(pins)} answered, {want} expected'
    assert _same_bits(res[0], out[row0:row0 + rows]), f'out of window [{row0}, {row0 + rows}) differs from the whole call ({want})'
    whole, _ = _acts_layout(rows)
    full, _ = _acts_layout(rows_total)
    for (name, ow, w), (_, of, _) in zip(whole, full):
        a = acts_w[ow: ow + rows * w]
        b = acts[of + row0 * w: of + (row0 + rows) * w]
        assert _same_bits(a, b), f'{name} of window [{row0}, {row0 + rows}) differs from the whole call ({want})'


def _run_windows(hip, c, rows_total, windows, pad, ws, bit_check=True):
    """The production sequence: every window through MLP.fwd(window=...), into one sentinel-filled `out` and `acts`.  Per
    window: the kernel pin, sentinel bits kept everywhere else (and replaced everywhere inside), the acts-free call's bits,
    and the whole-call bits where the window runs on the panels or the whole-MLP kernel."""
    m, sp, ld = c['m'], c['sparse'], IN + pad
    xs = _strided(c['x'], pad)
    out = _sentinel(rows_total, m.out_dim)
    acts = _sentinel(m.acts_floats(rows_total))
    done = []
    for row0, rows, path in windows:
        want = _expected(hip, m, rows, path, pad, sp)
        pins = GP.profiled_rows(hip, lambda: m.fwd(xs, ld, rows, ws, acts=acts, sparse_cols=sp, window=(rows_total, row0), out=out))
        got = _path(pins)
        assert got == want, f'window [{row0}, {row0 + rows}) of {rows_total}, ldx {ld}: {got} answered, {want} expected'
        done.append((row0, rows))
        rows_done = torch.zeros(rows_total, dtype=torch.bool, device=DEV)
        for r0, n in done:
            rows_done[r0:r0 + n] = True
        assert torch.equal((_bits(out) != SENT).all(1), rows_done) and torch.equal((_bits(out) == SENT).any(1), ~rows_done), \
            f'out: rows outside the windows {done} were written, or rows inside were not'
        assert torch.equal(_bits(acts) != SENT, _acts_mask(rows_total, done)), \
            f'acts: elements outside the windows {done} were written, or elements inside were not'
        out2 = _sentinel(rows_total, m.out_dim)
        m.fwd(xs, ld, rows, ws, save_acts=False, sparse_cols=sp, window=(rows_total, row0), out=out2)
        only = torch.zeros(rows_total, dtype=torch.bool, device=DEV)
        only[row0:row0 + rows] = True
        assert bool((_bits(out2)[~only] == SENT).all()), 'acts-free call wrote outside its window'
        assert _same_bits(out2[row0:row0 + rows], out[row0:row0 + rows]), 'acts-free call: other bits than the saving call'
        if bit_check and want != PER_LAYER:
            _check_whole_equals_window(hip, c, xs, ld, row0, rows, want, out, acts, rows_total, ws)
    assert not torch.isnan(xs[:, :IN]).any()
    return xs, out, acts


def _check_fp64(c, xs, ld, rows_total, windows, out, acts, ws):
    m = c['m']
    covered = sum(n for _, n, _ in windows) == rows_total
    for row0, rows, _ in windows:
        _close(out[row0:row0 + rows], c['out'][row0:row0 + rows], 1e-4, 1e-5, f'forward, window [{row0}, {row0 + rows})')
    if not covered:
        return
    dx = _sentinel(rows_total, IN)
    grads, _, _ = m.bwd(xs, ld, rows_total, acts, c['dout'], ws, dx=dx, lddx=IN, dx_accum=False)      # ONE backward over all rows
    e = _rel_l2(dx, c['dx'])
    assert e < 1e-4, f'dx: {e:.3e}'
    for (name, _), g in zip(m.named_parameters(), grads):
        e = _rel_l2(g, c['grads']['h.' + name.replace('model.', '', 1)])
        assert e < 1e-4, f'{name}: {e:.3e}'


WINDOW_CASES = [(rows_total, variant, out_dim, pad) for rows_total in sorted(WINDOWS) for variant in ('dense', 'onehot')
                for out_dim in (1, 6) for pad in (0, 4, 1) if pad != 1 or rows_total in (16700, 700)]


@pytest.mark.parametrize('rows_total,variant,out_dim,pad', WINDOW_CASES)
def test_windowed_forward_then_one_backward(hip, rows_total, variant, out_dim, pad):
    """WINDOWS[rows_total] through MLP.fwd(window=...), then ONE dm_mlp_head_bwd over rows_total on the window-filled
    activations (600 rows: a middle window alone, forward only).  in_dim 136 dense, and 72 + 8 x 8 one-hot columns with
    sparse_cols 64; out_dim 1 (the critic) and 6.  Reached and pinned: row panels (16 400-row window, ragged last panel, row0 300),
    whole-MLP kernel (300, 290, 410, 270 and 300 rows), per-layer launches (250 rows).  pad 4: ldx = in_dim + 4 with NaN padding.
    pad 1 (16 700 and 700 rows only): ldx = in_dim + 1, rows of x are not 16-byte aligned - the whole-MLP kernel must hand over to
    the per-layer launches and the panels to their scalar-load path.  A panel or whole-MLP window must give the bits of a whole
    call over the same rows on the same kernel (out and every activation array); rows outside a window keep the sentinel."""
    assert hip.lib().dm_mlp_chain_min_rows(0) == 256
    c = _case(rows_total, variant, out_dim)
    ws = _ws()
    windows = WINDOWS[rows_total]
    xs, out, acts = _run_windows(hip, c, rows_total, windows, pad, ws)
    _check_fp64(c, xs, IN + pad, rows_total, windows, out, acts, ws)


def test_acts_layout_helper_matches_the_library(hip):
    for rows in (1, 7, 31, 32, 250, 520, 600, 700, 16700, 33100):
        assert _acts_layout(rows)[1] == hip.lib().dm_mlp_acts_floats(rows, HID, LAYERS), rows


@pytest.mark.parametrize('variant', ['dense', 'onehot'])
@pytest.mark.parametrize('rows,path', [(16700, PANEL), (700, CHAIN), (200, PER_LAYER)])
def test_full_window_equals_the_whole_call(hip, rows, path, variant):
    """row0 = 0, rows = rows_total is dm_mlp_head_fwd / dm_mlp_head_fwd_sparse, bit for bit, on each of the three paths."""
    c = _case(rows, variant, 6, need_ref=False)
    m, sp, ws = c['m'], c['sparse'], _ws()
    res = []
    pins = GP.profiled_rows(hip, lambda: res.append(m.fwd(c['x'], IN, rows, ws, acts=_sentinel(m.acts_floats(rows)), sparse_cols=sp)))
    assert _path(pins) == path
    out_w, acts_w = res[0]
    out, acts = _sentinel(rows, 6), _sentinel(m.acts_floats(rows))
    pins = GP.profiled_rows(hip, lambda: m.fwd(c['x'], IN, rows, ws, acts=acts, sparse_cols=sp, window=(rows, 0), out=out))
    assert _path(pins) == path
    assert _same_bits(out, out_w)
    assert torch.equal(_bits(acts) != SENT, _acts_mask(rows, [(0, rows)]))
    live = _bits(acts) != SENT
    assert _same_bits(acts[live], acts_w[live])


@pytest.mark.parametrize('variant,out_dim', [('dense', 6), ('onehot', 1)])
def test_shifted_panel_window_equals_the_whole_call(hip, variant, out_dim):
    """A 16 689-row window at row0 16 411 (a multiple of neither 16 nor 64) of 33 100 rows runs on the row panels and gives the
    bits of a whole panel call over the same rows; the other 16 411 rows keep the sentinel."""
    rows_total, row0, rows = 33100, 16411, 16689
    c = _case(rows_total, variant, out_dim, need_ref=False)
    _run_windows(hip, c, rows_total, [(row0, rows, PANEL)], 0, _ws())


@pytest.mark.parametrize('variant', ['dense', 'onehot'])
def test_large_whole_mlp_window(hip, variant):
    """A 4 200-row window at row0 333 of 4 700 rows: the whole-MLP kernel on a grid of more than 256 blocks, where it no longer
    asks for a compute unit to itself (every other whole-MLP window of this module is 410 rows or fewer; the step's second head
    window has 12 000).  Pinned; bits of the whole call over the same rows; the forward at the fp64 bar; sentinel outside."""
    rows_total, row0, rows = 4700, 333, 4200
    c = _case(rows_total, variant, 6)
    windows = [(row0, rows, CHAIN)]
    ws = _ws()
    xs, out, acts = _run_windows(hip, c, rows_total, windows, 0, ws)
    _check_fp64(c, xs, IN, rows_total, windows, out, acts, ws)


@pytest.mark.parametrize('variant', ['dense', 'onehot'])
def test_windows_bf16_operands(hip, variant):
    """precision = 1 at 16 700 rows, both windows (whole-MLP kernel, then row panels): window bits = whole-call bits on the same
    kernel, and the forward within the bars test_mlp_head_panel_bf16_operands states against the bf16-operand arithmetic in
    fp64: max error < 5e-3, mean error < 0.2 x the fp32 path's mean distance to it."""
    rows_total = 16700
    c = _case(rows_total, variant, 6, need_ref=False)
    m, ws = c['m'], _ws()
    windows = WINDOWS[rows_total]
    _, out32, _ = _run_windows(hip, c, rows_total, windows, 0, ws, bit_check=False)
    m.precision = 1
    try:
        _, out, _ = _run_windows(hip, c, rows_total, windows, 0, ws)
    finally:
        m.precision = 0
    h = c['x'].double().cpu()
    sd = {k: v.detach().double().cpu() for k, v in m.model.state_dict().items()}
    for i in range(LAYERS):
        pre = h.float().bfloat16().double() @ sd[f'{3 * i}.weight'].float().bfloat16().double().t() + sd[f'{3 * i}.bias']
        h = F.elu(F.layer_norm(pre, (HID,), sd[f'{3 * i + 1}.weight'], sd[f'{3 * i + 1}.bias'], 1e-3))
    ref = h @ sd['12.weight'].t() + sd['12.bias']
    for row0, rows, path in windows:
        err = (out[row0:row0 + rows].double().cpu() - ref[row0:row0 + rows]).abs()
        gap = (out32[row0:row0 + rows].double().cpu() - ref[row0:row0 + rows]).abs()
        print(f'bf16 {path}: max err {float(err.max()):.3e} mean err {float(err.mean()):.3e} fp32 gap {float(gap.mean()):.3e}')
        assert float(err.max()) < 5e-3 and float(err.mean()) < 0.2 * float(gap.mean()), (path, float(err.max()), float(err.mean()), float(gap.mean()))


def test_window_bounds_are_checked_on_the_host(hip):
    """row0 < 0, rows < 1 and row0 + rows > rows_total: DM_E_SHAPE before any launch, `out` keeps its sentinel.  x and out are the
    middle thirds of buffers three times the size, so that even a call that got past the check would stay inside them."""
    c = _case(600, 'dense', 6, need_ref=False)
    m, ws, n = c['m'], _ws(), 600
    st = m.struct()
    x3 = torch.zeros(3 * n, IN, device=DEV)
    out3 = _sentinel(3 * n, 6)
    lib = hip.lib()
    for row0, rows in ((-1, 10), (0, 0), (10, -5), (500, 101), (600, 1), (0, 601)):
        rc = lib.dm_mlp_head_fwd_rows(n, row0, rows, IN, 0, HID, LAYERS, 6, hip.fptr(x3[n:2 * n]), IN, ctypes.byref(st), None,
                                      hip.fptr(out3[n:2 * n]), hip.ptr(ws), ws.numel(), hip.stream())
        assert rc == DM_E_SHAPE, (row0, rows, rc)
        assert b'window' in lib.dm_last_error()
    torch.cuda.synchronize()
    assert bool((_bits(out3) == SENT).all())
