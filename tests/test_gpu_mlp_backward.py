"""-m gpu: dm_mlp_head_bwd, the one backward pass of every MLP of the project, ELEMENT BY ELEMENT at every branch of its plan.

tests/mlp_backward_cases.py holds the case table (one row per branch of mlp_bwd_plan and of dm_panel_ln_bwd_launch's ladder,
csrc/mlp.hip and csrc/panel.hip) and the references; tests/test_mlp_backward_cases_cpu.py holds the table to the library's own
plan without a device.  Per case, here: MLP.fwd into a sentinel-filled activation set, ONE dm_mlp_head_bwd through MLP.bwd_into
with every gradient pre-filled with NaN and dx with a sentinel bit pattern (dx_accum: a base at the scale of the gradient, the
padding columns of lddx = in_dim + 8 still the sentinel), then

  * the path, pinned from the per-launch profiler rows (tests/gemm_pin.py): kind 21 (a row-panel backward launch) exactly `layers`
    times on the panels and never on the per-layer path, and the GEMM rows in the order and with the shapes backward_products
    names, each carrying the bf16 flag exactly when the case's precision is 1.  (The row says that bf16 mode reached the
    product; whether its operands can take the 16-byte loads the bf16 tiles need follows from strides the caller knows -
    gemm_rounds restates that - and the element-wise bars below then hold the rule: a product rounded on one side only misses
    them by orders of magnitude.  At precision 1, outputs behind no rounded product must have the fp32 path's bits.)
  * completeness: no NaN left in any gradient, the padding columns of dx keep their sentinel bits;
  * accuracy: every tensor - dx, dW_l, db_l, dgamma_l, dbeta_l, dW_out, db_out - through oracle.conv_reference.check_tensor:
    max element error over rms(ref64) at most BAR_FACTOR = 10 times what the same arithmetic in torch fp32 misses torch fp64
    by, floored at 64 fp32 roundings.  fp32 cases: the reference runs its own forward.  bf16 cases: the reference rounds the
    operands of exactly the backward products the library rounds and is handed the activation set the library's forward saved
    (reference()'s docstring), and additionally every output behind a rounded product sits five times closer (mean absolute
    error) to that arithmetic than the library's fp32 backward on the same activations does;
  * the bf16 W^T copies against the transpose into the scratch: the same bits in every output (both round the same fp32 weights
    with the same instruction, the transpose is exact, the MFMAs see the same operands in the same k order);
  * determinism: a second identical call gives the same bits in every output (no float atomics on either path).

Each report row is also printed as `[bars] case tensor err err_ref32 ratio bar`; profiles/mlp_backward_bars.txt holds those of the
run this module was written on.
"""
import os
import sys

import pytest
import torch

from oracle import conv_reference as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/gemm_pin.py, tests/mlp_backward_cases.py
import gemm_pin as GP                                # noqa: E402
import mlp_backward_cases as MC                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = 0x7FC0DEAD                     # a NaN with a payload no arithmetic produces
PANEL_BWD_KIND = 21

_SHARED = {}


def _sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.view(torch.int32)


def _ws():
    if 'ws' not in _SHARED:
        _SHARED['ws'] = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    return _SHARED['ws']


def _setup(case):
    """Model and inputs of a case, built once per shape (the two bf16 workspace cases share theirs) and never modified."""
    key = case[1:8]
    if key not in _SHARED:
        x, dout = MC.make_inputs(case, DEV)
        _SHARED[key] = (MC.make_model(case, DEV), x, dout)
    return _SHARED[key]


def _backward(hip, case, m, x, dout, acts, ws, base):
    """One dm_mlp_head_bwd: ({name: gradient}, dx buffer or None, profiler rows)."""
    rows = case.rows
    grads = [torch.full_like(p, float('nan')) for p in m.parameters()]
    gof = {id(p): g for p, g in zip(m.parameters(), grads)}
    dx, lddx = None, 0
    if case.dx != 'none':
        lddx = MC.lddx_of(case)
        dx = _sentinel(rows, lddx)
        if case.dx == 'accum':
            dx[:, :case.in_dim] = base
    pins = GP.profiled_rows(hip, lambda: m.bwd_into(gof, x, MC.ldx_of(case), rows, acts, dout, ws, dx, lddx, case.dx == 'accum'))
    return dict(zip(MC.grad_names(case), grads)), dx, pins


def _outputs(case, grads, dx):
    out = dict(grads)
    if dx is not None:
        out['dx'] = dx[:, :case.in_dim]
    return out


def _check_pins(case, pins):
    kinds = [r[0] for r in pins]
    assert 20 not in kinds and 22 not in kinds, kinds
    if case.path == MC.PANEL:
        assert kinds.count(PANEL_BWD_KIND) == case.layers, f'{case.name}: {kinds.count(PANEL_BWD_KIND)} panel launches, {case.layers} layers'
    else:
        assert PANEL_BWD_KIND not in kinds, f'{case.name}: a panel launch on the per-layer path ({kinds})'
    want = []
    for name, l, who, (al, bl, M, N, K, lda, ldb), _ in MC.backward_products(case):
        if who == 'panel':
            want.append('panel')
        elif not MC.gemm_skinny(al, bl, M, N, K, lda, ldb):
            want.append((al, bl, M, N, K))
    got = []
    for r in pins:
        if r[0] == PANEL_BWD_KIND:
            got.append('panel')
            continue
        _, _, al, bl, _, flags = GP.decode(r)
        got.append((al, bl) + r[1:4])
        assert bool(flags & GP.FLAG_BF16) == (case.precision == 1) and not flags & GP.FLAG_BF16_STORAGE, (case.name, r)
    assert got == want, f'{case.name}: launches {got}, expected {want}'


def _same_bits(case, a, b, what):
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f'{case.name}: {k} differs {what}'


@pytest.mark.parametrize('case', MC.CASES, ids=lambda c: c.name)
def test_mlp_backward_every_element(hip, case):
    lib = hip.lib()
    rows, in_dim = case.rows, case.in_dim
    m, x, dout = _setup(case)
    ws = _ws()
    ws_case = ws[:MC.ws_bytes_of(lib, case)]
    m.precision = case.precision
    try:
        acts = _sentinel(m.acts_floats(rows))
        m.fwd(x, MC.ldx_of(case), rows, ws, acts=acts)
        xpre, ys = MC.split_acts(acts, rows, case.hidden, case.layers)
        assert not any(bool(torch.isnan(t).any()) for t in xpre + ys), 'the forward left part of the activation set unwritten'
        given = acts if case.precision else None
        ref64 = MC.reference(case, m, x, dout, torch.float64, acts=given)
        ref32 = MC.reference(case, m, x, dout, torch.float32, acts=given)
        base = None
        if case.dx == 'accum':
            g = torch.Generator().manual_seed(rows + in_dim)
            base = (torch.randn(rows, in_dim, generator=g) * float(ref64['dx'].square().mean().sqrt())).float().to(DEV)
            ref64['dx'] = base.double() + ref64['dx']
            ref32['dx'] = base + ref32['dx']

        grads, dx, pins = _backward(hip, case, m, x, dout, acts, ws_case, base)
        _check_pins(case, pins)
        got = _outputs(case, grads, dx)
        assert sorted(got) == sorted(k for k in ref64 if k != 'out')
        for k, t in got.items():
            assert not bool(torch.isnan(t).any()), f'{case.name}: NaN left in {k}'
        if dx is not None and MC.lddx_of(case) > in_dim:
            assert bool((_bits(dx[:, in_dim:]) == SENT).all()), f'{case.name}: the padding columns of dx were written'
        assert bool(torch.isnan(x[:, in_dim:]).all()) and not bool(torch.isnan(x[:, :in_dim]).any())

        grads2, dx2, _ = _backward(hip, case, m, x, dout, acts, ws_case, base)
        _same_bits(case, got, _outputs(case, grads2, dx2), 'between two identical calls')
        if case.ws == 'no_copies':      # the same call with room for the bf16 W^T copies
            full = ws[:MC.ws_bytes_of(lib, case._replace(ws='ample'))]
            grads3, dx3, pins3 = _backward(hip, case, m, x, dout, acts, full, base)
            _check_pins(case._replace(ws='ample'), pins3)
            _same_bits(case, got, _outputs(case, grads3, dx3), 'between the transposed-scratch and the bf16-copies launch')

        report, failures = [], []
        for k in sorted(got, key=lambda n: (n != 'dx', n)):
            axes = ('row', 'feature') if k == 'dx' else ('out', 'in') if got[k].dim() == 2 else ('out',)
            try:
                R.check_tensor(k, got[k], ref64[k], ref32[k], axes, report)
            except AssertionError as e:
                failures.append(str(e))
        print(f'\n[MLP backward, {case.name}: {rows} rows, in {in_dim}+{case.pad}, hidden {case.hidden}, {case.layers} layers, out '
              f'{case.out_dim}, layer_norm {case.layer_norm}, precision {case.precision}, dx {case.dx}, workspace {case.ws}]')
        for name, err, err32, bar in report:
            ratio = err / max(err32, 1e-300)
            print(f'  {name:<10} err {err:.3e}  err_ref32 {err32:.3e}  err/err_ref32 {ratio:7.2f}  bar {bar:.3e}')
            print(f'[bars] {case.name} {name} {err:.3e} {err32:.3e} {ratio:.2f} {bar:.3e}')

        if case.precision:
            m.precision = 0
            grads32, dx32, _ = _backward(hip, case._replace(precision=0), m, x, dout, acts, ws, base)
            m.precision = case.precision
            path32 = _outputs(case, grads32, dx32)
            touched = MC.bf16_touched(case)
            for k in got:
                if k not in touched:
                    assert torch.equal(_bits(got[k]), _bits(path32[k])), f'{case.name}: {k} lies behind no rounded product but differs from the fp32 path'
                    continue
                err = float((got[k].double() - ref64[k]).abs().mean())
                gap = float((path32[k].double() - ref64[k]).abs().mean())
                print(f'  {k:<10} mean err {err:.3e}  fp32 path mean gap {gap:.3e}')
                if not err < 0.2 * gap:
                    failures.append(f'{k}: mean error {err:.3e} to the bf16-operand arithmetic, the fp32 path is {gap:.3e} away (bar 0.2)')
        assert not failures, f'{case.name}: ' + ' | '.join(failures)
    finally:
        m.precision = 0
