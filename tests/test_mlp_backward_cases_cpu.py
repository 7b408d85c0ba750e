"""CPU (-m "not gpu"): the case table of tests/test_gpu_mlp_backward.py (tests/mlp_backward_cases.py) against the library's own
backward plan, its branch coverage, and the hand-written backward the bf16 cases rely on against autograd in fp64.
"""
import os
import sys

import pytest
import torch

from oracle import dreamer_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/mlp_backward_cases.py
import mlp_backward_cases as MC                      # noqa: E402

DM_E_WORKSPACE = -2


@pytest.mark.parametrize('case', MC.CASES, ids=lambda c: c.name)
def test_table_agrees_with_the_plan(hip, case):
    """dm_mlp_plan_query(which = 1) runs the mlp_bwd_plan of a call: its path and its bf16_copies are the table's, on the
    workspace the case hands over; branch_of restates the same rules and gives the launches the row names."""
    lib = hip.lib()
    assert 1 <= case.layers <= MC.MAX_LAYERS and case.dx in ('none', 'write', 'accum') and case.ws in ('ample', 'no_copies')
    ws_bytes = MC.ws_bytes_of(lib, case)
    rc, path, copies, need = MC.plan_query(lib, case, ws_bytes)
    assert rc == 0, lib.dm_last_error()
    assert path == case.path == MC.path_of(case), (path, case.path, MC.path_of(case))
    assert copies == int(MC.copies_of(case)), (copies, MC.copies_of(case))
    assert MC.branch_of(case) == MC.expected_launches(case), (MC.branch_of(case), MC.expected_launches(case))
    hidden_branches = {b for b, _ in MC.branch_of(case)[1][1:]}
    assert (MC.BF16_COPIES in hidden_branches) == bool(copies)
    assert 4 * need <= ws_bytes
    if case.ws == 'no_copies':
        assert 4 * need == ws_bytes and MC.plan_query(lib, case, ws_bytes - 4)[0] == DM_E_WORKSPACE
        assert hidden_branches == {MC.BF16_WT}


def test_every_branch_is_reached():
    """Over the whole table: both backward paths, {fp32-vec, fp32-scalar} x {one k-tile, several}, both bf16 branches, every
    dx mode on either path, one layer and DM_MAX_MLP_LAYERS, a last panel of one row.  An edit of the table cannot drop one
    silently."""
    paths, launches, dx_modes = set(), set(), set()
    for c in MC.CASES:
        path, ls = MC.branch_of(c)
        paths.add(path)
        dx_modes.add((path, c.dx))
        launches |= {(b, 'one' if kt == 1 else 'several') for b, kt in ls}
    assert paths == {MC.PANEL, MC.PER_LAYER}
    want = {(b, n) for b in (MC.FP32_VEC, MC.FP32_SCALAR) for n in ('one', 'several')}
    want |= {(MC.BF16_COPIES, 'several'), (MC.BF16_WT, 'several')}
    assert launches == want, launches ^ want
    assert {(MC.PANEL, 'write'), (MC.PANEL, 'accum'), (MC.PANEL, 'none'), (MC.PER_LAYER, 'write'), (MC.PER_LAYER, 'accum')} <= dx_modes
    panel = [c for c in MC.CASES if MC.path_of(c) == MC.PANEL]
    assert {1, MC.MAX_LAYERS} <= {c.layers for c in panel}
    assert any(c.rows % MC.PANEL_BM == 1 for c in panel) and any(c.rows % MC.PANEL_BM == 0 for c in panel)
    assert any(c.pad % 4 for c in panel) and any(c.in_dim % 4 for c in panel)
    assert any(not c.layer_norm and c.dx != 'none' for c in MC.CASES) and any(c.rows == 1 for c in MC.CASES)
    assert {128, 400, 1024} <= {c.hidden for c in MC.CASES if MC.path_of(c) == MC.PER_LAYER}


def test_rounding_rule_of_the_bf16_cases():
    """backward_products on the bf16 rows: the output layer's data gradient stays fp32 (launched without scratch or copy), the
    hidden panels round, the GEMMs round where both operands take 16-byte loads - not the output layer's weight gradient at
    out_dim 6 or 255 (dout rows of 6 / 255 floats)."""
    for name in ('panel-bf16-copies', 'panel-bf16-nocopies', 'panel-bf16-out255', 'panel-bf16-L1'):
        c = MC.BY_NAME[name]
        got = {(n, l): (who, r) for n, l, who, _, r in MC.backward_products(c)}
        L = c.layers
        assert got[('wgrad', L)] == ('gemm', False) and got[('dgrad', L)] == ('panel', False)
        for l in range(L):
            assert got[('wgrad', l)] == ('gemm', True)
        for l in range(1, L):
            assert got[('dgrad', l)] == ('panel', True)
        assert got[('dgrad', 0)] == ('gemm', True)
        assert len(got) == 2 * L + 2
    for c in MC.CASES:
        if c.precision == 0:
            assert not any(r for *_, r in MC.backward_products(c))
    assert MC.gemm_rounds(1, 1, 32, 400, 16400, 32, 400) and not MC.gemm_rounds(1, 1, 400, 136, 16400, 400, 137)
    assert not MC.gemm_rounds(0, 1, 300, 400, 400, 400, 400) and MC.gemm_rounds(0, 1, 16400, 400, 400, 400, 400)      # skinny


SMALL = [
    MC.Case('small-ln', 37, 12, 3, 24, 3, 5, True, 0, 'write', 'ample', MC.PER_LAYER, None, None),
    MC.Case('small-nonorm', 37, 12, 0, 24, 2, 5, False, 0, 'accum', 'ample', MC.PER_LAYER, None, None),
    MC.Case('small-scalar-head', 19, 7, 1, 16, 1, 1, True, 0, 'write', 'ample', MC.PER_LAYER, None, None),
    MC.Case('small-no-dx', 5, 8, 0, 16, 4, 3, True, 0, 'none', 'ample', MC.PER_LAYER, None, None),
]


@pytest.mark.parametrize('case', SMALL, ids=lambda c: c.name)
def test_explicit_backward_equals_autograd(case):
    """precision = 0, fp64, CPU: reference()'s layer-by-layer backward against autograd through oracle.dreamer_oracle.mlp, every
    tensor to 1e-12 of its largest element - with the reference's own forward, and again with an activation set handed over in
    the library's layout (mlp_carve) in place of that forward."""
    m = MC.make_model(case, 'cpu')
    x, dout = MC.make_inputs(case, 'cpu')
    assert bool(torch.isnan(x[:, case.in_dim:]).all())
    p = {f'h.{k}': v.detach().double().requires_grad_(True) for k, v in m.model.state_dict().items()}
    xr = x[:, :case.in_dim].double().requires_grad_(True)
    out = O.mlp(p, 'h', xr, case.layers)
    out.backward(dout.double().reshape(out.shape))
    want = dict(zip(MC.grad_names(case), [p['h.' + n.replace('model.', '', 1)].grad for n, _ in m.named_parameters()]))
    want['out'] = out.detach().reshape(case.rows, case.out_dim)
    if case.dx != 'none':
        want['dx'] = xr.grad

    # the activation set in the library's layout, from a plain fp64 forward
    pre, ys, hcur = [], [], x[:, :case.in_dim].double()
    for l in range(case.layers):
        q = torch.nn.functional.linear(hcur, p[f'h.{3 * l}.weight'], p[f'h.{3 * l}.bias']).detach()
        pre.append(q)
        hcur = torch.nn.functional.elu(O._norm(p, f'h.{3 * l + 1}', q)).detach()
        ys.append(hcur)
    chunks = []
    for l in range(case.layers):
        for t in (pre[l], torch.full((case.rows, 2), float('nan'), dtype=torch.float64), ys[l]):
            flat = torch.full(((t.numel() + 63) // 64 * 64,), float('nan'), dtype=torch.float64)
            flat[:t.numel()] = t.reshape(-1)
            chunks.append(flat)
    acts = torch.cat(chunks)
    assert acts.numel() == MC.acts_floats(case)

    for given in (None, acts):
        got = MC.reference(case, m, x, dout, torch.float64, acts=given)
        assert sorted(got) == sorted(want), (sorted(got), sorted(want))
        for k, w in want.items():
            assert got[k].shape == w.shape, (k, got[k].shape, w.shape)
            err = float((got[k] - w).abs().max()) / float(w.abs().max())
            assert err <= 1e-12, (k, 'acts given' if given is not None else 'own forward', err)


def test_acts_layout_matches_the_library(hip):
    for case in MC.CASES:
        assert MC.acts_floats(case) == hip.lib().dm_mlp_acts_floats(case.rows, case.hidden, case.layers), case.name
