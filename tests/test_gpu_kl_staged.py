"""-m gpu: the LDS-staged categorical KL-balance kernels (dm_kl_staged_enable, csrc/elementwise.hip: a workgroup of 128 threads
copies 128 consecutive groups of both tensors into LDS with coalesced 16-byte loads, a lane then works on its group there; the
forward gives a wave two rows at S <= 32; the backward returns both gradients through LDS) against the per-lane-addressed kernels
(switch off) and against OneHotCategorical in fp64, through dm_kl_balance_fwd / dm_kl_balance_bwd.

Shapes (rows, S, C):
  (1 | 3 | 5 | 9, 32, 32)   the workload's group shape, at row counts around the four rows a workgroup owns in both kernels
  (3, 32, 63), (3, 32, 64)  the two sides of the admission bound C <= 63 (2 tensors x 128 groups x (C + 1) floats = 64 KB of LDS)
  (5, 33, 8)                S = 33: the forward keeps its wave-per-row kernel (the staged one gives a wave two rows of <= 32
                            groups), the backward, flat over groups, is staged
  (3, 5, 7)                 105 floats: a run that is not a whole number of 16-byte loads, groups that straddle them, S < 32
Per shape: all five outputs (kl, both entropies, both gradients) equal under `==` between switch on and off - the staged kernels
run the same expressions in the same order, and a row's reduction tree keeps its shape - and within the bounds of
tests/test_gpu_distributions.py::test_kl_balance_categorical_shapes (copied below) of the fp64 reference.  Outputs are NaN-filled
before each call.  One more case hands the kernels pointers that are 4 bytes off a 16-byte boundary (the scalar copy path).
"""
import pytest
import torch
import torch.distributions as D

pytestmark = pytest.mark.gpu

DEV = 'cuda'
_EPS = 2.0 ** -23                 # fp32 machine epsilon: ulp(v) <= _EPS * |v|
NAN = float('nan')
SHAPES = [(1, 32, 32), (3, 32, 32), (5, 32, 32), (9, 32, 32), (3, 32, 63), (3, 32, 64), (5, 33, 8), (3, 5, 7)]


def _rand(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _close(a, b, tol, what=''):
    """|a - b| <= tol element-wise (tol a tensor or a scalar); prints the worst err/tol ratio so runs can report it."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(b)
    err = (a - b).abs()
    bad = ~(err <= tol)                              # NaN in a or b fails
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f'[tol] {what}: max err {float(err.max()) if err.numel() else 0:.3e}, worst err/tol {ratio:.3f}')
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e}, ' \
                          f'worst err/tol {ratio:.3e}'


def _cat_mags(a, b):
    """Per (row, group, k): p, q, log p, log q and the fp32 error scale of log p and log q (|x_k| + |lse|)."""
    la, lb = a.logsumexp(-1, keepdim=True), b.logsumexp(-1, keepdim=True)
    lp, lq = a - la, b - lb
    ea, eb = a.abs() + la.abs(), b.abs() + lb.abs()
    return lp.exp(), lq.exp(), lp, lq, ea, eb


def _launch(hip, rows, S, C, post, prior, sp, sq):
    """Both entry points into NaN-filled outputs; post / prior: (rows, S*C) views, contiguous."""
    out = {k: torch.full((rows,), NAN, device=DEV) for k in ('kl', 'ent_post', 'ent_prior')}
    hip.call('dm_kl_balance_fwd', rows, S, C, hip.fptr(post), hip.fptr(prior), hip.fptr(out['kl']), hip.fptr(out['ent_post']),
             hip.fptr(out['ent_prior']), hip.stream())
    out['dpost'] = torch.full((rows, S * C), NAN, device=DEV)
    out['dprior'] = torch.full((rows, S * C), NAN, device=DEV)
    hip.call('dm_kl_balance_bwd', rows, S, C, hip.fptr(post), hip.fptr(prior), sp, sq, hip.fptr(out['dpost']),
             hip.fptr(out['dprior']), hip.stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _on_and_off(hip, rows, S, C, post, prior, sp, sq):
    lib = hip.lib()
    assert lib.dm_kl_staged_enable(-1) == 1, 'the staged kernels are on by default'
    try:
        on = _launch(hip, rows, S, C, post, prior, sp, sq)
        assert lib.dm_kl_staged_enable(0) == 0
        off = _launch(hip, rows, S, C, post, prior, sp, sq)
    finally:
        lib.dm_kl_staged_enable(1)
    for k in on:
        assert bool(torch.isfinite(on[k]).all()), f'({rows}, {S}, {C}): {k} holds a non-finite value (an element not written?)'
    differ = [f'{k} ({int((on[k] != off[k]).sum())} elements)' for k in on if not bool((on[k] == off[k]).all())]
    assert not differ, f'({rows}, {S}, {C}): {differ} differ between the staged and the per-lane-addressed kernels'
    return on


def _check_fp64(rows, S, C, post, prior, sp, sq, got):
    def dist(x):
        return D.Independent(D.OneHotCategorical(logits=x.reshape(rows, S, C), validate_args=False), 1, validate_args=False)
    a = post.double().cpu().requires_grad_(True)
    b = prior.double().cpu().requires_grad_(True)
    with torch.no_grad():
        p, q, lp, lq, ea, eb = _cat_mags(a.reshape(rows, S, C), b.reshape(rows, S, C))
        kl_g = (p * (lp - lq)).sum(-1, keepdim=True)
        gmag = p * (ea + eb) * (1 + (lp - lq).abs())
        c = 8 + C + S
        _close(got['kl'], D.kl_divergence(dist(a), dist(b)), c * _EPS * gmag.sum((1, 2)), 'kl')
        _close(got['ent_post'], dist(a).entropy(), c * _EPS * (p * ea * (1 + lp.abs())).sum((1, 2)), 'entropy post')
        _close(got['ent_prior'], dist(b).entropy(), c * _EPS * (q * eb * (1 + lq.abs())).sum((1, 2)), 'entropy prior')
    loss = sp * D.kl_divergence(dist(a), dist(b.detach())) + sq * D.kl_divergence(dist(a.detach()), dist(b))
    loss.sum().backward()
    tol_p = (8 + C) * _EPS * sp * (p * (ea + eb) * (1 + (lp - lq).abs() + kl_g.abs()) + p * gmag.sum(-1, keepdim=True))
    tol_q = 8 * _EPS * sq * (q * eb + p * ea)
    _close(got['dpost'], a.grad, tol_p.reshape(rows, -1), 'dpost')
    _close(got['dprior'], b.grad, tol_q.reshape(rows, -1), 'dprior')


@pytest.mark.parametrize('rows,S,C', SHAPES)
def test_kl_staged_equals_per_lane_and_matches_fp64(hip, rows, S, C):
    post = _rand(rows, S * C, seed=S + C, scale=2.0)
    prior = _rand(rows, S * C, seed=S + C + 1, scale=2.0)
    sp, sq = 0.2 / rows, 0.8 / rows * 1.1
    got = _on_and_off(hip, rows, S, C, post, prior, sp, sq)
    _check_fp64(rows, S, C, post, prior, sp, sq, got)


def test_kl_staged_inputs_off_a_16_byte_boundary(hip):
    rows, S, C = 5, 32, 32
    n = rows * S * C
    post = _rand(n + 1, seed=101, scale=2.0)[1:].view(rows, S * C)
    prior = _rand(n + 1, seed=102, scale=2.0)[1:].view(rows, S * C)
    assert post.data_ptr() % 16 == 4 and prior.data_ptr() % 16 == 4
    sp, sq = 0.2 / rows, 0.8 / rows * 1.1
    got = _on_and_off(hip, rows, S, C, post, prior, sp, sq)
    _check_fp64(rows, S, C, post, prior, sp, sq, got)
