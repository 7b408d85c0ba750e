"""-m gpu: Plan2Explore - the two kernels of csrc/disag.hip against float64 on the same fp32 inputs, the ensemble step
and the intrinsic reward of explore.Plan2Explore against a float64 torch restatement written here, the exploration actor-critic's
inputs, bit-identity of the Dreamer's own step beside it, acting with the exploration actor, and the trainer loop.

Kernel tolerances are first-order rounding bounds, u = 2^-24, derived in the docstrings of the two kernel tests from the operation
order csrc/disag.hip states; `_close` prints err / tol.  The step bars are those tests/test_gpu_goals_probe.py holds the same MLP
kernels to."""
import ast
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dreamer_oracle as O
from pydreamer_amd import config

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
U = 2.0 ** -24
NAN = float('nan')
KS = [2, 3, 10, 16]
DS = [1, 5, 63, 64, 65, 1024]
ROWS = [1, 63, 64, 65, 257]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, ref, tol, what):
    """|got - ref| <= tol element-wise (NaN fails); prints the worst err / tol."""
    got, ref, tol = got.detach().double().cpu(), ref.double().cpu(), tol.double().cpu()
    err = (got - ref).abs()
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f'[tol] {what}: max err {float(err.max()) if err.numel() else 0.0:.3e}, worst err/tol {ratio:.3f}')
    assert not torch.isnan(got).any(), f'{what}: NaN in the result'
    assert not (err > tol).any(), f'{what}: {int((err > tol).sum())}/{err.numel()} above the bound, worst err/tol {ratio:.3f}'
    return ratio


def _r4(n):
    return (n + 3) // 4 * 4


def _layouts(rows, D):
    """(name, ld, head_stride, ldt, target column offset): dense; odd padding (rows lose their 16-byte alignment: the one-float-
    per-lane walk); padding in multiples of four floats (aligned rows with D % 4 columns left over: 16-byte walk and tail)."""
    return [('dense', D, rows * D, D, 0), ('odd', D + 3, rows * (D + 3) + 7, D + 5, 3),
            ('aligned', _r4(D) + 4, rows * (_r4(D) + 4) + 8, _r4(D) + 8, 4)]


def _heads(K, rows, D, ld, stride, values):
    """values (K, rows, D) placed into a NaN-filled buffer with the given layout; returns the flat device buffer."""
    buf = torch.full(((K - 1) * stride + rows * ld + 5,), NAN)
    for k in range(K):
        buf[k * stride:k * stride + rows * ld].view(rows, ld)[:, :D] = values[k]
    return buf.to(DEV)


def _pad_mask(K, rows, D, ld, stride, n):
    m = torch.ones(n, dtype=torch.bool)
    for k in range(K):
        m[k * stride:k * stride + rows * ld].view(rows, ld)[:, :D] = False
    return m


# ------------------------------------------------------------------------------------------------ dm_disag_reward
def _disag_ref_and_tol(m32, scale):
    """m32 (K, rows, D) fp32 -> (float64 reference (rows,), first-order bound (rows,)); see test_disag_reward_against_fp64."""
    K, rows, D = m32.shape
    m = m32.double()
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    sig = m.std(0, unbiased=False)                                # (rows, D)
    X = (m - m[:1]).abs().amax(0)                                 # max_k |m_k - m_0|
    ref = s32 * sig.mean(-1)
    n_lane = -(-D // 64)
    tol = abs(s32) / D * U * (((K + 4) * X + (K / 2 + 2) * sig).sum(-1) + (n_lane + 7) * sig.sum(-1))
    return ref, tol


def _disag(hip, K, rows, D, buf, stride, ld, scale):
    out = torch.full((rows + 2,), -7.0, device=DEV)
    hip.call('dm_disag_reward', K, rows, D, hip.fptr(buf), stride, ld, scale, hip.fptr(out), hip.stream())
    torch.cuda.synchronize()
    assert out[rows:].tolist() == [-7.0, -7.0], 'written past rows floats'
    return out[:rows].cpu()


@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('K', KS)
def test_disag_reward_against_fp64(hip, K, D):
    """reward[r] = scale (1/D) sum_d sqrt((1/K) sum_k (x_k - mu)^2) against torch.std(0, unbiased=False).mean(-1) in float64 on the
    same fp32 means, rows in {1, 63, 64, 65, 257}, three layouts (ld > D, head_stride > rows ld; the padding is NaN and must not
    reach a result), data (a) N(0,1) and (b) the cancellation case: a common value of 1e3 per column plus deviations of 1e-2.

    Bound, first order in u = 2^-24, per column with X = max_k |m_k - m_0| and sigma the exact std:
      x_k = fl(m_k - m_0): |error| <= u X (zero when Sterbenz applies);  mu = fl(fl(sum_k x_k) / K): K - 1 additions and the
      division, |error| <= K u X;  c_k = fl(x_k - mu), |x_k - mu| <= 2 X: 2 u X.  So c_k = (x_k - mean x) + g_k with
      |g_k| <= (1 + 1 + K + 2) u X = (K + 4) u X, and since  c -> ||c|| / sqrt(K)  is 1-Lipschitz in max|.|, the std moves by at most
      (K + 4) u X - an ABSOLUTE bound, no division by sigma;
      the evaluation of sqrt(fl(sum_k c_k^2) / K): squares 1, K - 1 additions, division 1 -> (K + 1) u relative under the root, halved
      by it, plus the root's own rounding: (K / 2 + 2) u sigma.
    Over the columns: a lane adds its ceil(D / 64) columns in sequence, six butterfly levels, the division by D, the product with
    scale: (ceil(D / 64) + 7) u sum_d sigma_d.  tol = |scale| / D * u * (sum_d ((K + 4) X_d + (K / 2 + 2) sigma_d) +
    (ceil(D / 64) + 7) sum_d sigma_d).

    (b): X ~ 3e-2, sigma ~ 1e-2, so tol ~ 1e-8 on a reward of 1e-2.  A one-pass E[x^2] - mu^2 squares 1e3: each x^2 ~ 1e6 carries a
    rounding error of u 1e6 = 6e-2 - 600 times the variance 1e-4 it is supposed to resolve.  The test evaluates that formula in fp32
    on the host and asserts that it misses the bound the kernel meets.

    Also: a second call gives the same bits; scale is applied (scale 1 vs 0.37 vs -2: the outputs are fl(scale * q) of one q)."""
    worst = 0.0
    for rows in ROWS:
        for case in ('normal', 'cancel'):
            g = _gen(7000 + 100 * K + D + 13 * rows + (case == 'cancel'))
            if case == 'normal':
                vals = torch.randn(K, rows, D, generator=g)
            else:
                vals = (1e3 + 50.0 * torch.randn(1, rows, D, generator=g)) + 1e-2 * torch.randn(K, rows, D, generator=g)
            vals = vals.float()
            for name, ld, stride, _, _ in _layouts(rows, D):
                buf = _heads(K, rows, D, ld, stride, vals)
                scale = 0.37 if name == 'odd' else 1.0
                got = _disag(hip, K, rows, D, buf, stride, ld, scale)
                assert torch.equal(got.view(torch.int32), _disag(hip, K, rows, D, buf, stride, ld, scale).view(torch.int32))
                ref, tol = _disag_ref_and_tol(vals, scale)
                worst = max(worst, _close(got, ref, tol, f'disag K={K} D={D} rows={rows} {case} {name}'))
                if name == 'dense':
                    q = _disag(hip, K, rows, D, buf, stride, ld, 1.0)
                    for s in (0.37, -2.0):
                        want = (torch.tensor(s, dtype=torch.float32) * q)
                        assert torch.equal(_disag(hip, K, rows, D, buf, stride, ld, s), want), f'scale {s} is not applied as scale * q'
            if case == 'cancel' and rows == 257:
                v = vals.numpy().astype(np.float32)
                one_pass = np.sqrt(np.maximum((v * v).mean(0, dtype=np.float32) - v.mean(0, dtype=np.float32) ** 2, 0)).mean(-1)
                ref, tol = _disag_ref_and_tol(vals, 1.0)
                miss = float((torch.from_numpy(one_pass).double() - ref).abs().max() / tol.max())
                print(f'[one-pass] K={K} D={D}: the fp32 E[x^2] - mu^2 form is off by {miss:.1f} x the bound')
                assert miss > 100.0
    print(f'[worst] disag K={K} D={D}: err/tol {worst:.3f}')


@pytest.mark.parametrize('K', KS)
def test_identical_heads_give_exactly_zero(hip, K):
    for rows, D in ((1, 1), (65, 63), (257, 1024), (64, 65)):
        one = (1e3 * torch.randn(1, rows, D, generator=_gen(rows + D))).float()
        for name, ld, stride, _, _ in _layouts(rows, D):
            got = _disag(hip, K, rows, D, _heads(K, rows, D, ld, stride, one.expand(K, rows, D)), stride, ld, 3.0)
            assert torch.equal(got, torch.zeros(rows)), (K, rows, D, name, got.abs().max())


# ------------------------------------------------------------------------------------------------ dm_ensemble_mse
def _mse(hip, K, rows, D, buf, stride, ld, tgt, ldt, off, skip, scale, want_d=True):
    loss = torch.full((K * rows + 2,), -7.0, device=DEV)
    dm = torch.full((buf.numel(),), -7.0, device=DEV) if want_d else None
    hip.call('dm_ensemble_mse', K, rows, D, hip.fptr(buf), stride, ld, hip.fptr(tgt[off:]), ldt, hip.ptr(skip), scale, hip.fptr(loss),
             hip.fptr(dm), hip.stream())
    torch.cuda.synchronize()
    assert loss[K * rows:].tolist() == [-7.0, -7.0], 'loss written past K * rows floats'
    return loss[:K * rows].view(K, rows).cpu(), None if dm is None else dm.cpu()


@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('K', KS)
def test_ensemble_mse_against_fp64(hip, K, D):
    """loss[k][r] = 0.5 sum_d (m_k - y)^2 and dmeans = scale (m_k - y) against float64, rows in {1, 63, 64, 65, 257}, three layouts;
    the target lies inside a wider NaN-filled matrix (ldt > D) at a column offset; the padding of means is NaN; dmeans' padding
    keeps its sentinel.
    Bound: e = fl(m - y) 1 rounding, doubled by the square, the square 1: 3 u per term; a lane adds at most ceil(D / 64) + 4 terms
    (the 16-byte walk: four per step, one tail column) in sequence, six butterfly levels; 0.5 x is exact:
      tol_loss = (ceil(D / 64) + 13) u * 0.5 sum_d e^2.   dmeans = fl(scale fl(m - y)), two roundings and nothing else: tol = (2 u + u^2) |scale (m - y)|, exact.
    skip rows: loss and dmeans exactly zero though their means and target rows are NaN (nothing of them is read); skip = NULL
    equals an all-false skip bit for bit; dmeans = NULL leaves the loss bits; a second call gives the same bits."""
    worst = 0.0
    scale = 1.0 / 7.0
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    for rows in ROWS:
        g = _gen(9000 + 100 * K + D + 13 * rows)
        vals = torch.randn(K, rows, D, generator=g).float()
        y = (vals.mean(0) + 0.5 * torch.randn(rows, D, generator=g)).float()
        skipped = torch.rand(rows, generator=g) < 0.3
        for name, ld, stride, ldt, off in _layouts(rows, D):
            what = f'mse K={K} D={D} rows={rows} {name}'
            buf = _heads(K, rows, D, ld, stride, vals)
            tgt = torch.full((rows * ldt + off + 3,), NAN)
            tgt[off:off + rows * ldt].view(rows, ldt)[:, :D] = y
            tgt = tgt.to(DEV)
            none = torch.zeros(rows, dtype=torch.bool, device=DEV)
            loss, dm = _mse(hip, K, rows, D, buf, stride, ld, tgt, ldt, off, none, scale)
            loss2, dm2 = _mse(hip, K, rows, D, buf, stride, ld, tgt, ldt, off, None, scale)
            assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(dm.view(torch.int32), dm2.view(torch.int32)), \
                f'{what}: skip = NULL differs from an all-false skip'
            loss3, _ = _mse(hip, K, rows, D, buf, stride, ld, tgt, ldt, off, None, scale, want_d=False)
            assert torch.equal(loss.view(torch.int32), loss3.view(torch.int32)), f'{what}: dmeans = NULL changes the loss'
            e = vals.double() - y.double()
            tol_loss = (-(-D // 64) + 13) * U * 0.5 * (e * e).sum(-1)
            worst = max(worst, _close(loss, 0.5 * (e * e).sum(-1), tol_loss + 1e-300, what + ' loss'))
            pad = _pad_mask(K, rows, D, ld, stride, buf.numel())
            assert bool((dm[pad] == -7.0).all()), f'{what}: dmeans written outside the (rows, D) blocks'
            got_d = torch.stack([dm[k * stride:k * stride + rows * ld].view(rows, ld)[:, :D] for k in range(K)])
            worst = max(worst, _close(got_d, s32 * e, 2 * U * (1 + U) * (s32 * e).abs() + 1e-300, what + ' dmeans'))
            # skipped rows: poisoned means and targets, exact zeros out, the other rows keep their bits
            vals_p, y_p = vals.clone(), y.clone()
            vals_p[:, skipped], y_p[skipped] = NAN, NAN
            buf_p = _heads(K, rows, D, ld, stride, vals_p)
            tgt_p = torch.full((rows * ldt + off + 3,), NAN)
            tgt_p[off:off + rows * ldt].view(rows, ldt)[:, :D] = y_p
            loss_s, dm_s = _mse(hip, K, rows, D, buf_p, stride, ld, tgt_p.to(DEV), ldt, off, skipped.to(DEV), scale)
            got_s = torch.stack([dm_s[k * stride:k * stride + rows * ld].view(rows, ld)[:, :D] for k in range(K)])
            assert bool((loss_s[:, skipped] == 0).all()) and bool((got_s[:, skipped] == 0).all()), f'{what}: skipped rows are not zero'
            keep = ~skipped
            assert torch.equal(loss_s[:, keep].view(torch.int32), loss[:, keep].view(torch.int32)), what
            assert torch.equal(got_s[:, keep].view(torch.int32), got_d[:, keep].view(torch.int32)), what
            assert bool((dm_s[pad] == -7.0).all())
    print(f'[worst] mse K={K} D={D}: err/tol {worst:.3f}')


# ------------------------------------------------------------------------------------------------ the module on the tiny model
K_TINY = 3


def _hip_conf(oconf, **more):
    return config.load_config('defaults', 'atari', **{**{k: getattr(oconf, k) for k in vars(oconf)}, 'disag_models': K_TINY, **more})


def _dreamer(oconf, conf, overlap=True):
    from pydreamer_amd.models import Dreamer
    model = Dreamer(conf)
    model.load_state_dict(O.make_params(oconf), strict=True)
    model = model.to(DEV)
    model.overlap_backward = overlap
    return model


def _explorer(conf, model, state=None, seed=11):
    from pydreamer_amd.explore import Plan2Explore
    torch.manual_seed(seed)
    p = Plan2Explore(conf, model)
    if state is not None:
        p.load_state_dict(state)
    else:
        with torch.no_grad():      # non-trivial LayerNorm parameters and biases
            gen = _gen(seed)
            for n, v in p.named_parameters():
                if v.dim() == 1:
                    v.add_(0.1 * torch.randn(v.shape, generator=gen))
    return p.to(DEV)


def _batch(oconf, seed=1234):
    """The oracle's synthetic batch (a reset at (T // 2, B - 1), inside the window) with one more reset in the LAST row, column 1: that
    row is a target only, never an input."""
    raw = O.synthetic_batch(oconf, seed=seed)
    raw['reset'][oconf.batch_length - 1, 1] = True
    obs = {k: v.to(DEV) for k, v in O.preprocess(raw, oconf).items()}
    noise = {k: v.to(DEV) for k, v in O.make_noise(oconf).items()}
    return obs, noise


def _expl_noise(oconf, seed=4242):
    n = O.make_noise(oconf, seed=seed)
    return {k: n[k].to(DEV) for k in ('u_act', 'u_prior')}


def _mlp64(head, x):
    """Linear -> LayerNorm(eps 1e-3) -> ELU, four times, then Linear: float64 torch on the head's own weights; returns (output,
    the float64 leaf parameters in parameters() order)."""
    ps = [p.detach().double().cpu().requires_grad_(True) for p in head.parameters()]
    it = iter(ps)
    y = x
    for _ in range(head.hidden_layers):
        w, b = next(it), next(it)
        y = F.linear(y, w, b)
        if head.layer_norm:
            gamma, beta = next(it), next(it)
            y = F.layer_norm(y, (y.shape[-1],), gamma, beta, 1e-3)
        y = F.elu(y)
    w, b = next(it), next(it)
    return F.linear(y, w, b), ps


def _dreamer_step(model, opts, obs, noise, state):
    losses, state, _, _, _ = model.training_step(obs, state, noise=noise)
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    return losses, state


def test_ensemble_step_against_fp64_autograd(hip):
    """tiny oracle config, T 5, B 3, K 3, resets at (2, 2) and (4, 1).  loss_disag and every head's parameter gradients against a
    float64 autograd restatement on the step's own fp32 feature matrix: rows (t, b), t < T - 1, are [feat_t | action_{t+1}], the
    target is the stochastic part of feat_{t+1}, rows with reset[t+1] are left out, loss = sum_k (1/N) sum_r 0.5 |m_k - y|^2 with
    N = (T - 1) B.  Bars of tests/test_gpu_goals_probe.py: loss 2e-5 relative or 2e-6 absolute, each gradient 2e-3 relative L2.
    Then the masked target row (4, 1) - a target only - is overwritten with garbage: loss and gradients keep their bits."""
    oconf = O.tiny_conf()
    conf = _hip_conf(oconf)
    model = _dreamer(oconf, conf)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    p2e = _explorer(conf, model)
    eopts = p2e.init_optimizers()
    obs, noise = _batch(oconf)
    T, B, A, Dd = oconf.batch_length, oconf.batch_size, oconf.action_dim, oconf.deter_dim
    assert (T, B, p2e.K) == (5, 3, 3) and bool(obs['reset'][2, 2]) and bool(obs['reset'][4, 1])
    _dreamer_step(model, opts, obs, noise, model.init_state(B))
    feat = p2e.step_features()
    assert feat is model.wm._last_pack['feat'] and feat.shape == (T * B, p2e.features_dim) and not feat.requires_grad

    def run():
        (loss, _, _), metrics = p2e.training_step(noise=_expl_noise(oconf))
        for opt in eopts:
            opt.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), [p.grad.detach().clone() for p in p2e.ensemble.parameters()], metrics

    loss, grads, metrics = run()
    assert float(metrics['loss_disag']) == float(loss)
    N = (T - 1) * B
    f64 = feat.double().cpu()
    x = torch.cat((f64[:N], obs['action'].double().cpu().view(T * B, A)[B:]), -1)
    y = f64[B:, Dd:]
    keep = (~obs['reset'].cpu().view(T * B)[B:]).double()
    assert int((keep == 0).sum()) == 2
    ref, leaves = 0.0, []
    for head in p2e.heads:
        m, ps = _mlp64(head, x)
        ref = ref + (0.5 * ((m - y) ** 2).sum(-1) * keep).sum() / N
        leaves += ps
    ref.backward()
    ref = ref.detach()
    rel = abs(float(loss) - float(ref)) / abs(float(ref))
    print(f'loss_disag {float(loss):.9g} float64 {float(ref):.9g} rel {rel:.2e}')
    assert rel < 2e-5 or abs(float(loss) - float(ref)) < 2e-6
    assert len(grads) == len(leaves) == K_TINY * 18
    for (name, _), g, leaf in zip(p2e.ensemble.named_parameters(), grads, leaves):
        e = float((g.double().cpu() - leaf.grad).norm() / leaf.grad.norm())
        print(f'gradient {name}: relative L2 error {e:.3e}')
        assert e < 2e-3, (name, e)
    # garbage in the masked target (finite: the row also starts an imagined rollout; NaN targets are the kernel test's)
    feat[(T - 1) * B + 1, Dd:] = 7.5
    feat[(T - 1) * B + 1, Dd::3] = -3.25
    loss_g, grads_g, _ = run()
    assert torch.equal(loss_g.view(torch.int32), loss.view(torch.int32))
    for a, b in zip(grads, grads_g):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with torch.no_grad():      # the loss without a graph, the same bits, nothing kept for a backward
        feat[(T - 1) * B + 1, Dd:] = 0.0
        (l0, _, _), _ = p2e.training_step(noise=_expl_noise(oconf))
    assert not l0.requires_grad and float(l0) == float(loss)


def _setup(extr=0.0, intr=1.0, state=None, overlap=True, explorer=True):
    oconf = O.tiny_conf()
    conf = _hip_conf(oconf, expl_extr_scale=extr, expl_intr_scale=intr)
    model = _dreamer(oconf, conf, overlap)
    opts = list(model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps))
    p2e = None
    if explorer:
        p2e = _explorer(conf, model, state)
        p2e.init_optimizers()
    return oconf, conf, model, opts, p2e


def test_intrinsic_reward_end_to_end(hip):
    """With explicit noise, the (H+1, M) rewards are rebuilt from the step's own imagined features and actions: rows
    [feat_i | action_i], i < H, through the float64 heads, std over the heads (ddof 0), mean over the columns, at row i + 1; row 0 is
    zero.  (1) The kernel alone: against float64 on the fp32 means the heads give for those rows (Plan2Explore.predict, the same
    calls), within the bound of test_disag_reward_against_fp64.  (2) End to end against the float64 heads: that bound widened by the
    measured fp32 forward error - the std over the heads is 1-Lipschitz in max_k |.|, so by mean_d max_k |m32 - m64| per row; both
    terms and the margin are printed.  (3) expl_extr_scale = 0.5 on the same weights and noise adds exactly 0.5 x the reward head's
    means."""
    oconf, conf, model, opts, p2e = _setup()
    obs, noise = _batch(oconf)
    B = oconf.batch_size
    _dreamer_step(model, opts, obs, noise, model.init_state(B))
    _, metrics = p2e.training_step(noise=_expl_noise(oconf))
    ex = p2e.last_extras
    feats, actions, rewards = ex['dream_features'], ex['actions'], ex['rewards']
    Hh, M = actions.shape[:2]
    assert rewards.shape == (Hh + 1, M) == (oconf.imag_horizon + 1, oconf.batch_length * B)
    assert bool((rewards[0] == 0).all()) and bool((rewards[1:] > 0).all())
    f2, a2 = feats[:-1].reshape(Hh * M, -1), actions.reshape(Hh * M, -1)
    m32 = p2e.predict(f2.contiguous(), a2.contiguous()).cpu()
    ref_k, tol_k = _disag_ref_and_tol(m32, 1.0)
    got = rewards[1:].reshape(-1).cpu()
    _close(got, ref_k, tol_k, 'intrinsic reward against float64 on the fp32 means')
    x = torch.cat((f2.double().cpu(), a2.double().cpu()), -1)
    with torch.no_grad():
        m64 = torch.stack([_mlp64(h, x)[0] for h in p2e.heads])
    ref = m64.std(0, unbiased=False).mean(-1)
    widen = (m32.double() - m64).abs().amax(0).mean(-1)
    ratio = _close(got, ref, tol_k + widen, 'intrinsic reward against the float64 heads')
    print(f'[e2e] kernel bound max {float(tol_k.max()):.3e}, measured forward error max {float(widen.max()):.3e} on rewards of '
          f'{float(ref.mean()):.3e}; margin x{1 / max(ratio, 1e-12):.1f}')
    assert float(widen.max()) < 1e-4 * float(m64.abs().max()), 'the fp32 heads are further from float64 than an fp32 MLP should be'
    n = Hh * M
    mean64, std64 = got.double().mean(), got.double().std(unbiased=True)      # of the kernel's own rows: n 2^-23 max|x| covers any order
    assert abs(float(metrics['expl_reward']) - float(mean64)) <= n * 2 * U * float(got.abs().max())
    assert abs(float(metrics['expl_reward_std']) - float(std64)) <= 1e-4 * float(std64) and n > 1
    # (3)
    _, _, model2, opts2, p2e2 = _setup(extr=0.5, state={k: v.cpu() for k, v in p2e.state_dict().items()})
    _dreamer_step(model2, opts2, obs, noise, model2.init_state(B))
    p2e2.training_step(noise=_expl_noise(oconf))
    ex2 = p2e2.last_extras
    assert torch.equal(ex2['dream_features'], feats) and torch.equal(ex2['reward_pred'], ex['reward_pred'])
    assert float(ex['reward_pred'].abs().max()) > 0
    assert torch.equal(ex2['rewards'], rewards + 0.5 * ex['reward_pred'])
    assert bool((ex2['rewards'][0] == 0.5 * ex['reward_pred'][0]).all())


def test_exploration_actor_critic_trains_on_the_intrinsic_reward(hip):
    """value_target and the GAE advantage of the exploration actor-critic are dm_gae_losses of the intrinsic rewards (checked
    against float64 in test_intrinsic_reward_end_to_end), the imagined terminals and its own target network's values, bit for bit -
    and not those of the extrinsic reward.  expl_intr_scale = 2 doubles policy_reward of the explore buffer exactly, and the
    Dreamer's own metric buffer keeps its bits."""
    oconf, conf, model, opts, p2e = _setup()
    obs, noise = _batch(oconf)
    B = oconf.batch_size
    _dreamer_step(model, opts, obs, noise, model.init_state(B))
    own = model.metric_buffer.clone()
    _, metrics = p2e.training_step(noise=_expl_noise(oconf))
    ex = p2e.last_extras
    Hh, M = ex['actions'].shape[:2]

    def gae(rewards):
        out = [torch.empty(Hh, M, device=DEV) for _ in range(4)]
        hip.call('dm_gae_losses', Hh, M, p2e.ac.gamma, p2e.ac.lambda_, hip.fptr(rewards.contiguous()), hip.fptr(ex['terminal_pred'].contiguous()),
                 hip.fptr(ex['values']['value_t']), *[hip.fptr(o) for o in out], hip.stream())
        return out      # adv, agae, vtgt, wgt
    adv, agae, vtgt, wgt = gae(ex['rewards'])
    t = ex['ac_tensors']
    assert torch.equal(t['value_target'], vtgt) and torch.equal(t['value_advantage_gae'], agae) and torch.equal(t['value_advantage'], adv)
    _, agae_x, vtgt_x, _ = gae(ex['reward_pred'])
    assert not torch.equal(vtgt_x, vtgt) and not torch.equal(agae_x, agae)
    assert float(metrics['expl_policy_reward']) == float(p2e.metric_buffer[13]) > 0
    _, _, model2, opts2, p2e2 = _setup(intr=2.0, state={k: v.cpu() for k, v in p2e.state_dict().items()})
    _dreamer_step(model2, opts2, obs, noise, model2.init_state(B))
    own2 = model2.metric_buffer.clone()
    _, metrics2 = p2e2.training_step(noise=_expl_noise(oconf))
    torch.cuda.synchronize()
    assert float(metrics2['expl_policy_reward']) == 2.0 * float(metrics['expl_policy_reward'])
    assert float(metrics2['expl_reward']) == 2.0 * float(metrics['expl_reward'])
    assert torch.equal(p2e2.last_extras['rewards'], 2.0 * ex['rewards'])
    for a, b, m in ((own, model.metric_buffer, model), (own2, model2.metric_buffer, model2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'the exploration step wrote into the Dreamer\'s metric buffer'
    assert torch.equal(own.view(torch.int32), own2.view(torch.int32))
    assert model.metric_buffer.data_ptr() != p2e.metric_buffer.data_ptr() and p2e.metric_buffer.numel() == 48


# ------------------------------------------------------------------------------------------------ non-interference
def _iterations(overlap, mode, n=2):
    """n trainer iterations of the tiny model; mode 'alone': the Dreamer only; 'built': a Plan2Explore exists but is never called;
    'both': training_step -> p2e.training_step -> all seven backward() -> clips -> steps.  Returns per iteration the Dreamer's
    losses, flat gradients and flat parameters."""
    oconf, conf, model, opts, p2e = _setup(overlap=overlap, explorer=mode != 'alone')
    eopts = list(p2e._opt.values()) if mode == 'both' else []
    obs, noise = _batch(oconf)
    state = model.init_state(oconf.batch_size)
    out = []
    for it in range(n):
        losses, state, _, _, _ = model.training_step(obs, state, noise=noise)
        elosses = ()
        if mode == 'both':
            elosses, _ = p2e.training_step(noise=_expl_noise(oconf, seed=4242 + it))
        for opt in opts + (eopts if mode == 'both' else []):
            opt.zero_grad()
        for loss in tuple(losses) + tuple(elosses):
            loss.backward()
        model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        if mode == 'both':
            p2e.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        grads = [o.flat_grad.clone() for o in opts]
        for opt in opts + (eopts if mode == 'both' else []):
            opt.step()
        torch.cuda.synchronize()
        out.append(([float(x.detach()) for x in losses], grads, [o.flat_param.clone() for o in opts], model.metric_buffer.clone()))
    if mode == 'both':
        assert all(float(o.flat_grad.abs().sum()) > 0 for o in eopts)
    return out


@pytest.mark.parametrize('overlap', [True, False])
def test_the_dreamers_step_keeps_its_bits(hip, overlap):
    """Two iterations (the second one catches a workspace the exploration step left dirty, or one it took from a pre-launched
    backward pass): losses, flat gradients, parameters and the metric buffer of the Dreamer are bit-identical with and without the
    exploration step between training_step() and the backward() calls, and with a Plan2Explore that is built but never called."""
    alone = _iterations(overlap, 'alone')
    for mode in ('both', 'built'):
        other = _iterations(overlap, mode)
        for it, ((la, ga, pa, ma), (lb, gb, pb, mb)) in enumerate(zip(alone, other)):
            assert la == lb, (mode, it, la, lb)
            for a, b in zip(ga + pa + [ma], gb + pb + [mb]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{mode}, iteration {it}: the Dreamer\'s step changed'
    assert all(float(g.abs().sum()) > 0 for g in alone[1][1][:1])


# ------------------------------------------------------------------------------------------------ acting
def test_acting_with_the_exploration_actor(hip):
    """act(ac=p2e.ac) with supplied noise is dm_policy_draw on p2e.ac's actor and critic over the world model's features; act()
    without the keyword is the same call on the task actor-critic - its bits are unchanged - and NetworkPolicy(ac=...) passes it on."""
    from pydreamer_amd.policy import NetworkPolicy
    oconf, conf, model, opts, p2e = _setup()
    obs, noise = _batch(oconf)
    B, A = oconf.batch_size, oconf.action_dim
    obs1 = {k: v[:1].contiguous() for k, v in obs.items()}
    nz = dict(u_post=noise['u_post'][:1].contiguous(), u_act=torch.rand(B, generator=_gen(3)).to(DEV))
    state = model.init_state(B)

    def manual(ac):
        with torch.no_grad():
            features, _ = model.wm.forward(obs1, state, nz['u_post'])
            feat = features.reshape(B, -1)
            ws = model.wm.workspace(model.wm.shape(1, B, 1), feat.device)
            logits, _ = ac.actor.fwd(feat, feat.shape[1], B, ws, save_acts=False)
            value, _ = ac.critic.fwd(feat, feat.shape[1], B, ws, save_acts=False)
            action, stats = torch.empty(1, B, A, device=DEV), torch.empty(4, device=DEV)
            dws = torch.empty(int(hip.lib().dm_policy_draw_ws_floats(B)), device=DEV)
            hip.call('dm_policy_draw', 0, B, A, hip.fptr(logits), A, hip.fptr(nz['u_act']), hip.fptr(value), hip.fptr(action), A, None, None,
                     None, hip.fptr(stats), hip.fptr(dws), dws.numel() * 4, hip.stream())
            torch.cuda.synchronize()
        return action, stats, logits

    a_task, _, m_task = model.act(obs1, state, noise=nz)
    a_task2, _, _ = model.act(obs1, state, noise=nz, ac=model.ac)
    a_expl, _, m_expl = model.act(obs1, state, noise=nz, ac=p2e.ac)
    want_task, s_task, l_task = manual(model.ac)
    want_expl, s_expl, l_expl = manual(p2e.ac)
    assert not torch.equal(l_task, l_expl)
    assert torch.equal(a_task, want_task) and torch.equal(a_task2, want_task) and torch.equal(a_expl, want_expl)
    for k, i in (('policy_value', 0), ('action_prob', 1), ('policy_entropy', 2)):
        assert float(m_task[k]) == float(s_task[i]) and float(m_expl[k]) == float(s_expl[i]), k
    assert float(m_task['policy_entropy']) != float(m_expl['policy_entropy'])
    prep = lambda o: {k: v.cpu().numpy() for k, v in obs1.items()}
    for ac in (None, p2e.ac):
        torch.manual_seed(5)
        act_np, _ = NetworkPolicy(model, prep, batch_size=B, device=DEV, ac=ac)(None)
        torch.manual_seed(5)
        kw = {} if ac is None else dict(ac=ac)
        direct, _, _ = model.act(obs1, model.init_state(B), **kw)
        assert np.array_equal(act_np, direct.view(B, A).cpu().numpy())


# ------------------------------------------------------------------------------------------------ the loop
class RawLoopEnv:
    """A raw environment on a script (as tests/test_gpu_agent_metrics.py's): a (vec_dim,) vector observation, the reward a function
    of the action; episode e ends by itself after lengths[e % len] steps unless the wrapper's time limit comes first."""

    def __init__(self, idx, lengths, vec_dim):
        self.idx, self.lengths, self.vec_dim, self.episode, self.t = idx, lengths, vec_dim, -1, 0

    def _obs(self):
        return np.random.RandomState(1000 * self.idx + 37 * self.episode + self.t).randn(self.vec_dim).astype(np.float32)

    def reset(self):
        self.episode, self.t = self.episode + 1, 0
        return self._obs()

    def step(self, action):
        self.t += 1
        reward = np.float32(0.5 * int(np.argmax(action)) - 0.25 * self.t)
        return self._obs(), reward, self.t >= self.lengths[self.episode % len(self.lengths)], {}


def _loop_conf(**over):
    g = np.load(os.path.join(GOLD, 'tiny_vectorenv_inference.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    conf = config.load_config('defaults', 'vectorenv', **{**vars(oconf), **extra})
    assert (conf.batch_length, conf.batch_size) == (5, 3) and not conf.image_key
    return Namespace(**{**vars(conf), **dict(device='cuda:0', n_steps=6, log_interval=3, save_interval=3, eval_interval=0,
                                             generator_prefill_steps=40, env_time_limit=12, expl_behavior='plan2explore',
                                             disag_models=3), **over})


def test_the_trainer_loop_explores_then_switches(hip, tmp_path, monkeypatch):
    """run() online on the tiny vectorenv model, six gradient steps, 12 environment steps per gradient step, expl_until inside the
    run.  train/expl_* are logged beside the unchanged train/ keys; the ensemble's parameters move; every collected action (and per-environment value) is the one
    a replay of act() under the same generator state gives with the actor that should have acted - the exploration one while the
    collector's steps are below expl_until, the task one from then on, never the other way round; the checkpoint round-trips
    explore_state_dict and the three optimizer dicts, and a checkpoint written without them still loads."""
    from pydreamer_amd import collect as C, replay as R, train as TR
    from pydreamer_amd.envs import wrap_envs
    from pydreamer_amd.explore import EXPLORE_METRIC_SLOTS, Plan2Explore, log_name
    from pydreamer_amd.models import Dreamer
    conf = _loop_conf(expl_until=75)
    raws = [RawLoopEnv(b, lengths, conf.vecobs_size) for b, lengths in enumerate([[11, 13], [14, 10], [13, 11, 10]])]
    data_dir, logdir = str(tmp_path / 'episodes'), str(tmp_path / 'log')
    os.makedirs(data_dir)
    repo = R.LocalEpisodeRepository(data_dir)
    seen = {}
    collectors, calls = [], []
    real_run, real_act = C.Collector.run, Dreamer.act

    def run_spy(self, num_steps):
        if self not in collectors:
            collectors.append(self)
        return real_run(self, num_steps)

    def act_spy(self, obs, in_state, **kw):
        rng = torch.cuda.get_rng_state()
        out = real_act(self, obs, in_state, **kw)
        p2e = seen.get('p2e')
        if p2e is not None:      # (before the first gradient step nothing can be replayed: the prefill is random anyway)
            steps = collectors[0].steps
            expected = p2e.ac if steps < conf.expl_until else self.ac
            other = self.ac if expected is p2e.ac else p2e.ac
            after = torch.cuda.get_rng_state()
            torch.cuda.set_rng_state(rng)
            sig = lambda o: torch.cat((o[0].reshape(-1), o[2]['value'].reshape(-1)))      # the action and the critic's values
            same = torch.equal(sig(real_act(self, obs, in_state, **{**kw, 'ac': expected})), sig(out))
            torch.cuda.set_rng_state(rng)
            differs = not torch.equal(sig(real_act(self, obs, in_state, **{**kw, 'ac': other})), sig(out))
            torch.cuda.set_rng_state(after)
            calls.append((steps, kw.get('ac') is not None, same, differs))
        return out

    def on_step(step, model, obs, tensors, p2e):
        seen['p2e'] = p2e
        seen.setdefault('first', {k: v.detach().clone() for k, v in p2e.state_dict().items()})
        seen['model'] = model

    monkeypatch.setattr(C.Collector, 'run', run_spy)
    monkeypatch.setattr(Dreamer, 'act', act_spy)
    logged = []
    steps = TR.run(conf, repo, envs=wrap_envs(raws, conf), logdir=logdir, env_steps_per_grad_step=12, seed=1, steps_per_npz=10,
                   logger=lambda m, s: logged.append((s, dict(m))), on_step=on_step, agent_log_every=0)
    assert steps == 6
    train = [(s, m) for s, m in logged if 'train/steps' in m]
    assert [s for s, _ in train] == [3, 6]
    for _, m in train:
        for k in EXPLORE_METRIC_SLOTS:
            assert f'train/{log_name(k)}' in m and math.isfinite(m[f'train/{log_name(k)}']), k
        assert 'train/loss_model' in m and 'train/grad_norm' in m and m['train/expl_loss_disag'] > 0 and m['train/expl_reward'] > 0
        assert all(k.startswith('train/expl_') for k in m if 'expl' in k or 'disag' in k)
    p2e, model = seen['p2e'], seen['model']
    moved = [k for k, v in p2e.state_dict().items() if k.startswith('ensemble.') and not torch.equal(v, seen['first'][k])]
    assert len(moved) == 3 * 18, 'the ensemble was not trained'
    # who acted
    assert len(calls) >= 16 and all(same for _, _, same, _ in calls), [c for c in calls if not c[2]]
    flags = [explore for _, explore, _, _ in calls]
    n_expl = sum(flags)
    assert 0 < n_expl < len(flags) and flags == [True] * n_expl + [False] * (len(flags) - n_expl)
    assert all((s < conf.expl_until) == e for s, e, _, _ in calls)
    assert any(d for _, e, _, d in calls if e) and any(d for _, e, _, d in calls if not e), 'the two actors never disagreed'
    # the checkpoint
    path = os.path.join(logdir, 'checkpoints', 'latest.pt')
    ck = torch.load(path, map_location='cpu')
    assert ck['epoch'] == 6 and {'explore_state_dict', 'explore_optimizer_0_state_dict', 'explore_optimizer_1_state_dict',
                                 'explore_optimizer_2_state_dict', 'model_state_dict', 'optimizer_3_state_dict'} <= set(ck)
    assert not [k for k in ck['model_state_dict'] if 'ensemble' in k or 'expl' in k]
    model2 = Dreamer(conf).to(DEV)
    opts2 = model2.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    p2 = Plan2Explore(conf, model2).to(DEV)
    eopts2 = p2.init_optimizers()
    fresh = {k: v.detach().clone() for k, v in p2.state_dict().items()}
    assert TR.load_checkpoint(path, model2, opts2, map_location=DEV, explore=p2, explore_optimizers=eopts2) == 6
    sd, sd2 = p2e.state_dict(), p2.state_dict()
    assert list(sd) == list(sd2) == list(ck['explore_state_dict']) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert all(torch.equal(a.exp_avg, b.exp_avg) and a.step_count == b.step_count == 6 for a, b in zip(p2e._opt.values(), eopts2))
    assert all(torch.equal(model.state_dict()[k], v) for k, v in model2.state_dict().items())
    # a file from before: no explore keys, loads, leaves the explorer alone
    old = str(tmp_path / 'old.pt')
    TR.save_checkpoint(old, model, list(model._opt.values()), 4)
    assert 'explore_state_dict' not in torch.load(old, map_location='cpu')
    p3 = Plan2Explore(conf, model2).to(DEV)
    before = {k: v.detach().clone() for k, v in p3.state_dict().items()}
    assert TR.load_checkpoint(old, model2, opts2, map_location=DEV, explore=p3, explore_optimizers=p3.init_optimizers()) == 4
    assert all(torch.equal(before[k], v) for k, v in p3.state_dict().items()) and len(fresh) == len(before)
