"""-m gpu: the acting path - dm_policy_draw, Dreamer.act and NetworkPolicy.

  1 dm_policy_draw against the kernels the learner's imagination draws with, bit for bit: the one-hot index / row against
    dm_sample_onehot(rows, 1, A, ...), the continuous action against dm_sample_continuous; rows {1, 3, 65, 257}, one-hot
    A {1, 2, 6, 18, 33, 65, 130} with ldp = A + 3, continuous A {1, 6, 17} for both kinds; rows with u = 0, u = 1 - 2^-24, all-equal
    logits and one logit 40 above the rest keep log_prob and entropy finite.
  2 dm_policy_draw against the formulas in float64 on the CPU: log_prob and entropy per row at the tensor bar (|err| <= 1e-4 |ref| +
    1e-4 max(1, max |ref|)); the index for uniforms placed at the float64 midpoint of a class's CDF interval (interval > 1e-4 wide,
    margin > 5e-5 asserted, every row compared); stats against the float64 means of the kernel's own per-row outputs within the fp32
    summation bound rows 2^-23 max|x|; a second call gives the same stats, bit for bit.
  3 Dreamer.act on the reference-written inference fixtures (tiny_inference, tiny_minigrid_inference, tiny_vectorenv_inference,
    tiny_obs_inference) and on one continuous configuration per kind: out_state equal to inference()'s and at the existing
    inference tests' bars to the fixture, the action the one dm_sample_onehot / dm_sample_continuous give for inference()'s actor
    output, policy_value within the summation bound of inference()'s, action_prob and policy_entropy against float64 at the metric
    bar (1e-4 relative or 5e-6).
  4 carried state over two calls, a reset row, return_rows, and the draw without explicit noise (shape only).
  5 NetworkPolicy (B = 1 and 3, three steps) against direct act() calls under the same device-generator seed."""
import ast
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_form_params as CFP                     # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
ROWS = [1, 3, 65, 257]
ONEHOT_A = [1, 2, 6, 18, 33, 65, 130]
CONT_A = [1, 6, 17]
U_MAX = 1.0 - 2.0 ** -24
EPS32 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ helpers
def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-12)


def _close(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})'


def _close_rt(a, b, what, rtol=1e-4, atol=1e-4):
    """The tensor bar: |a - b| <= rtol |b| + atol max(1, max |b|); prints the worst err/tol ratio."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    err = (a - b).abs()
    bound = atol * max(1.0, float(b.abs().max())) + rtol * b.abs()
    print(f'[tol] {what}: max err {float(err.max()):.3e}, worst err/tol {float((err / bound).max()):.3f}')
    assert not (err > bound).any() and not torch.isnan(err).any(), \
        f'{what}: {int((err > bound).sum())}/{err.numel()} mismatches, max err {float(err.max()):.3e}'


def _check_metric(got, ref, what):
    print(f'[metric] {what}: got {float(got):.8g}, ref {float(ref):.8g}')
    assert _rel(got, ref) < 1e-4 or abs(float(got) - ref) < 5e-6, (what, float(got), ref)


def _within_sum_bound(got, x64, what):
    """|got - mean(x)| <= rows 2^-23 max|x|: the fp32 bound of a sum of `rows` terms in any order, divided by rows."""
    ref, bound = float(x64.mean()), x64.numel() * EPS32 * float(x64.abs().max())
    print(f'[sum] {what}: got {float(got):.9g}, float64 mean {ref:.9g}, |err| {abs(float(got) - ref):.3e}, bound {bound:.3e}')
    assert abs(float(got) - ref) <= bound, (what, float(got), ref, bound)


def _draw(hip, kind, A, params, noise, value=None, lda=None):
    """dm_policy_draw on `params` (rows, ldp) as they lie; the action rows sit in a (rows, lda) buffer filled with a sentinel."""
    rows, ldp = params.shape
    lda = lda or A
    lib = hip.lib()
    out = dict(action=torch.full((rows, lda), -7.0, device=DEV), act_idx=torch.full((rows,), -1, dtype=torch.int32, device=DEV),
               log_prob=torch.full((rows,), float('nan'), device=DEV), entropy=torch.full((rows,), float('nan'), device=DEV),
               stats=torch.full((4,), float('nan'), device=DEV))
    ws = torch.empty(int(lib.dm_policy_draw_ws_floats(rows)), device=DEV)
    hip.call('dm_policy_draw', kind, rows, A, hip.fptr(params), ldp, hip.fptr(noise), hip.fptr(value), hip.fptr(out['action']), lda,
             hip.ptr(out['act_idx']), hip.fptr(out['log_prob']), hip.fptr(out['entropy']), hip.fptr(out['stats']), hip.fptr(ws),
             ws.numel() * 4, hip.stream())
    assert torch.equal(out['action'][:, A:], torch.full((rows, lda - A), -7.0, device=DEV)), 'columns beyond A were written'
    return out


def _sample_onehot(hip, logits, A, u):
    rows, ldl = logits.shape
    onehot = torch.full((rows, A), -7.0, device=DEV)
    idx = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    hip.call('dm_sample_onehot', rows, 1, A, hip.fptr(logits), ldl, hip.fptr(u), None, hip.fptr(onehot), A, hip.ptr(idx), hip.stream())
    return onehot, idx


def _sample_continuous(hip, kind, params, eps):
    rows, A = eps.shape
    act = torch.empty(rows, A, device=DEV)
    hip.call('dm_sample_continuous', kind, rows, A, hip.fptr(params), hip.fptr(eps), hip.fptr(act), hip.stream())
    return act


def _onehot_case(rows, A, seed, special):
    """Logits (rows, A + 3) - the three columns beyond A hold 100, which would win any draw that read them - and uniforms.
    special: rows cycle through u = 0, u = 1 - 2^-24, all-equal logits, one logit 40 above the rest, both, and a plain row."""
    gen = torch.Generator().manual_seed(seed)
    logits = torch.full((rows, A + 3), 100.0)
    logits[:, :A] = 2.0 * torch.randn(rows, A, generator=gen)
    u = torch.rand(rows, generator=gen)
    if special:
        for r in range(rows):
            case = (r + seed) % 6
            if case in (0,):
                u[r] = 0.0
            if case in (1, 4):
                u[r] = U_MAX
            if case in (2, 4):
                logits[r, :A] = 0.37
            if case == 3:
                logits[r, (r * 7) % A] += 40.0
    return logits.to(DEV), u.to(DEV)


def _cont_case(rows, A, seed, extreme):
    gen = torch.Generator().manual_seed(seed)
    params = 1.5 * torch.randn(rows, 2 * A, generator=gen)
    eps = torch.randn(rows, A, generator=gen)
    if extreme:       # draws deep in tanh's saturation, very wide and very narrow scales
        eps[::3, 0] = 8.0
        eps[1::3, -1] = -8.0
        params[::2, A] = 30.0
        params[1::2, 2 * A - 1] = -30.0
    return params.to(DEV), eps.to(DEV)


def _cont_ref64(kind, params, eps):
    """functions.py:59-78 in float64: (pre-tanh draw x, action, log_prob, entropy) per row."""
    p, e = params.double().cpu(), eps.double().cpu()
    A = e.shape[1]
    m, s = p[:, :A], p[:, A:2 * A]
    if kind == 1:
        mean, std = 5.0 * torch.tanh(m / 5.0), F.softplus(s) + 0.1
    else:
        mean, std = torch.tanh(m), torch.sigmoid(s) + 0.01
    x = mean + std * e
    logn = -0.5 * ((x - mean) / std) ** 2 - torch.log(std) - 0.5 * np.log(2.0 * np.pi)
    if kind == 1:
        logn = logn - 2.0 * (np.log(2.0) - x - F.softplus(-2.0 * x))
    ent = (0.5 + 0.5 * np.log(2.0 * np.pi) + torch.log(std)).sum(-1)
    return x, (torch.tanh(x) if kind == 1 else x), logn.sum(-1), ent


# ------------------------------------------------------------------------------------------------ 1: against the existing kernels
@pytest.mark.parametrize('rows', ROWS)
def test_onehot_draw_equals_dm_sample_onehot(hip, rows):
    for ai, A in enumerate(ONEHOT_A):
        logits, u = _onehot_case(rows, A, seed=10 * rows + ai, special=True)
        onehot, idx = _sample_onehot(hip, logits, A, u)
        got = _draw(hip, 0, A, logits, u, lda=A + 2)
        assert torch.equal(got['act_idx'], idx), (rows, A)
        assert torch.equal(got['action'][:, :A], onehot), (rows, A)
        assert int(idx.min()) >= 0 and int(idx.max()) < A
        assert torch.equal(got['action'][:, :A], F.one_hot(idx.long(), A).float())
        assert bool(torch.isfinite(got['log_prob']).all()) and bool(torch.isfinite(got['entropy']).all()), (rows, A)
        assert float(got['log_prob'].max()) <= 0.0 and float(got['entropy'].min()) >= 0.0
        assert bool(torch.isfinite(got['stats']).all()) and float(got['stats'][0]) == 0.0 and float(got['stats'][3]) == 0.0


@pytest.mark.parametrize('kind', [1, 2])
@pytest.mark.parametrize('rows', ROWS)
def test_continuous_draw_equals_dm_sample_continuous(hip, rows, kind):
    for ai, A in enumerate(CONT_A):
        params, eps = _cont_case(rows, A, seed=100 * kind + 10 * rows + ai, extreme=True)
        want = _sample_continuous(hip, kind, params, eps)
        got = _draw(hip, kind, A, params, eps, lda=A + 1)
        assert torch.equal(got['action'][:, :A], want), (rows, A, kind)
        padded = torch.full((rows, 2 * A + 5), float('nan'), device=DEV)      # a leading dimension above the row width
        padded[:, :2 * A] = params
        again = _draw(hip, kind, A, padded, eps)
        for k in ('action', 'log_prob', 'entropy', 'stats', 'act_idx'):
            assert torch.equal(again[k], got[k][:, :A] if k == 'action' else got[k]), (k, rows, A, kind)
        assert int(got['act_idx'].abs().max()) == 0
        assert bool(torch.isfinite(got['log_prob']).all()) and bool(torch.isfinite(got['entropy']).all()), (rows, A, kind)
        if kind == 1:
            assert float(got['action'][:, :A].abs().max()) <= 1.0


# ------------------------------------------------------------------------------------------------ 2: against float64
@pytest.mark.parametrize('rows', ROWS)
def test_onehot_draw_against_float64(hip, rows):
    for ai, A in enumerate(ONEHOT_A):
        logits, _ = _onehot_case(rows, A, seed=1000 + 10 * rows + ai, special=False)
        x = logits[:, :A].double().cpu()
        logp = x - torch.logsumexp(x, -1, keepdim=True)
        p = logp.exp()
        cdf = torch.cumsum(p, -1)
        cdf = cdf / cdf[:, -1:]
        lo = torch.cat((torch.zeros(rows, 1, dtype=torch.float64), cdf[:, :-1]), -1)
        want = torch.empty(rows, dtype=torch.int64)
        u64 = torch.empty(rows, dtype=torch.float64)
        for r in range(rows):      # the (r-th, cyclically) class whose CDF interval is wider than 1e-4; its float64 midpoint
            wide = torch.nonzero(cdf[r] - lo[r] > 1e-4).flatten()
            want[r] = wide[(r + ai) % len(wide)]
            u64[r] = 0.5 * (lo[r, want[r]] + cdf[r, want[r]])
        u = u64.float()
        rr = torch.arange(rows)
        margin = torch.minimum(u.double() - lo[rr, want], cdf[rr, want] - u.double())
        assert float(margin.min()) > 5e-5, float(margin.min())
        value = torch.randn(rows, generator=torch.Generator().manual_seed(rows + ai)).to(DEV) * 3.0 + 1.0
        got = _draw(hip, 0, A, logits, u.to(DEV), value=value)
        assert torch.equal(got['act_idx'].cpu().long(), want), (rows, A)
        _close_rt(got['log_prob'], logp[rr, want], f'onehot log_prob rows {rows} A {A}')
        _close_rt(got['entropy'], -(p * logp).sum(-1), f'onehot entropy rows {rows} A {A}')
        _check_stats(hip, got, value, lambda: _draw(hip, 0, A, logits, u.to(DEV), value=value), f'onehot rows {rows} A {A}')


def _check_stats(hip, got, value, again, what):
    lp64 = got['log_prob'].double().cpu()
    assert float(lp64.min()) > -80.0, 'test inputs: exp(log_prob) must be a normal fp32 number'
    _within_sum_bound(got['stats'][0], value.double().cpu(), what + ' mean value')
    _within_sum_bound(got['stats'][1], lp64.exp(), what + ' mean exp(log_prob)')
    _within_sum_bound(got['stats'][2], got['entropy'].double().cpu(), what + ' mean entropy')
    assert float(got['stats'][3]) == 0.0
    second = again()
    assert torch.equal(second['stats'].view(torch.int32), got['stats'].view(torch.int32)), what + ': stats differ between two calls'


@pytest.mark.parametrize('kind', [1, 2])
@pytest.mark.parametrize('rows', ROWS)
def test_continuous_draw_against_float64(hip, rows, kind):
    for ai, A in enumerate(CONT_A):
        params, eps = _cont_case(rows, A, seed=2000 + 100 * kind + 10 * rows + ai, extreme=False)
        x, action, logp, ent = _cont_ref64(kind, params, eps)
        value = torch.randn(rows, generator=torch.Generator().manual_seed(7 * rows + ai)).to(DEV)
        got = _draw(hip, kind, A, params, eps, value=value)
        _close_rt(got['action'], action, f'kind {kind} action rows {rows} A {A}')
        _close_rt(got['log_prob'], logp, f'kind {kind} log_prob (at the pre-tanh draw) rows {rows} A {A}')
        _close_rt(got['entropy'], ent, f'kind {kind} entropy rows {rows} A {A}')
        _check_stats(hip, got, value, lambda: _draw(hip, kind, A, params, eps, value=value), f'kind {kind} rows {rows} A {A}')


def test_tanh_normal_log_prob_keeps_the_draw_in_saturation(hip):
    """x = mean + std eps far in tanh's tail: the action rounds to +-1 (atanh of it is infinite or clamped), the log-probability
    computed from x stays the float64 value."""
    A = 2
    params = torch.tensor([[3.0, -3.0, 0.5, 0.5], [-4.0, 4.0, 1.0, -1.0]], device=DEV)
    eps = torch.tensor([[8.0, -8.0], [-6.0, 16.0]], device=DEV)
    x, action, logp, ent = _cont_ref64(1, params, eps)
    got = _draw(hip, 1, A, params, eps)
    assert float(x.abs().min()) > 9.0 and torch.equal(got['action'].abs().cpu(), torch.ones(2, A))
    _close_rt(got['log_prob'], logp, 'saturated tanh_normal log_prob')
    _close_rt(got['entropy'], ent, 'saturated tanh_normal entropy')


# ------------------------------------------------------------------------------------------------ 3: end to end
def _build(conf, params=None, shapes=None):
    from pydreamer_amd.models import Dreamer
    model = Dreamer(conf)
    if params is None:
        assert list(model.state_dict().keys()) == list(shapes.keys())
        params = CFP.make_params(shapes, seed=0)
    model.load_state_dict(params, strict=True)
    return model.to(DEV)


def _fixture(name):
    """(g, model, obs) of an inference fixture, through the loader of the inference test that reads it."""
    from pydreamer_amd import config
    g = np.load(os.path.join(GOLD, name + '.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    t = lambda k: torch.from_numpy(g['in_' + k]).to(DEV)
    if name == 'tiny_inference':
        model = _build(config.load_config('defaults', 'atari', **vars(oconf)), params=O.make_params(oconf, seed=0))
        keys = ('action', 'reset')
    else:
        section = {'tiny_minigrid_inference': 'minigrid', 'tiny_vectorenv_inference': 'vectorenv', 'tiny_obs_inference': 'atari'}[name]
        extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
        model = _build(config.load_config('defaults', section, **{**vars(oconf), **extra}), shapes=CFP.shapes_of_fixture(g))
        keys = ('action', 'reset', 'reward', 'terminal') + (('vecobs',) if 'in_vecobs' in g.files else ())
    obs = {k: t(k) for k in keys}
    if 'in_image_u8' in g.files:
        obs['image'] = (torch.from_numpy(g['in_image_u8']).float() / 255.0 - 0.5).permute(0, 1, 4, 2, 3).contiguous().to(DEV)
    elif 'in_image_classes' in g.files:
        classes = torch.from_numpy(g['in_image_classes'].astype(np.int64))
        obs['image'] = F.one_hot(classes, oconf.image_channels).permute(0, 1, 4, 2, 3).float().contiguous().to(DEV)
    return g, model, obs


def _actor_rows(model, obs, state, u_post):
    """The actor's and critic's output rows exactly as inference() computes them (models.py Dreamer.inference)."""
    with torch.no_grad():
        features, _ = model.wm.forward(obs, state, u_post)
        B = obs['action'].shape[1]
        feat = features.reshape(B, -1)
        ws = model.wm.workspace(model.wm.shape(1, B, 1), feat.device)
        logits, _ = model.ac.actor.fwd(feat, feat.shape[1], B, ws, save_acts=False)
        value, _ = model.ac.critic.fwd(feat, feat.shape[1], B, ws, save_acts=False)
    return logits.clone(), value.view(B).clone()


@pytest.mark.parametrize('name', ['tiny_inference', 'tiny_minigrid_inference', 'tiny_vectorenv_inference', 'tiny_obs_inference'])
def test_act_on_the_reference_inference_fixtures(hip, name):
    g, model, obs = _fixture(name)
    B, A = obs['action'].shape[1], model.conf.action_dim
    state = (torch.from_numpy(g['in_h']).to(DEV), torch.from_numpy(g['in_z']).to(DEV))
    u_post = torch.from_numpy(g['in_u']).to(DEV)
    if 'action_probs' in g.files:
        p64 = torch.from_numpy(g['action_probs']).double().view(B, A)
    else:
        p64 = torch.softmax(torch.from_numpy(g['action_logits']).double().view(B, A), -1)
    p64 = p64 / p64.sum(-1, keepdim=True)
    # u_act: the float64 midpoint of the CDF interval of each row's (b-th, cyclically) class with probability above 1e-3
    cdf = torch.cumsum(p64, -1)
    lo = torch.cat((torch.zeros(B, 1, dtype=torch.float64), cdf[:, :-1]), -1)
    want = torch.stack([torch.nonzero(p64[b] > 1e-3).flatten()[b % int((p64[b] > 1e-3).sum())] for b in range(B)])
    bb = torch.arange(B)
    u_act = (0.5 * (lo[bb, want] + cdf[bb, want])).float().to(DEV)
    with torch.no_grad():
        dist, (h0, z0), m0 = model.inference(obs, state, noise=dict(u_post=u_post))
    raw_logits, value = _actor_rows(model, obs, state, u_post)
    action, (h1, z1), m1 = model.act(obs, state, noise=dict(u_post=u_post, u_act=u_act), return_rows=True)
    torch.cuda.synchronize()
    assert torch.equal(h1, h0) and torch.equal(z1, z0), 'act and inference disagree on the next state'
    if name == 'tiny_minigrid_inference':
        _close_rt(h1, torch.from_numpy(g['out_h']), 'out_state h')
    else:
        _close(h1, torch.from_numpy(g['out_h']), 0, 2e-6, 'out_state h')
    assert torch.equal(z1.cpu(), torch.from_numpy(g['out_z']))
    assert action.shape == (1, B, A) and action.dtype == torch.float32 and action.is_cuda
    _within_sum_bound(m1['policy_value'], value.double().cpu(), 'policy_value against the critic rows')
    assert abs(float(m1['policy_value']) - float(m0['policy_value'])) <= B * EPS32 * float(value.abs().max())
    # the action: dm_sample_onehot on inference()'s logits - the distribution's (normalised) ones and the actor's raw rows
    for lg in (dist.logits.reshape(B, A).contiguous(), raw_logits):
        onehot, idx = _sample_onehot(hip, lg, A, u_act)
        assert torch.equal(action.view(B, A), onehot) and torch.equal(m1['act_idx'], idx)
    assert torch.equal(m1['act_idx'].cpu().long(), want), 'the draw left the class whose CDF interval holds u'
    _check_metric(m1['action_prob'], float(p64[bb, want].mean()), 'action_prob')
    _check_metric(m1['policy_entropy'], float(-(p64 * p64.clamp_min(1e-300).log()).sum(-1).mean()), 'policy_entropy')
    _close_rt(m1['log_prob'], p64[bb, want].log(), 'per-row log_prob')
    assert m1['policy_value']._base is m1['policy_entropy']._base and m1['policy_value']._base.numel() == 4


@pytest.mark.parametrize('fixture,kind', [('tiny_dmc', 1), ('tiny_normal_tanh', 2)])
def test_act_continuous_actor(hip, fixture, kind):
    """The configuration of a continuous-actor fixture, weights by O.make_params, the first frame of the synthetic batch."""
    from pydreamer_amd import config
    g = np.load(os.path.join(GOLD, fixture + '.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    model = _build(config.load_config('defaults', 'atari', **vars(oconf)), params=O.make_params(oconf, seed=0))
    assert model.ac.dist_kind == kind
    B, A = oconf.batch_size, oconf.action_dim
    obs = {k: v[:1].contiguous().to(DEV) for k, v in O.preprocess(O.synthetic_batch(oconf), oconf).items()}
    gen = torch.Generator().manual_seed(5)
    state = tuple(0.5 * torch.randn(s.shape, generator=gen).to(DEV) for s in model.init_state(B))
    lat = torch.rand if oconf.stoch_discrete else torch.randn
    u_post = lat(1, B, oconf.stoch_dim, generator=gen).to(DEV)
    eps = torch.randn(B, A, generator=gen).to(DEV)
    with torch.no_grad():
        dist, (h0, z0), m0 = model.inference(obs, state, noise=dict(u_post=u_post))
    params, value = _actor_rows(model, obs, state, u_post)
    action, (h1, z1), m1 = model.act(obs, state, noise=dict(u_post=u_post, u_act=eps), return_rows=True)
    torch.cuda.synchronize()
    assert torch.equal(h1, h0) and torch.equal(z1, z0)
    assert torch.equal(action.view(B, A), _sample_continuous(hip, kind, params, eps))
    assert 'act_idx' not in m1 and m1['log_prob'].shape == (B,) and m1['entropy'].shape == (B,)
    assert abs(float(m1['policy_value']) - float(m0['policy_value'])) <= B * EPS32 * float(value.abs().max())
    x, act64, logp, ent = _cont_ref64(kind, params, eps)
    _close_rt(action.view(B, A), act64, 'action')
    _close_rt(m1['log_prob'], logp, 'per-row log_prob')
    _check_metric(m1['action_prob'], float(logp.exp().mean()), 'action_prob')
    _check_metric(m1['policy_entropy'], float(ent.mean()), 'policy_entropy')
    _check_metric(m1['policy_entropy'], float(dist.entropy().double().mean()), 'policy_entropy against the distribution object')
    with pytest.raises(ValueError, match='actor noise'):
        model.act(obs, state, noise=dict(u_act=eps[:, 0].contiguous()))


# ------------------------------------------------------------------------------------------------ 4: carried state, resets
@pytest.fixture(scope='module')
def tiny_model():
    from pydreamer_amd import config
    oconf = O.tiny_conf()
    model = _build(config.load_config('defaults', 'atari', **vars(oconf)), params=O.make_params(oconf, seed=0))
    return oconf, model


def _tiny_obs(oconf, B, seed, prev_action=None):
    rs = np.random.RandomState(seed)
    image = torch.from_numpy(rs.randint(0, 256, (1, B, 64, 64, oconf.image_channels)).astype(np.uint8))
    if prev_action is None:
        prev_action = F.one_hot(torch.from_numpy(rs.randint(0, oconf.action_dim, (1, B))), oconf.action_dim).float()
    return dict(image=image.to(DEV), action=prev_action.to(DEV), reset=torch.zeros(1, B, dtype=torch.bool, device=DEV))


def test_two_act_calls_carry_the_state_as_two_inference_calls(hip, tiny_model):
    oconf, model = tiny_model
    B, A, S = 4, oconf.action_dim, oconf.stoch_dim
    gen = torch.Generator().manual_seed(11)
    u_post = [torch.rand(1, B, S, generator=gen).to(DEV) for _ in range(2)]
    u_act = [torch.rand(B, generator=gen).to(DEV) for _ in range(2)]
    obs0 = _tiny_obs(oconf, B, 1)
    a0, s_act, m = model.act(obs0, model.init_state(B), noise=dict(u_post=u_post[0], u_act=u_act[0]), return_rows=True)
    assert m['log_prob'].shape == (B,) and m['entropy'].shape == (B,) and m['value'].shape == (B,) and m['act_idx'].shape == (B,)
    assert m['log_prob'].dtype == m['entropy'].dtype == m['value'].dtype == torch.float32 and m['act_idx'].dtype == torch.int32
    assert all(m[k].dim() == 0 and m[k].is_cuda for k in ('policy_value', 'action_prob', 'policy_entropy'))
    assert set(model.act(obs0, model.init_state(B))[2]) == {'policy_value', 'action_prob', 'policy_entropy'}
    obs1 = _tiny_obs(oconf, B, 2, prev_action=a0)
    a1, s_act2, _ = model.act(obs1, s_act, noise=dict(u_post=u_post[1], u_act=u_act[1]))
    with torch.no_grad():
        _, s_inf, _ = model.inference(obs0, model.init_state(B), noise=dict(u_post=u_post[0]))
        _, s_inf2, _ = model.inference(obs1, s_inf, noise=dict(u_post=u_post[1]))
    logits1, _ = _actor_rows(model, obs1, s_inf, u_post[1])
    for a, b in zip(list(s_act) + list(s_act2), list(s_inf) + list(s_inf2)):
        assert torch.equal(a, b)
    assert float(s_act2[0].abs().max()) > 0 and not torch.equal(s_act2[0], s_act[0])
    assert torch.equal(a1.view(B, A), _sample_onehot(hip, logits1, A, u_act[1])[0])


def test_a_reset_row_ignores_its_carried_state(hip, tiny_model):
    oconf, model = tiny_model
    B, S, b = 3, oconf.stoch_dim, 1
    gen = torch.Generator().manual_seed(12)
    noise = dict(u_post=torch.rand(1, B, S, generator=gen).to(DEV), u_act=torch.rand(B, generator=gen).to(DEV))
    state = tuple(torch.randn(s.shape, generator=gen).to(DEV) for s in model.init_state(B))
    assert float(state[0][b].abs().min()) > 0
    zeroed = tuple(s.clone() for s in state)
    for s in zeroed:
        s[b] = 0.0
    obs = _tiny_obs(oconf, B, 3)
    obs['reset'][0, b] = True
    outs = [model.act(obs, st, noise=noise, return_rows=True) for st in (state, zeroed)]
    (a_x, s_x, m_x), (a_y, s_y, m_y) = outs
    assert torch.equal(a_x, a_y) and all(torch.equal(p, q) for p, q in zip(s_x, s_y))
    for k in ('log_prob', 'entropy', 'value', 'act_idx', 'policy_value', 'action_prob', 'policy_entropy'):
        assert torch.equal(m_x[k], m_y[k]), k
    obs['reset'][0, b] = False      # without the reset the carried state matters: the comparison above is not vacuous
    _, s_z, _ = model.act(obs, state, noise=noise)
    assert not torch.equal(s_z[0][b], s_x[0][b]) and torch.equal(s_z[0][[0, 2]], s_x[0][[0, 2]])


def test_act_draws_its_own_noise(hip, tiny_model):
    oconf, model = tiny_model
    B, A = 5, oconf.action_dim
    obs = _tiny_obs(oconf, B, 4)
    for _ in range(2):
        action, state, metrics = model.act(obs, model.init_state(B))
        assert action.shape == (1, B, A)
        assert torch.equal(action.sum(-1), torch.ones(1, B, device=DEV)) and torch.equal(action.max(-1).values, torch.ones(1, B, device=DEV))
        assert all(bool(torch.isfinite(v)) for v in metrics.values())


# ------------------------------------------------------------------------------------------------ 5: NetworkPolicy
@pytest.mark.parametrize('B', [1, 3])
def test_network_policy_equals_direct_act_calls(hip, tiny_model, B):
    from pydreamer_amd import NetworkPolicy
    from pydreamer_amd.policy import StepPreprocessor
    oconf, model = tiny_model
    A = oconf.action_dim
    rs = np.random.RandomState(20 + B)
    steps = [dict(image=rs.randint(0, 256, (B, 64, 64, oconf.image_channels)).astype(np.uint8), action=rs.randint(0, A, B),
                  reward=rs.randn(B).astype(np.float32), terminal=np.zeros(B, np.float32), reset=(np.arange(B) == 0) & (i == 0))
             for i in range(3)]
    prep = StepPreprocessor(A, clip_rewards='tanh', batched=True)
    policy = NetworkPolicy(model, prep, batch_size=B)
    state = model.init_state(B)
    for i, env_obs in enumerate(steps):
        torch.manual_seed(100 + i)
        action, metrics = policy(env_obs)
        torch.manual_seed(100 + i)
        obs = {k: torch.from_numpy(v).to(DEV) for k, v in prep(env_obs).items()}
        a_ref, state, m_ref = model.act(obs, state)
        assert isinstance(action, np.ndarray) and action.shape == ((A,) if B == 1 else (B, A))
        assert np.array_equal(action.reshape(B, A), a_ref.view(B, A).cpu().numpy())
        assert set(metrics) == {'policy_value', 'action_prob', 'policy_entropy'}
        for k, v in metrics.items():
            assert type(v) is float and v == float(m_ref[k]), (k, v, float(m_ref[k]))
        for p, q in zip(policy.state, state):
            assert torch.equal(p, q)
    policy.reset_state(np.arange(B) == 0)
    assert float(policy.state[0][0].abs().max()) == 0.0 and (B == 1 or float(policy.state[0][1].abs().max()) > 0.0)
