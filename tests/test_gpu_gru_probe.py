"""-m gpu: WorldModelProbe(model='gru_probe') against the reference-written fixtures tests/golden/tiny_gru_probe_map_goals.npz and
tiny_gru_probe_goals.npz (scripts/gen_gru_probe_golden.py): trainer iterations with carried state and optimizer steps.

Bars: the step-case bars of tests/test_gpu_map_probe.py::test_training_steps_match_the_reference, unchanged - losses 2e-5 relative
(or 2e-6), metrics 1e-4 relative (or 5e-6) with NaN where the reference has NaN, tensors and out_state 1e-4 relative + 1e-4 max(1,
max |ref|), gradient norms (every parameter, and grad_norm) 2e-3 relative + 1e-7, the stored full gradients 2e-3 relative L2,
parameter |.| sums after the optimizer step 2e-6 relative, acc_map per frame exactly.  tests/test_baselines_cpu.py holds the
reference's own fp32-vs-fp64 deviation to a quarter of each bar.
"""
import ast
import math
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
FIXTURES = ['tiny_gru_probe_map_goals', 'tiny_gru_probe_goals']
AGE_NAMES = [f'mse_goal_age{a}' for a in (0, 5, 10, 50, 200, 1000)]
GOAL_METRICS = ['loss_goal_direction', 'loss_goals_direction', 'mse_goals', 'var_goals'] + AGE_NAMES
_GOLD = {}


def _gold(name):
    if name not in _GOLD:
        _GOLD[name] = dict(np.load(os.path.join(GOLD, name + '.npz')))
    return _GOLD[name]


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _close_rt(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bound = atol + rtol * b.abs()
    print(f'[tol] {what}: max err {float(err.max()):.3e}, worst err/tol {float((err / bound).max()):.3f}')
    assert not (err > bound).any(), f'{what}: {int((err > bound).sum())}/{err.numel()} mismatches, max err {float(err.max()):.3e}'


def _check_metric(got, ref, what):
    got, ref = float(got), float(ref)
    if math.isnan(ref) or math.isnan(got):
        assert math.isnan(ref) and math.isnan(got), (what, got, ref)
    else:
        assert _rel(got, ref) < 1e-4 or abs(got - ref) < 5e-6, (what, got, ref)


def _model(g):
    from pydreamer_amd import config
    from pydreamer_amd.models import WorldModelProbe
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    model = WorldModelProbe(config.load_config('defaults', 'atari', **{**vars(oconf), **extra}))
    shapes = CFP.shapes_of_fixture(g)
    assert list(model.state_dict().keys()) == list(shapes.keys())
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    return oconf, model.to(DEV)


def _obs(g, pre, oconf, model, u8=False):
    raw = {k: g[pre + 'in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
    obs = {k: v.to(DEV) for k, v in O.preprocess(raw, oconf).items()}
    if u8:
        obs['image'] = torch.from_numpy(raw['image_u8']).to(DEV)
    pm = model.conf.probe_model
    for k in ('action_next', 'goal_direction', 'goals_direction', 'goals_visage'):
        obs[k] = torch.from_numpy(g[pre + 'in_' + k]).to(DEV)
    if 'map' in pm:
        classes = torch.from_numpy(g[pre + 'in_map_classes'].astype(np.int64))
        obs['map'] = F.one_hot(classes, model.conf.map_channels).permute(0, 1, 4, 2, 3).float().contiguous().to(DEV)
        obs['map_coord'] = torch.from_numpy(g[pre + 'in_map_coord']).to(DEV)
        obs['map_seen_mask'] = torch.from_numpy(g[pre + 'in_map_seen_mask']).to(DEV)
    return obs


@pytest.mark.parametrize('name', FIXTURES)
def test_training_steps_match_the_reference(hip, name):
    g = _gold(name)
    oconf, model = _model(g)
    pm = model.conf.probe_model
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    assert len(opts) == 1 and [id(p) for p in opts[0]._plist] == [id(p) for p in model.parameters()]
    state = model.init_state(oconf.batch_size)
    assert tuple(state.shape) == (1, oconf.batch_size, oconf.deter_dim) and not state.any()
    expect = set(GOAL_METRICS) | ({'loss_map', 'acc_map', 'acc_map_seen'} if 'map' in pm else set())
    for s in range(2):
        pre = f's{s}_'
        obs = _obs(g, pre, oconf, model)
        assert g[pre + 'in_reset'][1:].any()
        losses, state, metrics, tensors, dream = model.training_step(obs, state)
        assert len(losses) == 1 and dream == {} and losses[0].requires_grad
        assert tuple(state.shape) == (1, oconf.batch_size, oconf.deter_dim) and not state.requires_grad
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        assert list(gm) == ['grad_norm']
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters()}
        for opt in opts:
            opt.step()
        ref = float(g[pre + 'loss'])
        print(f'step {s} loss: {float(losses[0].detach()):.8g} reference {ref:.8g} rel {_rel(losses[0].detach(), ref):.2e}')
        assert _rel(losses[0].detach(), ref) < 2e-5 or abs(float(losses[0].detach()) - ref) < 2e-6
        allm = {**metrics, **gm}
        assert set(metrics) == expect
        assert {k[len(pre + 'metric_'):] for k in g if k.startswith(pre + 'metric_')} == set(allm)
        for k in allm:
            assert allm[k].dim() == 0 and allm[k].is_cuda, k
            print(f'step {s} {k}: {float(allm[k]):.8g} reference {float(g[pre + "metric_" + k]):.8g}')
            _check_metric(allm[k], g[pre + 'metric_' + k], (s, k))
        assert math.isnan(float(metrics['mse_goal_age1000']))
        stored = [k[len(pre + 'tensor_'):] for k in g if k.startswith(pre + 'tensor_')]
        assert set(stored) == set(tensors)
        for k in stored:
            ref = torch.from_numpy(g[pre + 'tensor_' + k])
            assert tensors[k].shape == ref.shape, k
            _close_rt(tensors[k], ref, 1e-4, 1e-4 * max(1.0, float(ref.abs().max())), f'step {s} {k}')
        if 'map' in pm:
            assert torch.equal(tensors['acc_map'].cpu(), torch.from_numpy(g[pre + 'tensor_acc_map'])), f'step {s}: acc_map per frame'
        ref = torch.from_numpy(g[pre + 'out_state'])
        _close_rt(state, ref, 1e-4, 1e-4 * max(1.0, float(ref.abs().max())), f'step {s} out_state')
        names = [str(n) for n in g[pre + 'grad_names']]
        assert names == list(grads)
        for n, ref in zip(names, g[pre + 'grad_norms']):
            got = float(grads[n].double().norm())
            assert abs(got - ref) <= 2e-3 * ref + 1e-7, (s, n, got, ref)
        full = [k for k in g if k.startswith(pre + 'grad_') and k not in (pre + 'grad_names', pre + 'grad_norms')]
        assert len(full) == 5
        for k in full:
            e = _rel_l2(grads[k[len(pre + 'grad_'):]], torch.from_numpy(g[k]))
            print(f'step {s} full gradient {k[len(pre + "grad_"):]}: relative L2 error {e:.3e}')
            assert e < 2e-3, (s, k, e)
        sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
        np.testing.assert_allclose(sums, g[pre + 'param_abs_sums'], rtol=2e-6)


def _one_step(model, oconf, obs, state):
    opts = model._opts
    losses, out_state, metrics, tensors, _ = model.training_step(obs, state)
    for opt in opts:
        opt.zero_grad()
    losses[0].backward()
    model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
    torch.cuda.synchronize()
    return losses[0].detach().clone(), out_state.clone(), opts[0].flat_grad.clone(), metrics, tensors


@pytest.mark.parametrize('name', FIXTURES)
def test_exact_properties_of_a_step(hip, name):
    """From the same state: a repeated step is bit-identical (loss, out_state, every gradient); under no_grad the loss has the same
    bits, carries no graph and no gradient buffer is written; out_state is the last step's features; a batch whose only difference
    is a mid-sequence reset gives the same bits (mid-sequence resets are not read); uint8 frames work as the float frames do; a
    missing action_next raises; a second backward() raises."""
    g = _gold(name)
    oconf, model = _model(g)
    model._opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs = _obs(g, 's0_', oconf, model)
    state = (0.1 * torch.randn(1, oconf.batch_size, oconf.deter_dim, generator=torch.Generator().manual_seed(2))).to(DEV)
    la, sa, ga, ma, ta = _one_step(model, oconf, obs, state)
    lb, sb, gb, mb, tb = _one_step(model, oconf, obs, state)
    assert torch.equal(la, lb) and torch.equal(sa, sb) and torch.equal(ga, gb) and float(ga.abs().sum()) > 0
    # reset[0] masks the carried state: the row it resets equals a zero row of the state
    r0 = obs['reset'][0]
    assert bool(r0.any()) and not bool(r0.all())
    zeroed = state.clone()
    zeroed[0, r0] = 0
    lz, sz, gz, _, _ = _one_step(model, oconf, obs, zeroed)
    assert torch.equal(la, lz) and torch.equal(sa, sz) and torch.equal(ga, gz)
    # mid-sequence resets are not read
    other = dict(obs, reset=obs['reset'].clone())
    other['reset'][1:] = ~other['reset'][1:]
    lc, sc, gc, _, _ = _one_step(model, oconf, other, state)
    assert torch.equal(la, lc) and torch.equal(sa, sc) and torch.equal(ga, gc)
    # no_grad
    model._opts[0].flat_grad.fill_(3.0)
    with torch.no_grad():
        losses, s0, m0, t0, _ = model.training_step(obs, state)
    torch.cuda.synchronize()
    assert not losses[0].requires_grad and torch.equal(losses[0], la) and torch.equal(s0, sa)
    assert bool((model._opts[0].flat_grad == 3.0).all()), 'a no_grad step wrote gradients'
    same = lambda x, y: torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0))
    assert list(m0) == list(ma) and all(same(m0[k], ma[k]) for k in ma)
    assert list(t0) == list(ta) and all(same(t0[k], ta[k]) for k in ta)
    # uint8 frames: the same preprocessing inside the first convolution
    u8 = _obs(g, 's0_', oconf, model, u8=True)
    with torch.no_grad():
        lu = model.training_step(u8, state)[0][0]
    assert _rel(lu, la) < 2e-5
    # the flags and imag_horizon have no effect
    with torch.no_grad():
        lf = model.training_step(obs, state, 1, 7, True, True, True)[0][0]
    assert torch.equal(lf, la)
    with pytest.raises(ValueError):
        model.training_step({k: v for k, v in obs.items() if k != 'action_next'}, state)
    losses, s1, _, _, _ = model.training_step(obs, state)
    B, D_ = oconf.batch_size, oconf.deter_dim
    assert torch.equal(model._last_pack['Hs'][-B:].view(1, B, D_), s1), 'out_state is H[T - 1]'
    losses[0].backward()
    with pytest.raises(RuntimeError):
        losses[0].backward()


def test_state_dict_round_trip(hip):
    g = _gold('tiny_gru_probe_goals')
    oconf, model = _model(g)
    model.init_optimizers(oconf.adam_lr, eps=oconf.adam_eps)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want = CFP.make_params(CFP.shapes_of_fixture(g), seed=0)
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in want)
    model.load_state_dict({k: v + 1 for k, v in sd.items()}, strict=True)
    assert all(torch.equal(v.cpu(), sd[k] + 1) for k, v in model.state_dict().items())
