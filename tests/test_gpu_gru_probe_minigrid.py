"""-m gpu: WorldModelProbe(model='gru_probe') on the dense encoder of the `minigrid` section against the reference-written fixtures
tests/golden/tiny_gru_probe_minigrid.npz (reward_input, LayerNorm, three encoder layers: in_dim 294) and
tiny_gru_probe_minigrid_plain.npz (no planes, no LayerNorm, one layer: in_dim 196) of scripts/gen_gru_probe_minigrid_golden.py:
two trainer iterations with carried state and optimizer steps.

Bars: those of tests/test_gpu_gru_probe.py, unchanged - loss 2e-5 relative (or 2e-6), metrics 1e-4 relative (or 5e-6) with NaN
where the reference has NaN, tensors and out_state 1e-4 relative + 1e-4 max(1, max |ref|), gradient norms (every parameter, and
grad_norm) 2e-3 relative + 1e-7, the stored full gradients 2e-3 relative L2, parameter |.| sums after the optimizer step 2e-6
relative, acc_map per frame exactly.  tests/test_gru_probe_minigrid_cpu.py holds the reference's own fp32-vs-fp64 deviation to a
quarter of each bar.
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
FIXTURES = ['tiny_gru_probe_minigrid', 'tiny_gru_probe_minigrid_plain']
ENC_FIRST = 'wm.encoder.encoder_image.model.1.weight'
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
    assert not (err > bound).any() and not torch.isnan(err).any(), \
        f'{what}: {int((err > bound).sum())}/{err.numel()} mismatches, max err {float(err.max()):.3e}'


def _check_metric(got, ref, what):
    got, ref = float(got), float(ref)
    if math.isnan(ref) or math.isnan(got):
        assert math.isnan(ref) and math.isnan(got), (what, got, ref)
    else:
        assert _rel(got, ref) < 1e-4 or abs(got - ref) < 5e-6, (what, got, ref)


def _model(g):
    from pydreamer_amd import config
    from pydreamer_amd.models import DenseEncoder, WorldModelProbe
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    model = WorldModelProbe(config.load_config('defaults', 'minigrid', **{**vars(oconf), **extra}))
    assert model.dense and isinstance(model.wm.encoder.encoder_image, DenseEncoder)
    shapes = CFP.shapes_of_fixture(g)
    assert list(model.state_dict().keys()) == list(shapes.keys())
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    return oconf, model.to(DEV)


def _obs(g, pre, oconf, model, class_map=False):
    classes = torch.from_numpy(g[pre + 'in_image_classes'].astype(np.int64))
    image = classes if class_map else F.one_hot(classes, oconf.image_channels).permute(0, 1, 4, 2, 3).float().contiguous()
    mc = torch.from_numpy(g[pre + 'in_map_classes'].astype(np.int64))
    obs = dict(image=image, reward=torch.from_numpy(g[pre + 'in_reward']), terminal=torch.from_numpy(g[pre + 'in_terminal']),
               reset=torch.from_numpy(g[pre + 'in_reset']), action_next=torch.from_numpy(g[pre + 'in_action_next']),
               map=F.one_hot(mc, model.conf.map_channels).permute(0, 1, 4, 2, 3).float().contiguous(),
               map_coord=torch.from_numpy(g[pre + 'in_map_coord']), map_seen_mask=torch.from_numpy(g[pre + 'in_map_seen_mask']))
    return {k: v.to(DEV) for k, v in obs.items()}


@pytest.mark.parametrize('name', FIXTURES)
def test_training_steps_match_the_reference(hip, name):
    g = _gold(name)
    oconf, model = _model(g)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    assert len(opts) == 1 and [id(p) for p in opts[0]._plist] == [id(p) for p in model.parameters()]
    state = model.init_state(oconf.batch_size)
    assert tuple(state.shape) == (1, oconf.batch_size, oconf.deter_dim) and not state.any()
    enc = model.wm.encoder.encoder_image
    assert enc.in_dim == (196 if name.endswith('plain') else 294) and enc.layer_norm == (not name.endswith('plain'))
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
        assert set(metrics) == {'loss_map', 'acc_map', 'acc_map_seen'}
        assert {k[len(pre + 'metric_'):] for k in g if k.startswith(pre + 'metric_')} == set(allm)
        for k in allm:
            assert allm[k].dim() == 0 and allm[k].is_cuda, k
            print(f'step {s} {k}: {float(allm[k]):.8g} reference {float(g[pre + "metric_" + k]):.8g}')
            _check_metric(allm[k], g[pre + 'metric_' + k], (s, k))
        stored = [k[len(pre + 'tensor_'):] for k in g if k.startswith(pre + 'tensor_')]
        assert set(stored) == set(tensors) == {'map_rec', 'loss_map', 'acc_map'}
        for k in stored:
            ref = torch.from_numpy(g[pre + 'tensor_' + k])
            assert tensors[k].shape == ref.shape, k
            _close_rt(tensors[k], ref, 1e-4, 1e-4 * max(1.0, float(ref.abs().max())), f'step {s} {k}')
        assert torch.equal(tensors['acc_map'].cpu(), torch.from_numpy(g[pre + 'tensor_acc_map'])), f'step {s}: acc_map per frame'
        ref = torch.from_numpy(g[pre + 'out_state'])
        _close_rt(state, ref, 1e-4, 1e-4 * max(1.0, float(ref.abs().max())), f'step {s} out_state')
        names = [str(n) for n in g[pre + 'grad_names']]
        assert names == list(grads)
        for n, ref in zip(names, g[pre + 'grad_norms']):
            got = float(grads[n].double().norm())
            assert abs(got - ref) <= 2e-3 * ref + 1e-7, (s, n, got, ref)
        full = [k[len(pre + 'grad_'):] for k in g if k.startswith(pre + 'grad_') and k not in (pre + 'grad_names', pre + 'grad_norms')]
        # (the encoder's first Linear is stored at the first step only: the generator's header says why)
        assert len(full) == (5 if s == 0 else 4) and (ENC_FIRST in full) == (s == 0)
        assert {'wm.rnn.weight_hh_l0', 'wm.rnn.weight_ih_l0', 'wm.squeeze.weight'} <= set(full)
        for n in full:
            e = _rel_l2(grads[n], torch.from_numpy(g[pre + 'grad_' + n]))
            print(f'step {s} full gradient {n}: relative L2 error {e:.3e}')
            assert e < 2e-3, (s, n, e)
        sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
        np.testing.assert_allclose(sums, g[pre + 'param_abs_sums'], rtol=2e-6)


def _one_step(g, class_map=False, grad=True):
    oconf, model = _model(g)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs = _obs(g, 's0_', oconf, model, class_map=class_map)
    state = (0.1 * torch.randn(1, oconf.batch_size, oconf.deter_dim, generator=torch.Generator().manual_seed(2))).to(DEV)
    if not grad:
        opts[0].flat_grad.fill_(3.0)
        with torch.no_grad():
            losses, out_state, metrics, tensors, _ = model.training_step(obs, state)
        torch.cuda.synchronize()
        return model, opts, losses, out_state, tensors
    losses, out_state, metrics, tensors, _ = model.training_step(obs, state)
    opts[0].zero_grad()
    losses[0].backward()
    model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
    grad = opts[0].flat_grad.clone()
    opts[0].step()
    torch.cuda.synchronize()
    return losses, out_state.clone(), grad, opts[0].flat_param.clone(), {k: v.clone() for k, v in tensors.items()}


@pytest.mark.parametrize('name', FIXTURES)
def test_exact_properties_of_a_step(hip, name):
    """The integer class map and the float one-hot image give bit-identical loss, out_state, gradients, parameters after the step and
    tensors; a second backward() raises; under no_grad the loss and tensors have the same bits, no gradient is written and no
    backward pack is kept."""
    g = _gold(name)
    la, sa, ga, pa, ta = _one_step(g)
    assert float(ga.abs().sum()) > 0
    lb, sb, gb, pb, tb = _one_step(g, class_map=True)
    assert torch.equal(la[0].detach(), lb[0].detach()) and torch.equal(sa, sb)
    assert torch.equal(ga, gb), 'the class map changes gradients'
    assert torch.equal(pa, pb), 'the class map changes the parameters after the step'
    assert list(ta) == list(tb) and all(torch.equal(ta[k], tb[k]) for k in ta)
    with pytest.raises(RuntimeError):
        la[0].backward()
    for class_map in (False, True):
        model, opts, ln, sn, tn = _one_step(g, class_map=class_map, grad=False)
        assert not ln[0].requires_grad and torch.equal(ln[0], la[0].detach()) and torch.equal(sn, sa)
        assert bool((opts[0].flat_grad == 3.0).all()), 'a no_grad step wrote gradients'
        assert getattr(model, '_last_pack', None) is None, 'a no_grad step kept a backward pack'
        assert list(tn) == list(ta) and all(torch.equal(tn[k], ta[k]) for k in ta)


def test_inputs_are_checked_before_any_launch(hip):
    g = _gold('tiny_gru_probe_minigrid')
    oconf, model = _model(g)
    obs = _obs(g, 's0_', oconf, model)
    state = model.init_state(oconf.batch_size)
    T, B, S, C = oconf.batch_length, oconf.batch_size, oconf.image_size, oconf.image_channels
    with torch.no_grad():
        with pytest.raises(ValueError, match='integer class map'):      # an integer 5-D image, as in WorldModel
            model.training_step(dict(obs, image=torch.zeros(T, B, S, S, C, dtype=torch.uint8, device=DEV)), state)
        for bad in (obs['image'][:, :, :-1].contiguous(), obs['image'][..., :-1].contiguous(),
                    torch.zeros(T, B, S, S + 1, dtype=torch.int64, device=DEV)):
            with pytest.raises(ValueError, match=r'\(got, expected\)'):
                model.training_step(dict(obs, image=bad), state)
        for gone in ('reward', 'terminal', 'action_next'):
            with pytest.raises(ValueError):
                model.training_step({k: v for k, v in obs.items() if k != gone}, state)
    assert getattr(model, '_last_pack', None) is None


def test_state_dict_round_trip(hip):
    g = _gold('tiny_gru_probe_minigrid_plain')
    oconf, model = _model(g)
    model.init_optimizers(oconf.adam_lr, eps=oconf.adam_eps)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want = CFP.make_params(CFP.shapes_of_fixture(g), seed=0)
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in want)
    model.load_state_dict({k: v + 1 for k, v in sd.items()}, strict=True)
    assert all(torch.equal(v.cpu(), sd[k] + 1) for k, v in model.state_dict().items())
