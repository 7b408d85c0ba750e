"""-m gpu: the dense categorical image path end to end - Dreamer(load_config('defaults', 'minigrid', tiny dims)) against the
reference-written fixtures tests/golden/tiny_minigrid*.npz (scripts/gen_minigrid_golden.py).

The bars are the project's own, those of tests/test_gpu_map_probe.py::test_training_steps_match_the_reference: sampled indices
equal, losses 2e-5 relative (or 2e-6), metrics 1e-4 relative (or 5e-6), tensors 1e-4 relative + 1e-4 max(1, max |ref|), gradient
norms 2e-3 relative + 1e-7, stored full gradients 2e-3 relative L2, parameter |.| sums 2e-6 relative.  The reference's own
float32-vs-float64 deviation stays under a quarter of each (tests/test_dense_image_cpu.py).
"""
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


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-12)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


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
    if np.isnan(ref):
        assert np.isnan(float(got)), what
        return
    assert _rel(got, ref) < 1e-4 or abs(float(got) - ref) < 5e-6, (what, float(got), ref)


def _model(g, **more):
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    model = Dreamer(config.load_config('defaults', 'minigrid', **{**vars(oconf), **extra, **more}))
    shapes = CFP.shapes_of_fixture(g)
    assert list(model.state_dict().keys()) == list(shapes.keys())
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    return oconf, model.to(DEV)


def _obs(g, pre, oconf, model, class_map=False, noise_keys=('u_post', 'u_act', 'u_prior')):
    classes = torch.from_numpy(g[pre + 'in_image_classes'].astype(np.int64))
    image = classes if class_map else F.one_hot(classes, oconf.image_channels).permute(0, 1, 4, 2, 3).float().contiguous()
    obs = dict(image=image.to(DEV), action=F.one_hot(torch.from_numpy(g[pre + 'in_action_idx']), oconf.action_dim).float().to(DEV),
               reward=torch.from_numpy(g[pre + 'in_reward']).to(DEV), terminal=torch.from_numpy(g[pre + 'in_terminal']).to(DEV),
               reset=torch.from_numpy(g[pre + 'in_reset']).to(DEV))
    if model.conf.probe_model == 'map':
        mc = torch.from_numpy(g[pre + 'in_map_classes'].astype(np.int64))
        obs.update(map=F.one_hot(mc, model.conf.map_channels).permute(0, 1, 4, 2, 3).float().contiguous().to(DEV),
                   map_coord=torch.from_numpy(g[pre + 'in_map_coord']).to(DEV),
                   map_seen_mask=torch.from_numpy(g[pre + 'in_map_seen_mask']).to(DEV))
    noise = {k: torch.from_numpy(g[pre + 'in_' + k]).to(DEV) for k in noise_keys}
    return obs, noise


@pytest.mark.parametrize('name,steps', [('tiny_minigrid', 2), ('tiny_minigrid_minprob', 1)])
def test_training_steps_match_the_reference(hip, name, steps):
    """Trainer iterations with carried state and optimizer steps on the fixture's inputs and noise; the bars of the module
    docstring.  tiny_minigrid: reward_input, the map probe, min_prob 0 (dm_cat_image_loss); tiny_minigrid_minprob: no planes, no
    probe, image_decoder_min_prob 0.05 (dm_cat_image_loss_mix)."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    gg = np.load(os.path.join(GOLD, name + '_grads.npz')) if name == 'tiny_minigrid' else g
    oconf, model = _model(g)
    assert model.wm.dense and model.wm.decoder.image.min_prob == (0.05 if name.endswith('minprob') else 0.0)
    assert float(g['min_edge_distance']) > 1e-5
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    state = model.init_state(oconf.batch_size)
    for s in range(steps):
        pre = f's{s}_'
        obs, noise = _obs(g, pre, oconf, model)
        losses, state, metrics, tensors, _ = model.training_step(obs, state, noise=noise)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        for opt in opts:
            opt.step()
        assert np.array_equal(model.last_extras['post_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_post']), (s, 'posterior indices')
        assert np.array_equal(model.last_extras['act_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_act']), (s, 'action indices')
        for i, l in enumerate(losses):
            ref = g[pre + 'losses'][i]
            print(f'step {s} loss {i}: {float(l.detach()):.8g} reference {ref:.8g} rel {_rel(l.detach(), ref):.2e}')
            assert _rel(l.detach(), ref) < 2e-5 or abs(float(l) - ref) < 2e-6, (s, i, float(l), ref)
        allm = {**metrics, **gm}
        ref_names = {k[len(pre + 'metric_'):] for k in g.files if k.startswith(pre + 'metric_')}
        assert {'loss_image', 'loss_model', 'grad_norm'} <= set(allm) <= ref_names, set(allm) ^ ref_names
        for k in allm:
            ref = float(g[pre + 'metric_' + k])
            if k in ('loss_image', 'grad_norm', 'loss_model'):
                print(f'step {s} {k}: {float(allm[k]):.8g} reference {ref:.8g} rel {_rel(allm[k], ref):.2e}')
            _check_metric(allm[k], ref, (s, k))
        for k in ('image_rec', 'loss_image'):
            _close_rt(tensors[k], torch.from_numpy(g[pre + 'tensor_' + k]), f'step {s} {k}')
        assert tensors['image_rec'].shape == obs['image'].shape
        _close_rt(state[0], torch.from_numpy(g[pre + 'out_state_h']), f'step {s} out_state h')
        names = [str(n) for n in g[pre + 'grad_names']]
        assert names == [k for k in grads if k.startswith(('wm.encoder.', 'wm.decoder.image.'))]
        for n, ref in zip(names, g[pre + 'grad_norms']):
            got = float(grads[n].double().norm())
            assert abs(got - ref) <= 2e-3 * ref + 1e-7, (s, n, got, ref)
        full = [k for k in gg.files if k.startswith(pre + 'grad_wm.')]
        assert len(full) == (2 if s == 0 or gg is g else 0)
        for k in full:
            n = k[len(pre + 'grad_'):]
            e = _rel_l2(grads[n], torch.from_numpy(gg[k]))
            print(f'step {s} full gradient {n}: relative L2 error {e:.3e}')
            assert e < 2e-3, (s, k, e)
            if n.endswith('model.1.weight') and model.conf.reward_input:      # the reward and terminal columns on their own
                cells = oconf.image_size ** 2
                for lo, what in ((-2 * cells, 'reward'), (-cells, 'terminal')):
                    sl = slice(lo, lo + cells if lo + cells else None)
                    e = _rel_l2(grads[n][:, sl], torch.from_numpy(gg[k])[:, sl])
                    print(f'step {s} {what} columns of {n}: relative L2 error {e:.3e}')
                    assert e < 2e-3, (s, what, e)
        sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
        np.testing.assert_allclose(sums, g[pre + 'param_abs_sums'], rtol=2e-6)
    names, buf, idx = model.packed_metrics()
    vals = dict(zip(names, (buf.tolist()[i] for i in idx)))
    assert vals['loss_image'] == float(metrics['loss_image'])


def _one_step(g, class_map=False, overlap=True, tail=True, grad=True):
    oconf, model = _model(g)
    model.overlap_backward, model.wm_tail_on_side = overlap, tail
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs, noise = _obs(g, 's0_', oconf, model, class_map=class_map)
    with torch.enable_grad() if grad else torch.no_grad():
        losses, _, metrics, tensors, _ = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise)
    if not grad:
        torch.cuda.synchronize()
        return model, opts, losses, tensors
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
    grads = [o.flat_grad.clone() for o in opts]
    for opt in opts:
        opt.step()
    torch.cuda.synchronize()
    return losses, grads, [o.flat_param.clone() for o in opts], tensors['image_rec'].clone(), tensors['loss_image'].clone()


@pytest.mark.parametrize('name', ['tiny_minigrid', 'tiny_minigrid_minprob'])
def test_bit_identity(hip, name):
    """(1) The float one-hot image and the integer class map give bit-identical losses, gradients, parameters and tensors.  (2) So
    do overlap_backward on / off and wm_tail_on_side on / off.  (3) A second backward() on the same losses raises."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    base = _one_step(g)
    assert float(base[1][0].abs().sum()) > 0
    for kw in (dict(class_map=True), dict(overlap=False), dict(tail=False), dict(overlap=False, tail=False, class_map=True)):
        other = _one_step(g, **kw)
        assert [float(x) for x in other[0]] == [float(x) for x in base[0]], kw
        for a, b in zip(other[1] + other[2], base[1] + base[2]):
            assert torch.equal(a, b), f'{kw} changes gradients or parameters'
        assert torch.equal(other[3], base[3]) and torch.equal(other[4], base[4]), kw
    with pytest.raises(RuntimeError):
        base[0][0].backward()


def test_no_grad_writes_no_gradient_and_inputs_are_checked(hip):
    g = np.load(os.path.join(GOLD, 'tiny_minigrid.npz'))
    model, opts, losses, tensors = _one_step(g, grad=False)
    pk = model.wm._last_pack
    assert not losses[0].requires_grad and _rel(losses[0], g['s0_losses'][0]) < 2e-5
    assert pk['dlogits'] is None and pk['dec_acts'] is None and pk['enc_acts'] is None and 'pre' not in pk
    for o in opts:
        assert float(o.flat_grad.abs().sum()) == 0.0 and (o.scratch is None or float(o.scratch.abs().sum()) == 0.0)
    _close_rt(tensors['image_rec'], torch.from_numpy(g['s0_tensor_image_rec']), 'no_grad image_rec')
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    obs, noise = _obs(g, 's0_', oconf, model)
    state = model.init_state(oconf.batch_size)
    T, B, S, C = oconf.batch_length, oconf.batch_size, oconf.image_size, oconf.image_channels
    with torch.no_grad():
        for bad in (torch.zeros(T, B, S, S, C, dtype=torch.uint8, device=DEV), obs['image'][:, :, :-1].contiguous(),
                    obs['image'][..., :-1].contiguous(), torch.zeros(T, B, S, S + 1, dtype=torch.int64, device=DEV)):
            with pytest.raises(ValueError):
                model.training_step(dict(obs, image=bad), state, noise=noise)
        for gone in ('reward', 'terminal'):      # reward_input: inputs of the encoder, in inference() too
            with pytest.raises((ValueError, AssertionError)):
                model.training_step({k: v for k, v in obs.items() if k != gone}, state, noise=noise)
            with pytest.raises(ValueError):
                model.inference({k: v[:1] for k, v in obs.items() if k != gone and not k.startswith('map')}, state)


@pytest.mark.parametrize('tag', ['cl_', 'ol_'])
def test_evaluation_matches_the_reference(hip, tag):
    """training_step under no_grad with do_image_pred and do_dream_tensors (cl_), and with do_open_loop added (ol_): every logprob_*
    metric and tensor, image_pred (normalised log-probabilities from the prior-sample features) and the log dream's image_pred (the
    decoder's raw logits, dreamer.py:171)."""
    g = np.load(os.path.join(GOLD, 'tiny_minigrid_eval.npz'))
    oconf, model = _model(g)
    obs, noise = _obs(g, tag, oconf, model, noise_keys=('u_post', 'u_act', 'u_prior', 'u_pred', 'u_act_log', 'u_prior_log'))
    with torch.no_grad():
        losses, _, metrics, tensors, dream = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise, do_image_pred=True,
                                                                 do_dream_tensors=True, do_open_loop=tag == 'ol_')
    torch.cuda.synchronize()
    T, B, S = oconf.batch_length, oconf.batch_size, oconf.stoch_dim
    assert np.array_equal(model.last_extras['post_idx'].cpu().numpy().astype(np.uint8), g[tag + 'idx_post'])
    assert np.array_equal(model.last_extras['pred_idx'].view(T, B, S).cpu().numpy().astype(np.uint8), g[tag + 'idx_pred'])
    names = [k[len(tag + 'metric_'):] for k in g.files if k.startswith(tag + 'metric_')]
    assert 'logprob_image' in names and len(names) == 6
    for k in names:
        print(f'{tag}{k}: {float(metrics[k]):.8g} reference {float(g[tag + "metric_" + k]):.8g}')
        _check_metric(metrics[k], float(g[tag + 'metric_' + k]), (tag, k))
    tnames = [k[len(tag + 'tensor_'):] for k in g.files if k.startswith(tag + 'tensor_')]
    assert {'logprob_image', 'image_pred'} <= set(tnames)
    for k in tnames:
        ref = torch.from_numpy(g[tag + 'tensor_' + k])
        got = tensors[k]
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(ref)), k
        _close_rt(torch.nan_to_num(got), torch.nan_to_num(ref), f'{tag}{k}')
    assert tensors['image_pred'].shape == obs['image'].shape and dream['image_pred'].shape == obs['image'].shape
    _close_rt(dream['image_pred'], torch.from_numpy(g[tag + 'dream_image_pred']), f'{tag}dream image_pred')


def test_inference_matches_the_reference(hip):
    g = np.load(os.path.join(GOLD, 'tiny_minigrid_inference.npz'))
    oconf, model = _model(g)
    classes = torch.from_numpy(g['in_image_classes'].astype(np.int64))
    onehot = F.one_hot(classes, oconf.image_channels).permute(0, 1, 4, 2, 3).float().contiguous()
    obs = {k: torch.from_numpy(g['in_' + k]).to(DEV) for k in ('action', 'reset', 'reward', 'terminal')}
    state = (torch.from_numpy(g['in_h']).to(DEV), torch.from_numpy(g['in_z']).to(DEV))
    noise = dict(u_post=torch.from_numpy(g['in_u']).to(DEV))
    out = []
    for image in (onehot, classes):
        with torch.no_grad():
            dist, (h1, z1), metrics = model.inference(dict(obs, image=image.to(DEV)), state, noise=noise)
        torch.cuda.synchronize()
        out.append((dist.logits.clone(), h1.clone(), z1.clone(), metrics['policy_value'].clone()))
    logits, h1, z1, value = out[0]
    assert torch.equal(z1.cpu(), torch.from_numpy(g['out_z']))
    _close_rt(logits.view(g['action_logits'].shape), torch.from_numpy(g['action_logits']), 'action logits')
    _close_rt(h1, torch.from_numpy(g['out_h']), 'out_state h')
    _check_metric(value, float(g['policy_value'][0]), 'policy_value')
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b), 'the class map and its one-hot form give different bits'
