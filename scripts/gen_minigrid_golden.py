"""Golden vectors for the dense categorical image path: the `minigrid` section (defaults.yaml:122-141) - DenseEncoder
(encoders.py:99-125) on the one-hot image with the reward / terminal planes, CatImageDecoder (decoders.py:183-254) as the image
decoder, with and without image_decoder_min_prob.

    python scripts/gen_minigrid_golden.py      # writes tests/golden/tiny_minigrid.npz (+ _grads), tiny_minigrid_minprob.npz,
                                               # tiny_minigrid_eval.npz and tiny_minigrid_inference.npz

Runs the REAL reference on CPU, imported in place as scripts/gen_goals_probe_golden.py does (only where the reference checkout
exists), at the tiny dimensions of `oracle.tiny_conf()` with image_size=7, image_channels=4, action_dim=7 and the small map of
gen_map_probe_golden.MAP: trainer iterations with carried state (train.py:165-198), data-only fixtures.  Weights are never
stored: both sides compute them with tests/closed_form_params.py from the ordered {name: shape} map of the reference's
state_dict, which the fixture records.  Class images are stored as uint8 (T,B,S,S) and fed one-hot.

Sampled indices must be EQUAL: the noise seed is advanced until every uniform lies more than 1e-5 from the nearest edge of the
reference's CDF (the rule of gen_obs_golden.py); with the map probe the top-two-gap rule of gen_map_probe_golden.py holds too.

Every run is repeated with the model and every floating input in float64 (the same uniforms, which must draw the same indices).
Per class of compared quantity the fixture stores `fp64_dev_<class>`: the largest deviation of the fp32 reference from that run
as a FRACTION OF THE BAR the GPU test applies to the class (tests/test_gpu_minigrid.py BARS; 1.0 = the reference alone would
sit on the bar).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from oracle import dreamer_oracle as O                                   # noqa: E402
from oracle.gen_golden import REF, reference_conf                        # noqa: E402
import closed_form_params as CFP                                         # noqa: E402
from gen_obs_golden import MIN_EDGE, MarginPatch, make_batch, tiny_overrides      # noqa: E402
from gen_map_probe_golden import MAP, MIN_GAP, map_inputs, map_obs       # noqa: E402

GRID = dict(image_size=7, image_channels=4, action_dim=7)
MAIN = dict(MAP, reward_input=True, image_decoder_min_prob=0)
MINPROB = dict(probe_model='none', reward_input=False, image_decoder_min_prob=0.05)
ENC_FIRST = 'wm.encoder.encoder_image.model.1.weight'

# the bars of the GPU test, as (relative, absolute) pairs; `either`: rel OR abs suffices, else err <= rel * |ref| + abs
BARS = dict(losses=(2e-5, 2e-6, 'either'), metrics=(1e-4, 5e-6, 'either'), tensors=(1e-4, 1e-4, 'sum'), grad_norms=(2e-3, 1e-7, 'sum'),
            full_grads=(2e-3, 0.0, 'l2'), param_abs_sums=(2e-6, 0.0, 'sum'))


def bar_fraction(kind, got, ref):
    """Largest err / bar over the elements of one quantity (got: the fp32 run, ref: the float64 run)."""
    rel, ab, mode = BARS[kind]
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    keep = ~(np.isnan(got) & np.isnan(ref))
    got, ref = got[keep], ref[keep]
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    if mode == 'l2':
        return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30) / rel)
    if mode == 'either':
        return float(np.max(np.minimum(err / np.maximum(rel * np.abs(ref), 1e-300), err / ab)))
    if kind == 'tensors':
        ab = ab * max(1.0, float(np.abs(ref).max()))
    return float(np.max(err / (rel * np.abs(ref) + ab)))


class KeepDouble:
    """The reference forces float32 with `.float()` at three places (rssm.py:199, a2c.py:44, decoders.py:265: its AMP guards).  Inside
    this context `.float()` leaves a float64 tensor as it is, so the float64 pass stays float64 end to end."""

    def __init__(self, on):
        self.on, self.orig = on, torch.Tensor.float

    def __enter__(self):
        if self.on:
            orig = self.orig
            torch.Tensor.float = lambda t, *a, **k: t if t.dtype == torch.float64 else orig(t, *a, **k)

    def __exit__(self, *a):
        torch.Tensor.float = self.orig


def grid_batch(oconf, step):
    """gen_obs_golden.make_batch without its frames, plus a random class image (T,B,S,S) uint8."""
    raw = make_batch(oconf, step)
    del raw['image_u8']
    T, B, C, S = oconf.batch_length, oconf.batch_size, oconf.image_channels, oconf.image_size
    raw['image_classes'] = np.random.RandomState(2468 + step).randint(0, C, (T, B, S, S)).astype(np.uint8)
    return raw


def grid_obs(raw, oconf, dtype=torch.float32):
    onehot = torch.nn.functional.one_hot(torch.from_numpy(raw['image_classes'].astype(np.int64)), oconf.image_channels)
    return dict(image=onehot.permute(0, 1, 4, 2, 3).contiguous().to(dtype),                   # img_to_onehot, preprocessing.py:15-18
                action=torch.nn.functional.one_hot(torch.from_numpy(raw['action_idx']), oconf.action_dim).to(dtype),
                reward=torch.from_numpy(raw['reward']).to(dtype), terminal=torch.from_numpy(raw['terminal']).to(dtype),
                reset=torch.from_numpy(raw['reset']))


def _setup(overrides):
    torch.set_num_threads(8)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import torch.distributions as D
    D.Distribution.set_default_validate_args(False)   # train.py:30
    rconf = reference_conf(['defaults', 'minigrid'], tiny_overrides(**{**GRID, **overrides}))
    oconf = O.make_conf(**{k: getattr(rconf, k) for k in O.DEFAULTS})
    return rconf, oconf


def _model(rconf, dtype):
    from pydreamer.models import Dreamer          # the reference, imported in place
    torch.manual_seed(0)
    model = Dreamer(rconf)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    return model.to(dtype), shapes


def _header(oconf, extra_conf, shapes):
    nd = max(len(s) for s in shapes.values())
    return {'conf_json': np.array(repr(sorted(vars(oconf).items()))), 'extra_conf_json': np.array(repr(sorted(extra_conf.items()))),
            'param_names': np.array(list(shapes.keys())),
            'param_shapes': np.array([list(s) + [-1] * (nd - len(s)) for s in shapes.values()], dtype=np.int64)}


def _full_obs(rconf, oconf, raw, step, dtype):
    obs, extra = grid_obs(raw, oconf, dtype), {}
    if 'map' in rconf.probe_model:
        extra = map_inputs(rconf, step)
        obs.update({k: v.to(dtype) if v.is_floating_point() else v for k, v in map_obs(extra, rconf.map_channels).items()})
    return obs, extra


def _iterate(rconf, oconf, steps, noise_seed, dtype):
    """Trainer iterations in `dtype`: (records per step, shapes, min edge distance, min map_rec gap)."""
    model, shapes = _model(rconf, dtype)
    optimizers = model.init_optimizers(rconf.adam_lr, rconf.adam_lr_actor, rconf.adam_lr_critic, rconf.adam_eps)
    T, B, S, H = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon
    with_map = 'map' in rconf.probe_model
    state = tuple(x.to(dtype) for x in model.init_state(B))
    records, min_edge, min_gap = [], float('inf'), float('inf')
    dec_last = f'wm.decoder.image.model.{3 * rconf.image_decoder_layers}.weight'
    for step in range(steps):
        raw = grid_batch(oconf, step)
        obs, extra = _full_obs(rconf, oconf, raw, step, dtype)
        noise = O.make_noise(oconf, seed=noise_seed + step)
        with MarginPatch() as mp, KeepDouble(dtype == torch.float64):
            mp.queue += [noise['u_post'][t] for t in range(T)]
            for i in range(H):
                mp.queue += [noise['u_act'][i], noise['u_prior'][i]]
            losses, new_state, metrics, tensors, _ = model.training_step(obs, state)
            assert not mp.queue, f'{len(mp.queue)} uniforms unused'
            post_idx = torch.stack(mp.idx[:T]).reshape(T, B, S)
            act_idx = torch.stack(mp.idx[T::2]).reshape(H, T * B)
            min_edge = min(min_edge, mp.min_edge)
        if with_map:
            top2 = tensors['map_rec'].detach().double().topk(2, dim=2).values
            min_gap = min(min_gap, float((top2[:, :, 0] - top2[:, :, 1]).min()))
        for opt in optimizers:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        grad_metrics = model.grad_clip(rconf.grad_clip, rconf.grad_clip_ac)
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        for opt in optimizers:
            opt.step()
        image_side = [k for k in grads if k.startswith(('wm.encoder.', 'wm.decoder.image.'))]
        post = dict(model.state_dict())
        records.append(dict(
            inputs={**raw, **extra}, noise={k: noise[k].numpy() for k in ('u_post', 'u_act', 'u_prior')},
            losses=np.array([float(l.detach()) for l in losses], dtype=np.float64),
            metrics={k: float(v) for k, v in {**metrics, **grad_metrics}.items()},
            tensors={k: tensors[k].detach().clone() for k in ('image_rec', 'loss_image')},
            out_state_h=new_state[0].detach().clone(), idx_post=post_idx, idx_act=act_idx,
            grad_names=image_side, grad_norms=np.array([float(grads[k].double().norm()) for k in image_side]),
            grads={k: grads[k] for k in (ENC_FIRST, dec_last)},
            param_abs_sums=np.array([float(v.double().abs().sum()) for v in post.values()])))
        state = new_state
    return records, shapes, min_edge, min_gap


def run(name, overrides, steps, grads_file=False):
    """grads_file: the two full gradients, of the first step only, go to a companion <name>_grads.npz (every file stays under
    1 MiB, as gen_obs_golden.py does for tiny_vecobs); their float64 deviation is taken over every step all the same."""
    rconf, oconf = _setup(overrides)
    with_map = 'map' in rconf.probe_model
    seed = 777
    while True:
        print(f'[{name}] noise seed {seed}')
        rec32, shapes, min_edge, min_gap = _iterate(rconf, oconf, steps, seed, torch.float32)
        if min_edge > MIN_EDGE and (not with_map or min_gap > MIN_GAP):
            break
        print(f'[{name}] edge distance {min_edge:.2e} (need > {MIN_EDGE}), map_rec top-two gap {min_gap:.2e} (need > {MIN_GAP}): next seed')
        seed += 1000
    rec64, _, _, _ = _iterate(rconf, oconf, steps, seed, torch.float64)
    out = dict(_header(oconf, overrides, shapes), noise_seed=np.array(seed), min_edge_distance=np.array(min_edge))
    if with_map:
        out['min_map_rec_gap'] = np.array(min_gap)
    dev = {k: 0.0 for k in BARS}
    for step, (a, b) in enumerate(zip(rec32, rec64)):
        pre = f's{step}_'
        assert torch.equal(a['idx_post'], b['idx_post']) and torch.equal(a['idx_act'], b['idx_act']), 'float64 drew other indices'
        for k, v in {**a['inputs'], **a['noise']}.items():
            out[pre + 'in_' + k] = v
        out[pre + 'losses'] = a['losses']
        for k, v in a['metrics'].items():
            out[pre + 'metric_' + k] = np.array(v, dtype=np.float64)
        for k, v in a['tensors'].items():
            out[pre + 'tensor_' + k] = v.numpy()
        out[pre + 'out_state_h'] = a['out_state_h'].numpy()
        out[pre + 'idx_post'] = a['idx_post'].numpy().astype(np.uint8)
        out[pre + 'idx_act'] = a['idx_act'].numpy().astype(np.uint8)
        out[pre + 'grad_names'], out[pre + 'grad_norms'] = np.array(a['grad_names']), a['grad_norms']
        for k, v in a['grads'].items():
            out[pre + 'grad_' + k] = v.numpy()
        out[pre + 'param_abs_sums'] = a['param_abs_sums']
        assert min(a['grad_norms']) > 0, 'a gradient of the image path is zero'
        dev['losses'] = max(dev['losses'], bar_fraction('losses', a['losses'], b['losses']))
        for k, v in a['metrics'].items():
            assert np.isnan(v) == np.isnan(b['metrics'][k]), k
            dev['metrics'] = max(dev['metrics'], bar_fraction('metrics', v, b['metrics'][k]))
        for k, v in a['tensors'].items():
            dev['tensors'] = max(dev['tensors'], bar_fraction('tensors', v.numpy(), b['tensors'][k].numpy()))
        dev['grad_norms'] = max(dev['grad_norms'], bar_fraction('grad_norms', a['grad_norms'], b['grad_norms']))
        for k, v in a['grads'].items():
            dev['full_grads'] = max(dev['full_grads'], bar_fraction('full_grads', v.numpy(), b['grads'][k].numpy()))
        dev['param_abs_sums'] = max(dev['param_abs_sums'], bar_fraction('param_abs_sums', a['param_abs_sums'], b['param_abs_sums']))
        print(f'  step {step}: losses', a['losses'], 'loss_image', a['metrics']['loss_image'], 'grad_norm', a['metrics']['grad_norm'])
    for k, v in dev.items():
        out['fp64_dev_' + k] = np.array(v)
    print(f'[{name}] fp32 reference against float64, fraction of each bar:', {k: f'{v:.2e}' for k, v in dev.items()})
    if grads_file:
        full = {k: out.pop(k) for k in list(out) if k[3:].startswith('grad_wm.')}
        _save(name + '_grads', {k: v for k, v in full.items() if k.startswith('s0_')})
    _save(name, out)


def _save(name, out):
    path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print('wrote', path, f'{size / 1024:.0f} KiB')


def _eval_pass(rconf, oconf, seed, dtype, do_open_loop):
    model, shapes = _model(rconf, dtype)
    T, B, S, H = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon
    raw = grid_batch(oconf, 0)
    obs, extra = _full_obs(rconf, oconf, raw, 0, dtype)
    noise = O.make_noise(oconf, seed=seed)
    with MarginPatch() as mp, torch.no_grad(), KeepDouble(dtype == torch.float64):
        mp.queue = [noise['u_post'][t] for t in range(T)] + [noise['u_pred'].reshape(-1, S)]
        for i in range(H):
            mp.queue += [noise['u_act'][i], noise['u_prior'][i]]
        for i in range(T - 1):
            mp.queue += [noise['u_act_log'][i], noise['u_prior_log'][i]]
        losses, _, metrics, tensors, dream = model.training_step(obs, tuple(x.to(dtype) for x in model.init_state(B)), do_image_pred=True, do_dream_tensors=True,
                                                                 do_open_loop=do_open_loop)
        assert not mp.queue
    keep = {k: v.detach().clone() for k, v in tensors.items() if k.startswith('logprob_') or k == 'image_pred'}
    return dict(inputs={**raw, **extra}, noise={k: noise[k].numpy() for k in ('u_post', 'u_act', 'u_prior', 'u_pred', 'u_act_log', 'u_prior_log')},
                metrics={k: float(v) for k, v in metrics.items() if k.startswith('logprob_')}, tensors=keep,
                dream_image_pred=dream['image_pred'].detach().clone(), idx=[i.clone() for i in mp.idx], edge=mp.min_edge), shapes


def run_eval(name, overrides):
    """training_step under no_grad with do_image_pred and do_dream_tensors (train.py:353-359,380-385), then with do_open_loop added:
    every logprob_* metric and tensor, image_pred, and the log dream's raw-logit image_pred (dreamer.py:171).  Keys `cl_` / `ol_`."""
    rconf, oconf = _setup(overrides)
    out, dev, edge = None, 0.0, float('inf')
    for tag, open_loop in (('cl_', False), ('ol_', True)):
        seed = 999
        while True:
            a, shapes = _eval_pass(rconf, oconf, seed, torch.float32, open_loop)
            if a['edge'] > MIN_EDGE:
                break
            print(f'[{name}] {tag}: a uniform lies {a["edge"]:.2e} from a CDF edge: next seed')
            seed += 1000
        b, _ = _eval_pass(rconf, oconf, seed, torch.float64, open_loop)
        assert all(torch.equal(x, y) for x, y in zip(a['idx'], b['idx'])), 'float64 drew other indices'
        if out is None:
            out = _header(oconf, overrides, shapes)
        T, B, S = rconf.batch_length, rconf.batch_size, rconf.stoch_dim
        out[tag + 'noise_seed'] = np.array(seed)
        for k, v in {**a['inputs'], **a['noise']}.items():
            out[tag + 'in_' + k] = v
        for k, v in a['metrics'].items():
            assert np.isnan(v) == np.isnan(b['metrics'][k]), k
            out[tag + 'metric_' + k] = np.array(v, dtype=np.float64)
            dev = max(dev, bar_fraction('metrics', v, b['metrics'][k]))
        for k, v in a['tensors'].items():
            out[tag + 'tensor_' + k] = v.numpy()
            dev = max(dev, bar_fraction('tensors', v.numpy(), b['tensors'][k].numpy()))
        out[tag + 'dream_image_pred'] = a['dream_image_pred'].numpy()
        dev = max(dev, bar_fraction('tensors', a['dream_image_pred'].numpy(), b['dream_image_pred'].numpy()))
        out[tag + 'idx_post'] = torch.stack(a['idx'][:T]).reshape(T, B, S).numpy().astype(np.uint8)
        out[tag + 'idx_pred'] = a['idx'][T].reshape(T, B, S).numpy().astype(np.uint8)
        edge = min(edge, a['edge'])
        print(f'[{name}] {tag}:', {k: round(v, 6) for k, v in a['metrics'].items()})
    out['min_edge_distance'] = np.array(edge)
    out['fp64_dev_eval'] = np.array(dev)
    print(f'[{name}] fp32 reference against float64, fraction of the metric / tensor bars: {dev:.2e}')
    _save(name, out)


def _inference_pass(rconf, seed, dtype):
    model, shapes = _model(rconf, dtype)
    B, S, C, A = 3, rconf.stoch_dim, rconf.stoch_discrete, rconf.action_dim
    g = torch.Generator().manual_seed(seed)
    classes = torch.randint(0, rconf.image_channels, (1, B, rconf.image_size, rconf.image_size), generator=g)
    image = torch.nn.functional.one_hot(classes, rconf.image_channels).permute(0, 1, 4, 2, 3).contiguous().to(dtype)
    action = torch.nn.functional.one_hot(torch.randint(0, A, (1, B), generator=g), A).to(dtype)
    reset = torch.tensor([[True, False, False]])
    h = torch.tanh(torch.randn(B, rconf.deter_dim, generator=g))
    z = torch.nn.functional.one_hot(torch.randint(0, C, (B, S), generator=g), C).float().reshape(B, S * C)
    u = torch.rand(1, B, S, generator=g)
    reward = torch.tanh(torch.randn(1, B, generator=g))
    terminal = torch.tensor([[0.0, 1.0, 0.0]])
    obs = dict(image=image, action=action, reset=reset, reward=reward.to(dtype), terminal=terminal.to(dtype))
    with MarginPatch() as mp, torch.no_grad(), KeepDouble(dtype == torch.float64):
        mp.queue = [u[0]]
        dist, (h1, z1), metrics = model.inference(obs, (h.to(dtype), z.to(dtype)))
        assert not mp.queue
    ins = dict(in_image_classes=classes.numpy().astype(np.uint8), in_action=action.float().numpy(), in_reset=reset.numpy(),
               in_reward=reward.numpy(), in_terminal=terminal.numpy(), in_h=h.numpy(), in_z=z.numpy(), in_u=u.numpy())
    outs = dict(action_logits=dist.logits.detach().clone(), out_h=h1.detach().clone(), out_z=z1.detach().clone(),
                policy_value=metrics['policy_value'].detach().reshape(1).clone())
    return ins, outs, mp.min_edge, shapes


def run_inference(name, overrides):
    """Dreamer.inference (dreamer.py:92-111): one step on (1,B,...) observations with the posterior draw pinned; the normalised
    action logits of the returned OneHotCategorical, out_state and policy_value."""
    rconf, oconf = _setup(overrides)
    seed = 31
    while True:
        ins, a, edge, shapes = _inference_pass(rconf, seed, torch.float32)
        if edge > MIN_EDGE:
            break
        seed += 1000
    _, b, _, _ = _inference_pass(rconf, seed, torch.float64)
    assert torch.equal(a['out_z'].double(), b['out_z'])
    out = dict(_header(oconf, overrides, shapes), **ins, min_edge_distance=np.array(edge))
    out.update({k: v.numpy() for k, v in a.items()})
    out['fp64_dev_inference'] = np.array(max(bar_fraction('tensors', a[k].numpy(), b[k].numpy()) for k in a))
    print(f'[{name}] fp32 reference against float64, fraction of the tensor bar: {float(out["fp64_dev_inference"]):.2e}')
    _save(name, out)


if __name__ == '__main__':
    which = sys.argv[1:] or ['tiny_minigrid', 'tiny_minigrid_minprob', 'tiny_minigrid_eval', 'tiny_minigrid_inference']
    if 'tiny_minigrid' in which:
        run('tiny_minigrid', MAIN, steps=2, grads_file=True)
    if 'tiny_minigrid_minprob' in which:
        run('tiny_minigrid_minprob', MINPROB, steps=1)
    if 'tiny_minigrid_eval' in which:
        run_eval('tiny_minigrid_eval', MAIN)
    if 'tiny_minigrid_inference' in which:
        run_inference('tiny_minigrid_inference', MAIN)
