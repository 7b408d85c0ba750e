"""Golden vectors for the GRU probe baseline: WorldModelProbe(model='gru_probe') (baselines.py:19-111 with GRUEncoderOnly,
baselines.py:314-357).

    python scripts/gen_gru_probe_golden.py      # writes tests/golden/tiny_gru_probe_map_goals.npz and tiny_gru_probe_goals.npz

Runs the REAL reference on CPU, imported in place as scripts/gen_goals_probe_golden.py does (only where the reference checkout
exists), at the tiny shape of `oracle.tiny_conf()` (T 5, B 3, deter 64, action_dim 6): trainer iterations with carried state
(train.py:165-198: zero_grad, backward, grad_clip, step), data-only fixtures.  Weights are never stored: both sides compute them
with tests/closed_form_params.py from the ordered {name: shape} map of the reference's state_dict, which the fixture records.

The model draws no random numbers, so there is no seed search.  The per-frame map accuracy must be EQUAL: the two largest values
of `map_rec` must differ by more than 1e-4 in every cell of every frame (the rule of gen_map_probe_golden.py); the generator
asserts it and stores the achieved minimum.  `reset` is stored unchanged, with its mid-sequence reset, which the reference does
not read (baselines.py:339).  `action_next` is the action of the following step, zero at the last one.

The same iterations are also run with the model and every floating input in float64; for each quantity the GPU test compares,
the fixture stores the fp32 reference's own deviation from that run (`fp64_dev_*`, the maximum over the steps).
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
from gen_obs_golden import make_batch, tiny_overrides, to_obs            # noqa: E402
from gen_map_probe_golden import MAP, MIN_GAP, map_inputs, map_obs       # noqa: E402
from gen_goals_probe_golden import goals_inputs                          # noqa: E402

BASE = dict(model='gru_probe', probe_gradients=True)
MAP_GOALS = dict(MAP, probe_model='map+goals', goals_size=3, **BASE)
GOALS = dict(probe_model='goals', goals_size=3, reward_input=True, **BASE)
FULL_GRADS = ['wm.rnn.weight_hh_l0', 'wm.rnn.weight_ih_l0', 'wm.squeeze.weight', 'wm.encoder.encoder_image.model.0.weight']


def action_next(raw, A):
    """(T, B, A): the one-hot action of step t + 1, zeros at the last step."""
    onehot = np.eye(A, dtype=np.float32)[raw['action_idx']]
    return np.concatenate([onehot[1:], np.zeros_like(onehot[:1])], 0)


def _iterate(rconf, oconf, steps, dtype):
    """The trainer iterations in `dtype`; returns (records per step, ordered shapes)."""
    from pydreamer.models.baselines import WorldModelProbe          # the reference, imported in place
    torch.manual_seed(0)
    model = WorldModelProbe(rconf)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    model = model.to(dtype)
    optimizers = model.init_optimizers(rconf.adam_lr, rconf.adam_lr_actor, rconf.adam_lr_critic, rconf.adam_eps)
    assert len(optimizers) == 1
    with_map = 'map' in rconf.probe_model
    state = model.init_state(rconf.batch_size).to(dtype)
    records = []
    for step in range(steps):
        raw = make_batch(oconf, step)
        assert raw['reset'][1:].any(), 'the batch must hold a mid-sequence reset'
        extra = dict(goals_inputs(rconf, step), action_next=action_next(raw, rconf.action_dim))
        obs = dict(to_obs(raw, oconf), **{k: torch.from_numpy(v) for k, v in extra.items()})
        if with_map:
            mextra = map_inputs(rconf, step)
            extra.update(mextra)
            obs.update(map_obs(mextra, rconf.map_channels))
        obs = {k: v.to(dtype) if v.is_floating_point() else v for k, v in obs.items()}
        losses, new_state, metrics, tensors, _ = model.training_step(obs, state)
        assert len(losses) == 1
        for opt in optimizers:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        grad_metrics = model.grad_clip(rconf.grad_clip, rconf.grad_clip_ac)
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters()}
        for opt in optimizers:
            opt.step()
        post = dict(model.state_dict())
        records.append(dict(
            inputs={**raw, **extra}, loss=float(losses[0].detach()), metrics={k: float(v) for k, v in {**metrics, **grad_metrics}.items()},
            tensors={k: v.detach().clone() for k, v in tensors.items()}, out_state=new_state.detach().clone(),
            grad_names=list(grads), grad_norms=np.array([float(g.double().norm()) for g in grads.values()]),
            grads={k: grads[k] for k in FULL_GRADS + [next(k for k in grads if k.startswith('probe_model.') and grads[k].dim() == 2)]},
            param_sums=np.array([float(v.double().sum()) for v in post.values()]),
            param_abs_sums=np.array([float(v.double().abs().sum()) for v in post.values()])))
        state = new_state
    return records, shapes


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def run(name, overrides, extra_conf, steps):
    torch.set_num_threads(8)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import torch.distributions as D
    D.Distribution.set_default_validate_args(False)   # train.py:30
    rconf = reference_conf(['defaults', 'atari'], overrides)
    oconf = O.make_conf(**{k: getattr(rconf, k) for k in O.DEFAULTS})
    rec32, shapes = _iterate(rconf, oconf, steps, torch.float32)
    rec64, _ = _iterate(rconf, oconf, steps, torch.float64)
    nd = max(len(s) for s in shapes.values())
    out = {'conf_json': np.array(repr(sorted(vars(oconf).items()))), 'extra_conf_json': np.array(repr(sorted(extra_conf.items()))),
           'param_names': np.array(list(shapes.keys())),
           'param_shapes': np.array([list(s) + [-1] * (nd - len(s)) for s in shapes.values()], dtype=np.int64)}
    with_map = 'map' in rconf.probe_model
    min_gap = float('inf')
    dev = dict(loss=0.0, metrics=0.0, tensors=0.0, grad_norms=0.0, full_grads=0.0, param_abs_sums=0.0)
    for step, (a, b) in enumerate(zip(rec32, rec64)):
        pre = f's{step}_'
        for k, v in a['inputs'].items():
            out[pre + 'in_' + k] = v
        out[pre + 'loss'] = np.array(a['loss'], dtype=np.float64)
        for k, v in a['metrics'].items():
            out[pre + 'metric_' + k] = np.array(v, dtype=np.float64)
        for k, v in a['tensors'].items():
            out[pre + 'tensor_' + k] = v.numpy()
        out[pre + 'out_state'] = a['out_state'].numpy()
        out[pre + 'grad_names'] = np.array(a['grad_names'])
        out[pre + 'grad_norms'] = a['grad_norms']
        for k, v in a['grads'].items():
            out[pre + 'grad_' + k] = v.numpy()
        out[pre + 'param_sums'], out[pre + 'param_abs_sums'] = a['param_sums'], a['param_abs_sums']
        if with_map:
            top2 = a['tensors']['map_rec'].double().topk(2, dim=2).values
            min_gap = min(min_gap, float((top2[:, :, 0] - top2[:, :, 1]).min()))
        ages = {k: v for k, v in a['metrics'].items() if k.startswith('mse_goal_age')}
        assert len(ages) == 6 and np.isnan(ages['mse_goal_age1000']) and sum(np.isnan(v) for v in ages.values()) == 1, ages
        # the fp32 reference against the same iterations in float64
        dev['loss'] = max(dev['loss'], _rel(a['loss'], b['loss']))
        for k, v in a['metrics'].items():
            assert np.isnan(v) == np.isnan(b['metrics'][k]), k
            if not np.isnan(v):
                dev['metrics'] = max(dev['metrics'], _rel(v, b['metrics'][k]))
        for k, v in a['tensors'].items():
            if k != 'acc_map':
                dev['tensors'] = max(dev['tensors'], float((v.double() - b['tensors'][k]).abs().max()))
        dev['tensors'] = max(dev['tensors'], float((a['out_state'].double() - b['out_state']).abs().max()))
        if with_map:
            assert torch.equal(a['tensors']['acc_map'].double(), b['tensors']['acc_map'].double()), 'acc_map differs between fp32 and fp64'
        dev['grad_norms'] = max(dev['grad_norms'], float(np.max(np.abs(a['grad_norms'] - b['grad_norms']) / np.maximum(b['grad_norms'], 1e-30))))
        for k, v in a['grads'].items():
            dev['full_grads'] = max(dev['full_grads'], float((v.double() - b['grads'][k]).norm() / b['grads'][k].norm()))
        dev['param_abs_sums'] = max(dev['param_abs_sums'], float(np.max(np.abs(a['param_abs_sums'] - b['param_abs_sums']) / b['param_abs_sums'])))
        print(f'  step {step}: loss {a["loss"]:.8g} (fp64 {b["loss"]:.8g}) grad_norm {a["metrics"]["grad_norm"]:.6g}',
              {k: round(v, 6) for k, v in a['metrics'].items() if k.startswith(('loss_', 'acc_'))})
        assert min(a['grad_norms'][:14]) > 0, 'a world-model gradient is zero'
    for k, v in dev.items():
        out['fp64_dev_' + k] = np.array(v)
    print(f'[{name}] fp32 reference against float64:', {k: f'{v:.2e}' for k, v in dev.items()})
    if with_map:
        assert min_gap > MIN_GAP, f'map_rec top-two gap {min_gap:.2e} (need > {MIN_GAP})'
        out['min_map_rec_gap'] = np.array(min_gap)
        print(f'[{name}] map_rec top-two gap {min_gap:.2e}')
    path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, f'{os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    which = sys.argv[1:] or ['tiny_gru_probe_map_goals', 'tiny_gru_probe_goals']
    if 'tiny_gru_probe_map_goals' in which:
        run('tiny_gru_probe_map_goals', tiny_overrides(**MAP_GOALS), MAP_GOALS, steps=2)
    if 'tiny_gru_probe_goals' in which:
        run('tiny_gru_probe_goals', tiny_overrides(**GOALS), GOALS, steps=2)
