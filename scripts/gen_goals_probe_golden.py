"""Golden vectors for the goals probe: probe_model='goals' (probes.py:89-137) and 'map+goals' (probes.py:15-29).

    python scripts/gen_goals_probe_golden.py      # writes tests/golden/tiny_goals_probe.npz, tiny_goals_probe_iwae.npz
                                                  # and tiny_map_goals_probe.npz

Runs the REAL reference on CPU, imported in place as scripts/gen_map_probe_golden.py does (only where the reference checkout
exists), at the tiny shape of `oracle.tiny_conf()` with goals_size=3: trainer iterations with carried state (train.py:165-198),
data-only fixtures.  Weights are never stored: both sides compute them with tests/closed_form_params.py from the ordered
{name: shape} map of the reference's state_dict, which the fixture records.

Sampled indices must be EQUAL: the noise seed is advanced until every uniform lies more than 1e-5 from the nearest edge of the
reference's CDF (the rule of gen_obs_golden.py).  The map+goals fixture uses the map probe's tiny map settings and its top-two-gap
rule as well (gen_map_probe_golden.py).  Goal targets are N(0,1).  `goals_visage` populates five age buckets, leaves (200, 1000]
empty - mse_goal_age1000 is NaN on both sides - and holds entries of 1e5 (a goal never seen), which belong to no bucket.
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
from gen_obs_golden import MIN_EDGE, MarginPatch, make_batch, tiny_overrides, to_obs      # noqa: E402
from gen_map_probe_golden import MAP, MIN_GAP, map_inputs, map_obs       # noqa: E402

GOALS = dict(probe_model='goals', goals_size=3)
MAP_GOALS = dict(MAP, probe_model='map+goals', goals_size=3)
AGES = (0, 1, 3, 5, 6, 10, 11, 30, 50, 51, 120, 200, 1e5)      # five buckets, nothing in (200, 1000], 1e5 = never seen


def goals_inputs(rconf, step):
    T, B, G = rconf.batch_length, rconf.batch_size, rconf.goals_size
    rs = np.random.RandomState(4321 + step)
    visage = rs.choice(np.array(AGES, dtype=np.float32), size=(T, B, G))
    visage[0, 0] = (0, 120, 1e5)
    return dict(goals_direction=rs.randn(T, B, 2 * G).astype(np.float32), goal_direction=rs.randn(T, B, 2).astype(np.float32),
                goals_visage=visage.astype(np.float32))


def _attempt(rconf, oconf, extra_conf, steps, noise_seed):
    from pydreamer.models import Dreamer          # the reference, imported in place
    torch.manual_seed(0)
    model = Dreamer(rconf)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    optimizers = model.init_optimizers(rconf.adam_lr, rconf.adam_lr_actor, rconf.adam_lr_critic, rconf.adam_eps)
    T, B, S, H, I = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon, rconf.iwae_samples
    M = T * B * I
    with_map = rconf.probe_model == 'map+goals'
    nd = max(len(s) for s in shapes.values())
    out = {'conf_json': np.array(repr(sorted(vars(oconf).items()))), 'extra_conf_json': np.array(repr(sorted(extra_conf.items()))),
           'param_names': np.array(list(shapes.keys())),
           'param_shapes': np.array([list(s) + [-1] * (nd - len(s)) for s in shapes.values()], dtype=np.int64),
           'noise_seed': np.array(noise_seed)}
    state = model.init_state(B * I)
    min_edge, min_gap = float('inf'), float('inf')
    for step in range(steps):
        raw = make_batch(oconf, step)
        extra = goals_inputs(rconf, step)
        obs = dict(to_obs(raw, oconf), **{k: torch.from_numpy(v) for k, v in extra.items()})
        if with_map:
            mextra = map_inputs(rconf, step)
            extra.update(mextra)
            obs.update(map_obs(mextra, rconf.map_channels))
        noise = O.make_noise(oconf, seed=noise_seed + step)
        with MarginPatch() as mp:
            mp.queue += [noise['u_post'][t] for t in range(T)]
            for i in range(H):
                mp.queue.append(noise['u_act'][i])
                mp.queue.append(noise['u_prior'][i])
            losses, new_state, metrics, tensors, _ = model.training_step(obs, state)
            assert not mp.queue, f'{len(mp.queue)} uniforms unused'
            post_idx = torch.stack(mp.idx[:T]).reshape(T, B * I, S)
            act_idx = torch.stack(mp.idx[T::2]).reshape(H, M)
            min_edge = min(min_edge, mp.min_edge)
        if with_map:
            top2 = tensors['map_rec'].detach().double().topk(2, dim=2).values
            min_gap = min(min_gap, float((top2[:, :, 0] - top2[:, :, 1]).min()))
        if min_edge <= MIN_EDGE or (with_map and min_gap <= MIN_GAP):
            return None, min_edge, min_gap
        for opt in optimizers:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        grad_metrics = model.grad_clip(rconf.grad_clip, rconf.grad_clip_ac)
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        for opt in optimizers:
            opt.step()
        pre = f's{step}_'
        for k, v in {**raw, **extra}.items():
            out[pre + 'in_' + k] = v
        for k in ('u_post', 'u_act', 'u_prior'):
            out[pre + 'in_' + k] = noise[k].numpy()
        out[pre + 'losses'] = np.array([float(l) for l in losses], dtype=np.float64)
        for k, v in {**metrics, **grad_metrics}.items():
            out[pre + 'metric_' + k] = np.array(float(v), dtype=np.float64)
        probe_tensors = [k for k in tensors if 'goal' in k] + (['map_rec', 'loss_map', 'acc_map'] if with_map else [])
        for k in probe_tensors:
            out[pre + 'tensor_' + k] = tensors[k].detach().numpy()
        out[pre + 'out_state_h'] = new_state[0].numpy()
        out[pre + 'idx_post'] = post_idx.numpy().astype(np.uint8)
        out[pre + 'idx_act'] = act_idx.numpy().astype(np.uint8)
        probe = [k for k in grads if k.startswith('probe_model.')]
        out[pre + 'probe_grad_names'] = np.array(probe)
        out[pre + 'probe_grad_norms'] = np.array([float(grads[k].double().norm()) for k in probe])
        weights = [k for k in probe if grads[k].dim() == 2]
        for k in (weights[0], weights[-1]):          # the first and the last probe weight
            out[pre + 'grad_' + k] = grads[k].numpy()
        post = dict(model.state_dict())
        out[pre + 'param_sums'] = np.array([float(v.double().sum()) for v in post.values()])
        out[pre + 'param_abs_sums'] = np.array([float(v.double().abs().sum()) for v in post.values()])
        state = new_state
        print(f'  step {step}: losses', out[pre + 'losses'], {k: round(float(v), 6) for k, v in metrics.items() if 'goal' in k},
              'grad_norm_probe', float(grad_metrics['grad_norm_probe']))
        ages = {k: float(v) for k, v in metrics.items() if k.startswith('mse_goal_age')}
        assert len(ages) == 6 and np.isnan(ages['mse_goal_age1000']) and sum(np.isnan(v) for v in ages.values()) == 1, ages
    out['min_edge_distance'] = np.array(min_edge)
    if with_map:
        out['min_map_rec_gap'] = np.array(min_gap)
    return out, min_edge, min_gap


def run(name, overrides, extra_conf, steps):
    torch.set_num_threads(8)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import torch.distributions as D
    D.Distribution.set_default_validate_args(False)   # train.py:30
    rconf = reference_conf(['defaults', 'atari'], overrides)
    oconf = O.make_conf(**{k: getattr(rconf, k) for k in O.DEFAULTS})
    seed = 777
    while True:
        print(f'[{name}] noise seed {seed}')
        out, min_edge, min_gap = _attempt(rconf, oconf, extra_conf, steps, seed)
        if out is not None:
            break
        print(f'[{name}] edge distance {min_edge:.2e} (need > {MIN_EDGE}), map_rec top-two gap {min_gap:.2e} (need > {MIN_GAP}): next seed')
        seed += 1000
    assert float(out['min_edge_distance']) > MIN_EDGE
    path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, f'{os.path.getsize(path) / 1024:.0f} KiB', 'min edge distance', float(out['min_edge_distance']))


if __name__ == '__main__':
    which = sys.argv[1:] or ['tiny_goals_probe', 'tiny_goals_probe_iwae', 'tiny_map_goals_probe']
    if 'tiny_goals_probe' in which:
        run('tiny_goals_probe', tiny_overrides(**GOALS), GOALS, steps=2)
    if 'tiny_goals_probe_iwae' in which:
        run('tiny_goals_probe_iwae', tiny_overrides(iwae_samples=2, **GOALS), GOALS, steps=1)
    if 'tiny_map_goals_probe' in which:
        run('tiny_map_goals_probe', tiny_overrides(**MAP_GOALS), MAP_GOALS, steps=1)
