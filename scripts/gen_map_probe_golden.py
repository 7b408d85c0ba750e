"""Golden vectors for the map probe: probe_model='map' (probes.py:32-86, the dense CatImageDecoder of decoders.py:183-254).

    python scripts/gen_map_probe_golden.py      # writes tests/golden/tiny_map_probe.npz and tiny_map_probe_iwae.npz

Runs the REAL reference on CPU, imported in place as scripts/gen_obs_golden.py does (only where the reference checkout exists),
at the tiny shape of `oracle.tiny_conf()` with a 6-class 5x5 map and a 2 x 128 probe MLP: trainer iterations with carried state
(train.py:165-198), data-only fixtures.  Weights are never stored: both sides compute them with tests/closed_form_params.py from
the ordered {name: shape} map of the reference's state_dict, which the fixture records.

Two demands of the tests are made fair here.  Sampled indices must be EQUAL: the noise seed is advanced until every uniform lies
more than 1e-5 from the nearest edge of the reference's CDF (the rule of gen_obs_golden.py).  The per-frame accuracy must be
EQUAL: the seed is also advanced until the two largest values of `map_rec` differ by more than 1e-4 in every cell of every
frame, a hundred times the fp32 rounding of a log-probability of magnitude ten, so no argmax of the fixture hangs on rounding.
Both achieved minima are stored.
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

MIN_GAP = 1e-4
MAP = dict(probe_model='map', map_size=5, map_channels=6, map_hidden_dim=128, map_hidden_layers=2)
FIRST, LAST = 'probe_model.decoder.model.0.weight', 'probe_model.decoder.model.6.weight'


def map_inputs(rconf, step):
    """A random class map (stored as classes, fed one-hot), map_coord ~ N(0,1), a 0/1 seen mask with one frame all zero."""
    T, B, C, S = rconf.batch_length, rconf.batch_size, rconf.map_channels, rconf.map_size
    rs = np.random.RandomState(9876 + step)
    classes = rs.randint(0, C, (T, B, S, S)).astype(np.uint8)
    coord = rs.randn(T, B, 4).astype(np.float32)
    seen = (rs.rand(T, B, S, S) < 0.6).astype(np.int64)
    seen[1 + step, 2 - step] = 0
    seen[0, 0] = 1
    return dict(map_classes=classes, map_coord=coord, map_seen_mask=seen)


def map_obs(extra, C):
    onehot = torch.nn.functional.one_hot(torch.from_numpy(extra['map_classes'].astype(np.int64)), C).float()
    return dict(map=onehot.permute(0, 1, 4, 2, 3).contiguous(), map_coord=torch.from_numpy(extra['map_coord']),
                map_seen_mask=torch.from_numpy(extra['map_seen_mask']))


def _attempt(rconf, oconf, steps, noise_seed):
    from pydreamer.models import Dreamer          # the reference, imported in place
    torch.manual_seed(0)
    model = Dreamer(rconf)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    optimizers = model.init_optimizers(rconf.adam_lr, rconf.adam_lr_actor, rconf.adam_lr_critic, rconf.adam_eps)
    T, B, S, H, I = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon, rconf.iwae_samples
    M = T * B * I
    nd = max(len(s) for s in shapes.values())
    out = {'conf_json': np.array(repr(sorted(vars(oconf).items()))), 'extra_conf_json': np.array(repr(sorted(MAP.items()))),
           'param_names': np.array(list(shapes.keys())),
           'param_shapes': np.array([list(s) + [-1] * (nd - len(s)) for s in shapes.values()], dtype=np.int64),
           'noise_seed': np.array(noise_seed)}
    state = model.init_state(B * I)
    min_edge, min_gap = float('inf'), float('inf')
    for step in range(steps):
        raw = make_batch(oconf, step)
        extra = map_inputs(rconf, step)
        obs = dict(to_obs(raw, oconf), **map_obs(extra, rconf.map_channels))
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
        top2 = tensors['map_rec'].detach().double().topk(2, dim=2).values
        min_gap = min(min_gap, float((top2[:, :, 0] - top2[:, :, 1]).min()))
        if min_edge <= MIN_EDGE or min_gap <= MIN_GAP:
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
        for k in ('map_rec', 'loss_map', 'acc_map'):
            out[pre + 'tensor_' + k] = tensors[k].detach().numpy()
        out[pre + 'out_state_h'] = new_state[0].numpy()
        out[pre + 'idx_post'] = post_idx.numpy().astype(np.uint8)
        out[pre + 'idx_act'] = act_idx.numpy().astype(np.uint8)
        probe = [k for k in grads if k.startswith('probe_model.')]
        out[pre + 'probe_grad_names'] = np.array(probe)
        out[pre + 'probe_grad_norms'] = np.array([float(grads[k].double().norm()) for k in probe])
        for k in (FIRST, LAST):
            out[pre + 'grad_' + k] = grads[k].numpy()
        post = dict(model.state_dict())
        out[pre + 'param_sums'] = np.array([float(v.double().sum()) for v in post.values()])
        out[pre + 'param_abs_sums'] = np.array([float(v.double().abs().sum()) for v in post.values()])
        state = new_state
        print(f'  step {step}: losses', out[pre + 'losses'], 'acc_map', float(metrics['acc_map']), 'acc_map_seen',
              float(metrics['acc_map_seen']), 'grad_norm_probe', float(grad_metrics['grad_norm_probe']))
    out['min_edge_distance'] = np.array(min_edge)
    out['min_map_rec_gap'] = np.array(min_gap)
    return out, min_edge, min_gap


def run(name, overrides, steps):
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
        out, min_edge, min_gap = _attempt(rconf, oconf, steps, seed)
        if out is not None:
            break
        print(f'[{name}] edge distance {min_edge:.2e} (need > {MIN_EDGE}), map_rec top-two gap {min_gap:.2e} (need > {MIN_GAP}): next seed')
        seed += 1000
    assert float(out['min_edge_distance']) > MIN_EDGE and float(out['min_map_rec_gap']) > MIN_GAP
    path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, f'{os.path.getsize(path) / 1024:.0f} KiB', 'min edge distance', float(out['min_edge_distance']),
          'min map_rec gap', float(out['min_map_rec_gap']))


if __name__ == '__main__':
    which = sys.argv[1:] or ['tiny_map_probe', 'tiny_map_probe_iwae']
    if 'tiny_map_probe' in which:
        run('tiny_map_probe', tiny_overrides(**MAP), steps=2)
    if 'tiny_map_probe_iwae' in which:
        run('tiny_map_probe_iwae', tiny_overrides(iwae_samples=2, **MAP), steps=1)
