"""Golden vectors for the GRU probe baseline on the dense encoder: WorldModelProbe(model='gru_probe') (baselines.py:19-111 with
GRUEncoderOnly, baselines.py:314-357) under the `minigrid` section, where MultiEncoder builds a DenseEncoder (encoders.py:23-27,
99-125) on the one-hot class image.

    python scripts/gen_gru_probe_minigrid_golden.py      # writes tests/golden/tiny_gru_probe_minigrid.npz and ..._plain.npz

Runs the REAL reference on CPU, imported in place as scripts/gen_gru_probe_golden.py and scripts/gen_minigrid_golden.py do (only
where the reference checkout exists), with sections defaults + minigrid at the tiny dimensions of `oracle.tiny_conf()`,
gen_minigrid_golden.GRID (7 x 7 cells, 4 classes, 7 actions) and the small map of gen_map_probe_golden.MAP: two trainer iterations
with carried state (train.py:165-198: zero_grad, backward, grad_clip, step), data-only fixtures.  Weights are never stored: both
sides compute them with tests/closed_form_params.py from the ordered {name: shape} map of the reference's state_dict, which the
fixture records.  Class images are stored as uint8 (T,B,S,S) and fed one-hot.

  tiny_gru_probe_minigrid        probe_model='map', reward_input=True: encoder in_dim 7 * 7 * (4 + 2) = 294, three hidden layers
  tiny_gru_probe_minigrid_plain  reward_input=False, layer_norm=False, image_encoder_layers=1: in_dim 196, no LayerNorm anywhere

The model draws no random numbers.  The per-frame map accuracy must be EQUAL: the two largest values of `map_rec` must differ by
more than MIN_GAP in every cell of every frame (the rule of gen_map_probe_golden.py); as there is no noise seed to advance, the
seed of the class IMAGE is advanced until the rule holds (`image_seed`, 0 = gen_minigrid_golden.grid_batch's own images), and
the achieved minimum is stored.  `reset` keeps its mid-sequence reset, which the reference does not read
(baselines.py:339).

Stored per step: loss, metrics, every tensor, out_state, every gradient norm, the parameter sums after the optimizer step, and the
full gradients of the GRU's two matrices, the squeeze, one probe weight and - at the FIRST step only, so that a fixture stays no
larger than tiny_gru_probe_*.npz (400 x 294 floats a step) - the encoder's first Linear.  Every iteration is also run with the
model and every floating input in float64; per class of compared quantity the fixture stores `fp64_dev_<class>`: the largest
deviation of the fp32 reference from that run, over BOTH steps, as a FRACTION OF THE BAR tests/test_gpu_gru_probe_minigrid.py
applies to the class (gen_minigrid_golden.BARS; 1.0 = the reference alone would sit on the bar).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import closed_form_params as CFP                                         # noqa: E402
from gen_gru_probe_golden import action_next                             # noqa: E402
from gen_map_probe_golden import MAP, MIN_GAP, map_inputs, map_obs       # noqa: E402
from gen_minigrid_golden import BARS, KeepDouble, _header, _setup, bar_fraction, grid_batch, grid_obs      # noqa: E402

BASE = dict(MAP, model='gru_probe', probe_gradients=True)
MAIN = dict(BASE, reward_input=True)
PLAIN = dict(BASE, reward_input=False, layer_norm=False, image_encoder_layers=1)
ENC_FIRST = 'wm.encoder.encoder_image.model.1.weight'
FULL_GRADS = ['wm.rnn.weight_hh_l0', 'wm.rnn.weight_ih_l0', 'wm.squeeze.weight', ENC_FIRST]
MAX_BYTES = 692022          # the smaller of tests/golden/tiny_gru_probe_map_goals.npz and tiny_gru_probe_goals.npz


def _batch(oconf, step, image_seed):
    """gen_minigrid_golden.grid_batch; image_seed > 0 redraws the class image from a stream of that seed."""
    raw = grid_batch(oconf, step)
    if image_seed:
        shape = raw['image_classes'].shape
        raw['image_classes'] = np.random.RandomState(2468 + step + image_seed).randint(0, oconf.image_channels, shape).astype(np.uint8)
    return raw


def _min_gap(records):
    gaps = [r['tensors']['map_rec'].double().topk(2, dim=2).values for r in records]
    return min(float((g[:, :, 0] - g[:, :, 1]).min()) for g in gaps)


def _iterate(rconf, oconf, steps, dtype, image_seed=0):
    """The trainer iterations in `dtype`; returns (records per step, ordered shapes)."""
    from pydreamer.models.baselines import WorldModelProbe          # the reference, imported in place
    torch.manual_seed(0)
    model = WorldModelProbe(rconf)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    model = model.to(dtype)
    optimizers = model.init_optimizers(rconf.adam_lr, rconf.adam_lr_actor, rconf.adam_lr_critic, rconf.adam_eps)
    assert len(optimizers) == 1
    state = model.init_state(rconf.batch_size).to(dtype)
    records = []
    for step in range(steps):
        raw = _batch(oconf, step, image_seed)
        assert raw['reset'][1:].any(), 'the batch must hold a mid-sequence reset'
        extra = dict(map_inputs(rconf, step), action_next=action_next(raw, rconf.action_dim))
        obs = dict(grid_obs(raw, oconf, dtype), action_next=torch.from_numpy(extra['action_next']), **map_obs(extra, rconf.map_channels))
        obs = {k: v.to(dtype) if v.is_floating_point() else v for k, v in obs.items()}
        with KeepDouble(dtype == torch.float64):
            losses, new_state, metrics, tensors, _ = model.training_step(obs, state)
            assert len(losses) == 1 and losses[0].dtype == dtype
            for opt in optimizers:
                opt.zero_grad()
            for loss in losses:
                loss.backward()
        grad_metrics = model.grad_clip(rconf.grad_clip, rconf.grad_clip_ac)
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters()}
        for opt in optimizers:
            opt.step()
        post = dict(model.state_dict())
        probe_w = next(k for k in grads if k.startswith('probe_model.') and grads[k].dim() == 2)
        records.append(dict(
            inputs={**raw, **extra}, loss=float(losses[0].detach()), metrics={k: float(v) for k, v in {**metrics, **grad_metrics}.items()},
            tensors={k: v.detach().clone() for k, v in tensors.items()}, out_state=new_state.detach().clone(),
            grad_names=list(grads), grad_norms=np.array([float(g.double().norm()) for g in grads.values()]),
            grads={k: grads[k] for k in FULL_GRADS + [probe_w]},
            param_sums=np.array([float(v.double().sum()) for v in post.values()]),
            param_abs_sums=np.array([float(v.double().abs().sum()) for v in post.values()])))
        state = new_state
    return records, shapes


def run(name, overrides, steps=2):
    rconf, oconf = _setup(overrides)
    assert rconf.image_encoder == 'dense' and rconf.image_categorical and rconf.model == 'gru_probe' and rconf.probe_gradients
    image_seed = 0
    while True:
        rec32, shapes = _iterate(rconf, oconf, steps, torch.float32, image_seed)
        min_gap = _min_gap(rec32)
        if min_gap > MIN_GAP:
            break
        print(f'[{name}] image seed {image_seed}: map_rec top-two gap {min_gap:.2e} (need > {MIN_GAP}): next seed')
        image_seed += 1000
    rec64, _ = _iterate(rconf, oconf, steps, torch.float64, image_seed)
    want_in = rconf.image_size ** 2 * (rconf.image_channels + (2 if rconf.reward_input else 0))
    assert shapes[ENC_FIRST] == (400, want_in), shapes[ENC_FIRST]
    out = dict(_header(oconf, overrides, shapes), image_seed=np.array(image_seed))
    dev = {k: 0.0 for k in BARS}
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
            if k != ENC_FIRST or step == 0:
                out[pre + 'grad_' + k] = v.numpy()
        out[pre + 'param_sums'], out[pre + 'param_abs_sums'] = a['param_sums'], a['param_abs_sums']
        # the fp32 reference against the same iterations in float64, as a fraction of each bar
        dev['losses'] = max(dev['losses'], bar_fraction('losses', a['loss'], b['loss']))
        for k, v in a['metrics'].items():
            assert np.isnan(v) == np.isnan(b['metrics'][k]), k
            dev['metrics'] = max(dev['metrics'], bar_fraction('metrics', v, b['metrics'][k]))
        for k, v in a['tensors'].items():
            if k != 'acc_map':
                dev['tensors'] = max(dev['tensors'], bar_fraction('tensors', v.numpy(), b['tensors'][k].numpy()))
        dev['tensors'] = max(dev['tensors'], bar_fraction('tensors', a['out_state'].numpy(), b['out_state'].numpy()))
        assert torch.equal(a['tensors']['acc_map'].double(), b['tensors']['acc_map'].double()), 'acc_map differs between fp32 and fp64'
        dev['grad_norms'] = max(dev['grad_norms'], bar_fraction('grad_norms', a['grad_norms'], b['grad_norms']))
        for k, v in a['grads'].items():
            dev['full_grads'] = max(dev['full_grads'], bar_fraction('full_grads', v.numpy(), b['grads'][k].numpy()))
        dev['param_abs_sums'] = max(dev['param_abs_sums'], bar_fraction('param_abs_sums', a['param_abs_sums'], b['param_abs_sums']))
        print(f'  step {step}: loss {a["loss"]:.8g} (fp64 {b["loss"]:.8g}) grad_norm {a["metrics"]["grad_norm"]:.6g}',
              {k: round(v, 6) for k, v in a['metrics'].items() if k.startswith(('loss_', 'acc_'))})
        assert min(a['grad_norms']) > 0, 'a gradient is zero'
    for k, v in dev.items():
        out['fp64_dev_' + k] = np.array(v)
    print(f'[{name}] fp32 reference against float64, fraction of each bar:', {k: f'{v:.2e}' for k, v in dev.items()})
    assert min_gap > MIN_GAP, f'map_rec top-two gap {min_gap:.2e} (need > {MIN_GAP})'
    out['min_map_rec_gap'] = np.array(min_gap)
    print(f'[{name}] map_rec top-two gap {min_gap:.2e}')
    path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote', path, f'{size / 1024:.0f} KiB')
    assert size <= MAX_BYTES, (size, MAX_BYTES)


if __name__ == '__main__':
    which = sys.argv[1:] or ['tiny_gru_probe_minigrid', 'tiny_gru_probe_minigrid_plain']
    if 'tiny_gru_probe_minigrid' in which:
        run('tiny_gru_probe_minigrid', MAIN)
    if 'tiny_gru_probe_minigrid_plain' in which:
        run('tiny_gru_probe_minigrid_plain', PLAIN)
