"""Golden vectors for the observation inputs beyond the image: reward_input (the reward / terminal planes of encoders.py:52-59)
and vecobs_size > 0 (the vector observation's MLP encoder and Normal decoder, encoders.py:33-36,64-68, decoders.py:45-48,66-71).

    python scripts/gen_obs_golden.py            # writes tests/golden/tiny_reward_input.npz, tiny_vecobs.npz and tiny_obs_*.npz

Runs the REAL reference on CPU (imported in place, as oracle/gen_golden.py does; only where the reference checkout exists) at
the tiny shape of `oracle.tiny_conf()`: two consecutive trainer iterations with carried state (train.py:165-198), data-only
fixtures.  Weights are never stored: both sides compute them with tests/closed_form_params.py from the ordered
{name: shape} map of the reference's state_dict, which the fixture records (`param_names`, `param_shapes`), so the tests can
check key order and shapes without the reference.

The tests demand EQUAL sampled indices.  To make that a fair demand, every categorical draw records the distance of its uniform
to the nearest edge of the reference's CDF; the noise seed is advanced until the minimum over the whole fixture is above 1e-5
(about a hundred times the 1.3e-7 at which fp32 summation order has been seen to flip a draw in the full-size parity tests), and
the achieved minimum is stored (`min_edge_distance`).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import dreamer_oracle as O                                   # noqa: E402
from oracle.gen_golden import REF, MultinomialPatch, reference_conf      # noqa: E402
import closed_form_params as CFP                                         # noqa: E402

MIN_EDGE = 1e-5


class MarginPatch(MultinomialPatch):
    """MultinomialPatch that also records how far every uniform is from the nearest inner edge of the normalised CDF."""

    def __init__(self):
        super().__init__()
        self.min_edge = float('inf')

    def __call__(self, probs, num_samples, replacement=False, **kw):
        u = self.queue[0].reshape(-1).double()
        cdf = torch.cumsum(probs.detach().double(), -1)
        edges = cdf[:, :-1] / cdf[:, -1:]                      # the last edge (= 1) is never crossed: the index is clamped
        self.min_edge = min(self.min_edge, float((edges - u.unsqueeze(-1)).abs().min()))
        return super().__call__(probs, num_samples, replacement, **kw)


def tiny_overrides(**kw):
    t = O.tiny_conf()
    base = dict(deter_dim=t.deter_dim, hidden_dim=t.hidden_dim, stoch_dim=t.stoch_dim, stoch_discrete=t.stoch_discrete,
                cnn_depth=t.cnn_depth, action_dim=t.action_dim, batch_length=t.batch_length, batch_size=t.batch_size,
                imag_horizon=t.imag_horizon)
    base.update(kw)
    return base


def make_batch(oconf, step, vecobs_size=0):
    """oracle.synthetic_batch, with terminal frames: its 0.5 % terminal rate leaves a 15-frame batch without one, and the
    terminal plane would then never carry a value.  vecobs_size = V: plus a (T,B,V) float32 `vecobs` from a stream of its own."""
    raw = O.synthetic_batch(oconf, seed=1234 + step, first=(step == 0))
    raw['terminal'][2 + step, 1] = 1.0
    raw['terminal'][4, 2 - step] = 1.0
    if vecobs_size:
        raw['vecobs'] = np.random.RandomState(4321 + step).randn(oconf.batch_length, oconf.batch_size, vecobs_size).astype(np.float32)
    return raw


def to_obs(raw, oconf):
    obs = O.preprocess(raw, oconf)
    if 'vecobs' in raw:
        obs['vecobs'] = torch.from_numpy(raw['vecobs'])
    return obs


def _attempt(rconf, oconf, steps, full_grads, noise_seed):
    from pydreamer.models import Dreamer          # the reference, imported in place
    torch.manual_seed(0)
    model = Dreamer(rconf)
    sd = model.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    optimizers = model.init_optimizers(rconf.adam_lr, rconf.adam_lr_actor, rconf.adam_lr_critic, rconf.adam_eps)
    T, B, S, H = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon
    I = rconf.iwae_samples
    M = T * B * I
    nd = max(len(s) for s in shapes.values())
    out = {'conf_json': np.array(repr(sorted(vars(oconf).items()))),
           'extra_conf_json': np.array(repr(sorted(dict(reward_input=bool(rconf.reward_input),
                                                         vecobs_size=int(rconf.vecobs_size)).items()))),
           'param_names': np.array(list(shapes.keys())),
           'param_shapes': np.array([list(s) + [-1] * (nd - len(s)) for s in shapes.values()], dtype=np.int64),
           'noise_seed': np.array(noise_seed)}
    state = model.init_state(B * I)
    min_edge = float('inf')
    for step in range(steps):
        raw = make_batch(oconf, step, rconf.vecobs_size)
        obs = to_obs(raw, oconf)
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
            lat_idx = torch.stack(mp.idx[T + 1::2]).reshape(H, M, S)
            min_edge = min(min_edge, mp.min_edge)
        if min_edge <= MIN_EDGE:
            return None, min_edge
        for opt in optimizers:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        grad_metrics = model.grad_clip(rconf.grad_clip, rconf.grad_clip_ac)
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        for opt in optimizers:
            opt.step()
        pre = f's{step}_'
        for k, v in raw.items():
            out[pre + 'in_' + k] = v
        for k in ('u_post', 'u_act', 'u_prior'):
            out[pre + 'in_' + k] = noise[k].numpy()
        out[pre + 'in_state_h'] = state[0].numpy()
        out[pre + 'in_state_z'] = state[1].numpy()
        out[pre + 'losses'] = np.array([float(l) for l in losses], dtype=np.float64)
        for k, v in {**metrics, **grad_metrics}.items():
            out[pre + 'metric_' + k] = np.array(float(v), dtype=np.float64)
        for k, v in tensors.items():
            if k == 'image_rec':
                out[pre + 'tensor_image_rec_sum'] = np.array(float(v.double().sum()))
                out[pre + 'tensor_image_rec_frames'] = v[:1, :1].numpy()
            else:
                out[pre + 'tensor_' + k] = v.detach().numpy()
        out[pre + 'out_state_h'] = new_state[0].numpy()
        out[pre + 'out_state_z'] = new_state[1].numpy()
        out[pre + 'idx_post'] = post_idx.numpy().astype(np.uint8)
        out[pre + 'idx_act'] = act_idx.numpy().astype(np.uint8)
        out[pre + 'idx_lat'] = lat_idx.numpy().astype(np.uint8)
        out[pre + 'grad_norms'] = np.array([float(g.double().norm()) for g in grads.values()])
        out[pre + 'grad_names'] = np.array(list(grads.keys()))
        for k in full_grads:
            out[pre + 'grad_' + k] = grads[k].numpy()
        post = dict(model.state_dict())
        out[pre + 'param_sums'] = np.array([float(v.double().sum()) for v in post.values()])
        out[pre + 'param_abs_sums'] = np.array([float(v.double().abs().sum()) for v in post.values()])
        state = new_state
        print(f'  step {step}: losses', out[pre + 'losses'], 'grad_norm', float(grad_metrics['grad_norm']))
    out['min_edge_distance'] = np.array(min_edge)
    return out, min_edge


def run(name, overrides, steps=2, full_grads=(), grads_file=False):
    """grads_file: the full gradients, of the first step only, go to a companion <name>_grads.npz (every file stays under 1 MiB)."""
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
        out, min_edge = _attempt(rconf, oconf, steps, full_grads, seed)
        if out is not None:
            break
        print(f'[{name}] a uniform lies {min_edge:.2e} from a CDF edge (<= {MIN_EDGE}): next seed')
        seed += 1000
    assert float(out['min_edge_distance']) > MIN_EDGE
    if grads_file:
        full = {k: out.pop(k) for k in list(out) if k[3:].startswith('grad_') and k[3:] not in ('grad_norms', 'grad_names')}
        full = {k: v for k, v in full.items() if k.startswith('s0_')}      # of the first step: 0.7 MB of fp32 per step
        path = os.path.join(ROOT, 'tests', 'golden', f'{name}_grads.npz')
        np.savez_compressed(path, **full)
        print('wrote', path, f'{os.path.getsize(path) / 1024:.0f} KiB')
    path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, f'{os.path.getsize(path) / 1024:.0f} KiB', 'min edge distance', float(out['min_edge_distance']))


def _reference_model(overrides):
    torch.set_num_threads(8)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pydreamer.models import Dreamer
    import torch.distributions as D
    D.Distribution.set_default_validate_args(False)
    rconf = reference_conf(['defaults', 'atari'], overrides)
    oconf = O.make_conf(**{k: getattr(rconf, k) for k in O.DEFAULTS})
    torch.manual_seed(0)
    model = Dreamer(rconf)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    nd = max(len(s) for s in shapes.values())
    out = {'conf_json': np.array(repr(sorted(vars(oconf).items()))),
           'extra_conf_json': np.array(repr(sorted(dict(reward_input=bool(rconf.reward_input),
                                                         vecobs_size=int(rconf.vecobs_size)).items()))),
           'param_names': np.array(list(shapes.keys())),
           'param_shapes': np.array([list(s) + [-1] * (nd - len(s)) for s in shapes.values()], dtype=np.int64)}
    return rconf, oconf, model, out


def _save(name, out):
    path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, f'{os.path.getsize(path) / 1024:.0f} KiB', 'min edge distance', float(out['min_edge_distance']))


def run_inference(name, overrides):
    """Dreamer.inference (dreamer.py:92-111) in the call shape of oracle/gen_golden.py run_inference - one step, (1,B,...) obs, the
    posterior draw pinned - with the reward and terminal the encoder now reads (non-zero, one terminal frame)."""
    seed = 31
    while True:
        rconf, oconf, model, out = _reference_model(overrides)
        B, S, C, A = 3, rconf.stoch_dim, rconf.stoch_discrete, rconf.action_dim
        g = torch.Generator().manual_seed(seed)
        image_u8 = torch.randint(0, 256, (1, B, 64, 64, 3), generator=g, dtype=torch.uint8)
        image = (image_u8.float() / 255.0 - 0.5).permute(0, 1, 4, 2, 3).contiguous()
        action = torch.nn.functional.one_hot(torch.randint(0, A, (1, B), generator=g), A).float()
        reset = torch.tensor([[True, False, False]])
        h = torch.tanh(torch.randn(B, rconf.deter_dim, generator=g))
        z = torch.nn.functional.one_hot(torch.randint(0, C, (B, S), generator=g), C).float().reshape(B, S * C)
        u = torch.rand(1, B, S, generator=g)
        reward = torch.tanh(torch.randn(1, B, generator=g))
        terminal = torch.tensor([[0.0, 1.0, 0.0]])
        obs = dict(image=image, action=action, reset=reset, reward=reward, terminal=terminal)
        vecobs = torch.randn(1, B, rconf.vecobs_size, generator=g) if rconf.vecobs_size else None
        if vecobs is not None:
            obs['vecobs'] = vecobs
        with MarginPatch() as mp, torch.no_grad():
            mp.queue = [u[0]]
            dist, (h1, z1), metrics = model.inference(obs, (h, z))
            assert not mp.queue
        if mp.min_edge > MIN_EDGE:
            break
        seed += 1000
    out.update(in_image_u8=image_u8.numpy(), in_action=action.numpy(), in_reset=reset.numpy(), in_reward=reward.numpy(),
               in_terminal=terminal.numpy(), in_h=h.numpy(), in_z=z.numpy(), in_u=u.numpy(), action_probs=dist.probs.numpy(),
               out_h=h1.numpy(), out_z=z1.numpy(), policy_value=np.array(float(metrics['policy_value'])),
               min_edge_distance=np.array(mp.min_edge))
    if vecobs is not None:
        out['in_vecobs'] = vecobs.numpy()
    _save(name, out)


def run_amp(name, overrides):
    """The reference's mixed-precision forward (train.py:166), produced the way oracle/gen_golden.py run_amp produces tiny_amp:
    one no_grad step in fp32 and one under torch.autocast('cpu', bfloat16); losses, metrics, posterior indices."""
    seed = 777
    while True:
        out, edge = _amp_attempt(name, overrides, seed)
        # The test teacher-forces the bf16 pass's posterior indices and holds loss_model to BOTH passes' values: that is a fair
        # demand only when the two passes walked the same trajectory (as they do in tiny_amp.npz: 0 of 120 indices differ;
        # autocast moves the CDFs by ~1e-3, so a seed can flip several draws between the passes)
        same = np.array_equal(out['fp32_idx_post'], out['bf16_idx_post'])
        if edge > MIN_EDGE and same:
            break
        print(f'[{name}] seed {seed}: edge distance {edge:.2e}, fp32 and bf16 passes drew the same posterior indices: {same}: next seed')
        seed += 1000
    out['noise_seed'] = np.array(seed)
    assert float(out['min_edge_distance']) > MIN_EDGE
    _save(name, out)


def _amp_attempt(name, overrides, seed):
    rconf, oconf, model, out = _reference_model(overrides)
    T, B, S, H = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon
    raw = make_batch(oconf, 0, rconf.vecobs_size)
    obs = to_obs(raw, oconf)
    noise = O.make_noise(oconf, seed=seed)
    for k, v in raw.items():
        out['in_' + k] = v
    for k in ('u_post', 'u_act', 'u_prior'):
        out['in_' + k] = noise[k].numpy()
    edge = float('inf')
    for tag, amp in (('fp32', False), ('bf16', True)):
        with MarginPatch() as mp:
            mp.queue = [noise['u_post'][t] for t in range(T)]
            for i in range(H):
                mp.queue += [noise['u_act'][i], noise['u_prior'][i]]
            with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16, enabled=amp):
                losses, _, metrics, _, _ = model.training_step(obs, model.init_state(B))
            post_idx = torch.stack(mp.idx[:T]).reshape(T, B, S)
            if not amp:
                edge = mp.min_edge
        out[tag + '_losses'] = np.array([float(l) for l in losses], dtype=np.float64)
        for k, v in metrics.items():
            out[tag + '_metric_' + k] = np.array(float(v), dtype=np.float64)
        out[tag + '_idx_post'] = post_idx.numpy().astype(np.uint8)
        print(f'[{name}] {tag}: losses', out[tag + '_losses'])
    out['min_edge_distance'] = np.array(edge)        # of the fp32 pass (the test teacher-forces the bf16 pass's indices)
    return out, edge


def run_eval(name, overrides, do_open_loop=False):
    """The logging variants of training_step (train.py:353-359,380-385), as oracle/gen_golden.py run_eval stores them: one forward
    under no_grad with do_image_pred and do_dream_tensors (and do_open_loop); inputs, the extra uniforms, every extra output."""
    seed = 999
    while True:
        rconf, oconf, model, out = _reference_model(overrides)
        T, B, S, H = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon
        raw = make_batch(oconf, 0, rconf.vecobs_size)
        obs = to_obs(raw, oconf)
        noise = O.make_noise(oconf, seed=seed)
        with MarginPatch() as mp:
            mp.queue = [noise['u_post'][t] for t in range(T)] + [noise['u_pred'].reshape(-1, S)]
            for i in range(H):
                mp.queue += [noise['u_act'][i], noise['u_prior'][i]]
            for i in range(T - 1):
                mp.queue += [noise['u_act_log'][i], noise['u_prior_log'][i]]
            with torch.no_grad():
                losses, new_state, metrics, tensors, dream_tensors = model.training_step(
                    obs, model.init_state(B), do_image_pred=True, do_dream_tensors=True, do_open_loop=do_open_loop)
            assert not mp.queue
            pred_idx = mp.idx[T].reshape(T, B, S)
            tail = mp.idx[T + 1 + 2 * H:]
            log_act, log_lat = torch.stack(tail[0::2]), torch.stack(tail[1::2]).reshape(T - 1, B, S)
        if mp.min_edge > MIN_EDGE:
            break
        print(f'[{name}] a uniform lies {mp.min_edge:.2e} from a CDF edge: next seed')
        seed += 1000
    for k, v in raw.items():
        out['in_' + k] = v
    for k in ('u_post', 'u_act', 'u_prior', 'u_pred', 'u_act_log', 'u_prior_log'):
        out['in_' + k] = noise[k].numpy()
    out['losses'] = np.array([float(l) for l in losses], dtype=np.float64)
    for k, v in metrics.items():
        out['metric_' + k] = np.array(float(v), dtype=np.float64)
    for k, v in tensors.items():
        if k in ('image_rec', 'image_pred'):
            out['tensor_' + k + '_sum'] = np.array(float(v.double().sum()))
            out['tensor_' + k + '_frame'] = v[:1, :1].numpy()
        else:
            out['tensor_' + k] = v.detach().numpy()
    for k, v in dream_tensors.items():
        if k == 'image_pred':
            out['dream_image_pred_sum'] = np.array(float(v.double().sum()))
            out['dream_image_pred_frame'] = v[-1:, :1].numpy()
        else:
            out['dream_' + k] = v.detach().numpy()
    out.update(idx_post=torch.stack(mp.idx[:T]).reshape(T, B, S).numpy().astype(np.uint8), out_state_h=new_state[0].numpy(),
               idx_pred=pred_idx.numpy().astype(np.uint8), idx_log_act=log_act.numpy().astype(np.uint8),
               idx_log_lat=log_lat.numpy().astype(np.uint8), open_loop=np.array(bool(do_open_loop)),
               min_edge_distance=np.array(mp.min_edge))
    _save(name, out)


if __name__ == '__main__':
    ALL = ['tiny_reward_input', 'tiny_vecobs', 'tiny_obs_combo', 'tiny_obs_eval', 'tiny_obs_open_loop', 'tiny_obs_inference',
           'tiny_obs_amp']
    which = sys.argv[1:] or ALL
    both = dict(reward_input=True, vecobs_size=27)
    if 'tiny_reward_input' in which:
        # the full dW of encoder layer 0: its two plane slices are what the fold produces
        run('tiny_reward_input', tiny_overrides(reward_input=True), steps=2,
            full_grads=('wm.encoder.encoder_image.model.0.weight', 'wm.encoder.encoder_image.model.0.bias',
                        'wm.core.cell.post_mlp_e.weight', 'wm.core.cell.a_mlp.weight', 'ac.actor.model.12.weight'))
    if 'tiny_vecobs' in which:
        # the first and the last Linear of both vecobs MLPs
        run('tiny_vecobs', tiny_overrides(vecobs_size=27), steps=2,
            full_grads=('wm.encoder.encoder_vecobs.model.0.weight', 'wm.encoder.encoder_vecobs.model.6.weight',
                        'wm.decoder.vecobs.model.model.0.weight', 'wm.decoder.vecobs.model.model.12.weight'), grads_file=True)
    if 'tiny_obs_combo' in which:
        run('tiny_obs_combo', tiny_overrides(iwae_samples=2, **both), steps=2,
            full_grads=('wm.encoder.encoder_image.model.0.weight', 'wm.encoder.encoder_vecobs.model.0.weight',
                        'wm.decoder.vecobs.model.model.12.weight'))
    if 'tiny_obs_eval' in which:
        run_eval('tiny_obs_eval', tiny_overrides(**both))
    if 'tiny_obs_open_loop' in which:
        run_eval('tiny_obs_open_loop', tiny_overrides(**both), do_open_loop=True)
    if 'tiny_obs_inference' in which:
        run_inference('tiny_obs_inference', tiny_overrides(**both))
    if 'tiny_obs_amp' in which:
        run_amp('tiny_obs_amp', tiny_overrides(**both))
