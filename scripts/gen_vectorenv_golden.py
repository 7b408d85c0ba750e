"""Golden vectors for image-less world models - the `vectorenv` section (defaults.yaml:236-242): image_key, image_encoder and
image_decoder all empty, the vector observation the only input (encoders.py:28-40,64-69, decoders.py:29-30,59-64).

    python scripts/gen_vectorenv_golden.py            # writes tests/golden/tiny_vectorenv*.npz and vectorenv_preprocess.npz

Runs the REAL reference on CPU (imported in place, only where the reference checkout exists) with sections defaults + vectorenv
at tiny dims.  Data-only fixtures in the manner of scripts/gen_obs_golden.py: weights are never stored - both sides compute them
with tests/closed_form_params.py from the recorded `param_names` / `param_shapes` - inputs and draws are, and the noise seed is
advanced until no categorical draw sits within 1e-5 of an edge of the reference's CDF (`min_edge_distance`; infinite for a fixture
that draws from no categorical: Gaussian latents with a continuous actor).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import dreamer_oracle as O                                   # noqa: E402
from oracle.gen_golden import REF, reference_conf                        # noqa: E402
from gen_obs_golden import MIN_EDGE, MarginPatch                         # noqa: E402
import closed_form_params as CFP                                         # noqa: E402

SECTIONS = ['defaults', 'vectorenv']
TINY = dict(deter_dim=64, hidden_dim=64, stoch_dim=8, stoch_discrete=8, batch_length=5, batch_size=3, imag_horizon=4)
EXTRA_KEYS = ('vecobs_size', 'reward_input', 'image_key', 'image_encoder', 'image_decoder')


def make_batch(oconf, step, V):
    """oracle.synthetic_batch without the frames (drawn from streams of their own, so nothing 64 x 64 is generated): integer
    actions, tanh-clipped rewards, two terminal frames, a forced first reset and a mid-sequence one, a (T,B,V) float32 vecobs."""
    T, B, A = oconf.batch_length, oconf.batch_size, oconf.action_dim
    rs = np.random.RandomState(1234 + step)
    raw = dict(action_idx=rs.randint(0, A, (T, B)).astype(np.int64), reward=np.tanh(rs.randn(T, B)).astype(np.float32),
               terminal=np.zeros((T, B), np.float32), reset=np.zeros((T, B), bool))
    raw['terminal'][2 + step, 1] = 1.0
    raw['terminal'][4, 2 - step] = 1.0
    raw['reset'][0, 0] = step == 0
    raw['reset'][T // 2, B - 1] = True
    raw['vecobs'] = np.random.RandomState(4321 + step).randn(T, B, V).astype(np.float32)
    return raw


def to_obs(raw, oconf):
    """preprocessing.py with image_key empty: one-hot float actions, everything else as it is; no `image`."""
    action = torch.nn.functional.one_hot(torch.from_numpy(raw['action_idx']), oconf.action_dim).float()
    return dict(action=action, reward=torch.from_numpy(raw['reward']), terminal=torch.from_numpy(raw['terminal']),
                reset=torch.from_numpy(raw['reset']), vecobs=torch.from_numpy(raw['vecobs']))


def _reference_model(overrides):
    torch.set_num_threads(8)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pydreamer.models import Dreamer          # the reference, imported in place
    import torch.distributions as D
    D.Distribution.set_default_validate_args(False)   # train.py:30
    rconf = reference_conf(SECTIONS, {**TINY, **overrides})
    oconf = O.make_conf(**{k: getattr(rconf, k) for k in O.DEFAULTS})
    torch.manual_seed(0)
    model = Dreamer(rconf)
    assert model.wm.encoder.encoder_image is None and model.wm.decoder.image is None
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert not [k for k in shapes if 'image' in k]
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    nd = max(len(s) for s in shapes.values())
    out = {'conf_json': np.array(repr(sorted(vars(oconf).items()))),
           'extra_conf_json': np.array(repr(sorted({k: getattr(rconf, k) for k in EXTRA_KEYS}.items()))),
           'param_names': np.array(list(shapes.keys())),
           'param_shapes': np.array([list(s) + [-1] * (nd - len(s)) for s in shapes.values()], dtype=np.int64)}
    return rconf, oconf, model, out


def _queue_step(mp, rconf, noise):
    """The step's draws in the reference's call order: T posterior draws, then H x [actor, prior].  Categorical draws go through
    torch.multinomial, Gaussian latents through Normal.rsample, continuous actors through torch.normal (MultinomialPatch)."""
    T, H = rconf.batch_length, rconf.imag_horizon
    onehot, gaussian = rconf.actor_dist == 'onehot', not rconf.stoch_discrete
    lat = mp.std_queue if gaussian else mp.queue
    lat += [noise['u_post'][t] for t in range(T)]
    for i in range(H):
        if onehot:
            mp.queue.append(noise['u_act'][i])
        else:
            mp.eps_queue.append(noise['eps_act'][i])
        lat.append(noise['u_prior'][i])


def _indices(mp, rconf):
    T, B, S, H, I = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon, rconf.iwae_samples
    M = T * B * I
    onehot, gaussian = rconf.actor_dist == 'onehot', not rconf.stoch_discrete
    out = {}
    if not gaussian:
        out['idx_post'] = torch.stack(mp.idx[:T]).reshape(T, B * I, S)
        rest = mp.idx[T:]
        out['idx_lat'] = torch.stack(rest[1::2] if onehot else rest).reshape(H, M, S)
        if onehot:
            out['idx_act'] = torch.stack(rest[0::2]).reshape(H, M)
    elif onehot:
        out['idx_act'] = torch.stack(mp.idx).reshape(H, M)
    return {k: v.numpy().astype(np.uint8) for k, v in out.items()}


def _attempt(overrides, steps, full_grads, noise_seed):
    rconf, oconf, model, out = _reference_model(overrides)
    optimizers = model.init_optimizers(rconf.adam_lr, rconf.adam_lr_actor, rconf.adam_lr_critic, rconf.adam_eps)
    out['noise_seed'] = np.array(noise_seed)
    state = model.init_state(rconf.batch_size * rconf.iwae_samples)
    min_edge = float('inf')
    for step in range(steps):
        raw = make_batch(oconf, step, rconf.vecobs_size)
        obs = to_obs(raw, oconf)
        noise = O.make_noise(oconf, seed=noise_seed + step)
        with MarginPatch() as mp:
            _queue_step(mp, rconf, noise)
            losses, new_state, metrics, tensors, dream_tensors = model.training_step(obs, state)
            assert not mp.queue and not mp.eps_queue and not mp.std_queue, 'draws left unused'
            idx = _indices(mp, rconf)
            min_edge = min(min_edge, mp.min_edge)
        if min_edge <= MIN_EDGE:
            return None, min_edge
        assert dream_tensors == {} and not [k for k in {**metrics, **tensors} if 'image' in k]
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
        for k in ('u_post', 'u_act', 'u_prior', 'eps_act'):
            out[pre + 'in_' + k] = noise[k].numpy()
        out[pre + 'in_state_h'] = state[0].numpy()
        out[pre + 'in_state_z'] = state[1].numpy()
        out[pre + 'losses'] = np.array([float(l) for l in losses], dtype=np.float64)
        for k, v in {**metrics, **grad_metrics}.items():
            out[pre + 'metric_' + k] = np.array(float(v), dtype=np.float64)
        for k, v in tensors.items():
            out[pre + 'tensor_' + k] = v.detach().numpy()
        out[pre + 'out_state_h'] = new_state[0].numpy()
        out[pre + 'out_state_z'] = new_state[1].numpy()
        for k, v in idx.items():
            out[pre + k] = v
        out[pre + 'grad_norms'] = np.array([float(g.double().norm()) for g in grads.values()])
        out[pre + 'grad_names'] = np.array(list(grads.keys()))
        for k in full_grads:
            out[pre + 'grad_' + k] = grads[k].numpy()
        post = dict(model.state_dict())
        out[pre + 'param_abs_sums'] = np.array([float(v.double().abs().sum()) for v in post.values()])
        state = new_state
        print(f'  step {step}: losses', out[pre + 'losses'], 'grad_norm', float(grad_metrics['grad_norm']))
    out['min_edge_distance'] = np.array(min_edge)
    return out, min_edge


def _save(name, out):
    path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, f'{os.path.getsize(path) / 1024:.0f} KiB', 'min edge distance', float(out['min_edge_distance']))


def run(name, overrides, steps, full_grads=(), grads_file=False):
    """grads_file: the full gradients, of the first step only, go to a companion <name>_grads.npz."""
    seed = 777
    while True:
        print(f'[{name}] noise seed {seed}')
        out, min_edge = _attempt(overrides, steps, full_grads, seed)
        if out is not None:
            break
        print(f'[{name}] a uniform lies {min_edge:.2e} from a CDF edge (<= {MIN_EDGE}): next seed')
        seed += 1000
    if grads_file:
        full = {k: out.pop(k) for k in list(out) if k[3:].startswith('grad_') and k[3:] not in ('grad_norms', 'grad_names')}
        path = os.path.join(ROOT, 'tests', 'golden', f'{name}_grads.npz')
        np.savez_compressed(path, **{k: v for k, v in full.items() if k.startswith('s0_')})
        print('wrote', path, f'{os.path.getsize(path) / 1024:.0f} KiB')
    _save(name, out)


def run_eval(name, overrides, do_open_loop=False):
    """do_image_pred + do_dream_tensors (+ do_open_loop) under no_grad (train.py:353-359,380-385).  There is no image decoder, so the
    log dream is skipped (dreamer.py:164): it draws nothing and dream_tensors is {}."""
    seed = 999
    while True:
        rconf, oconf, model, out = _reference_model(overrides)
        T, B, S, H = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon
        raw = make_batch(oconf, 0, rconf.vecobs_size)
        noise = O.make_noise(oconf, seed=seed)
        with MarginPatch() as mp:
            mp.queue = [noise['u_post'][t] for t in range(T)] + [noise['u_pred'].reshape(-1, S)]
            for i in range(H):
                mp.queue += [noise['u_act'][i], noise['u_prior'][i]]
            with torch.no_grad():
                losses, new_state, metrics, tensors, dream_tensors = model.training_step(
                    to_obs(raw, oconf), model.init_state(B), do_image_pred=True, do_dream_tensors=True, do_open_loop=do_open_loop)
            assert not mp.queue and dream_tensors == {}
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
        out['tensor_' + k] = v.detach().numpy()
    out.update(idx_post=torch.stack(mp.idx[:T]).reshape(T, B, S).numpy().astype(np.uint8), out_state_h=new_state[0].numpy(),
               idx_pred=mp.idx[T].reshape(T, B, S).numpy().astype(np.uint8), open_loop=np.array(bool(do_open_loop)),
               min_edge_distance=np.array(mp.min_edge), noise_seed=np.array(seed))
    _save(name, out)


def run_inference(name, overrides):
    """Dreamer.inference (dreamer.py:92-111) on an obs without `image`: one step, (1,B,...) inputs, the posterior draw pinned."""
    seed = 31
    while True:
        rconf, oconf, model, out = _reference_model(overrides)
        B, S, C, A, V = 3, rconf.stoch_dim, rconf.stoch_discrete, rconf.action_dim, rconf.vecobs_size
        g = torch.Generator().manual_seed(seed)
        action = torch.nn.functional.one_hot(torch.randint(0, A, (1, B), generator=g), A).float()
        reset = torch.tensor([[True, False, False]])
        h = torch.tanh(torch.randn(B, rconf.deter_dim, generator=g))
        z = torch.nn.functional.one_hot(torch.randint(0, C, (B, S), generator=g), C).float().reshape(B, S * C)
        u = torch.rand(1, B, S, generator=g)
        reward = torch.tanh(torch.randn(1, B, generator=g))
        terminal = torch.tensor([[0.0, 1.0, 0.0]])
        vecobs = torch.randn(1, B, V, generator=g)
        obs = dict(action=action, reset=reset, reward=reward, terminal=terminal, vecobs=vecobs)
        with MarginPatch() as mp, torch.no_grad():
            mp.queue = [u[0]]
            dist, (h1, z1), metrics = model.inference(obs, (h, z))
            assert not mp.queue
        if mp.min_edge > MIN_EDGE:
            break
        seed += 1000
    out.update(in_action=action.numpy(), in_reset=reset.numpy(), in_reward=reward.numpy(), in_terminal=terminal.numpy(),
               in_vecobs=vecobs.numpy(), in_h=h.numpy(), in_z=z.numpy(), in_u=u.numpy(), action_probs=dist.probs.numpy(),
               out_h=h1.numpy(), out_z=z1.numpy(), policy_value=np.array(float(metrics['policy_value'])),
               min_edge_distance=np.array(mp.min_edge), noise_seed=np.array(seed))
    _save(name, out)


def run_amp(name, overrides):
    """The reference's mixed-precision forward (train.py:166), made as tiny_obs_amp was: one no_grad step in fp32 and one under
    torch.autocast('cpu', bfloat16); the seed is advanced until both passes draw the same posterior indices."""
    seed = 777
    while True:
        rconf, oconf, model, out = _reference_model(overrides)
        T, B, S, H = rconf.batch_length, rconf.batch_size, rconf.stoch_dim, rconf.imag_horizon
        raw = make_batch(oconf, 0, rconf.vecobs_size)
        noise = O.make_noise(oconf, seed=seed)
        for k, v in raw.items():
            out['in_' + k] = v
        for k in ('u_post', 'u_act', 'u_prior'):
            out['in_' + k] = noise[k].numpy()
        edge = float('inf')
        for tag, amp in (('fp32', False), ('bf16', True)):
            with MarginPatch() as mp:
                _queue_step(mp, rconf, noise)
                with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16, enabled=amp):
                    losses, _, metrics, _, _ = model.training_step(to_obs(raw, oconf), model.init_state(B))
                post_idx = torch.stack(mp.idx[:T]).reshape(T, B, S)
                if not amp:
                    edge = mp.min_edge
            out[tag + '_losses'] = np.array([float(l) for l in losses], dtype=np.float64)
            for k, v in metrics.items():
                out[tag + '_metric_' + k] = np.array(float(v), dtype=np.float64)
            out[tag + '_idx_post'] = post_idx.numpy().astype(np.uint8)
            print(f'[{name}] {tag}: losses', out[tag + '_losses'])
        same = np.array_equal(out['fp32_idx_post'], out['bf16_idx_post'])
        if edge > MIN_EDGE and same:
            break
        print(f'[{name}] seed {seed}: edge distance {edge:.2e}, fp32 and bf16 passes drew the same posterior indices: {same}: next seed')
        seed += 1000
    out.update(min_edge_distance=np.array(edge), noise_seed=np.array(seed))
    _save(name, out)


def run_preprocess(name):
    """The reference Preprocessor(image_key=None, action_dim=2, clip_rewards='tanh') on one small synthetic batch: the raw fields
    as `in_*`, every field of the result as `out_*`."""
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from pydreamer.preprocessing import Preprocessor
    rs = np.random.RandomState(7)
    T, B, V = 4, 3, 4
    raw = dict(action=rs.randint(0, 2, (T, B)).astype(np.int64), action_next=rs.randint(0, 2, (T, B)).astype(np.int64),
               reward=(3 * rs.randn(T, B)).astype(np.float64), terminal=(rs.rand(T, B) < 0.3), reset=(rs.rand(T, B) < 0.3),
               vecobs=rs.randn(T, B, V).astype(np.float64))
    got = Preprocessor(image_key=None, action_dim=2, clip_rewards='tanh').apply({k: v.copy() for k, v in raw.items()})
    assert 'image' not in got and got['vecobs'].dtype == np.float32
    out = {'in_' + k: v for k, v in raw.items()}
    out.update({'out_' + k: np.asarray(v) for k, v in got.items()})
    path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, sorted(got))


if __name__ == '__main__':
    ALL = ['tiny_vectorenv', 'tiny_vectorenv_iwae', 'tiny_vectorenv_cont', 'tiny_vectorenv_eval', 'tiny_vectorenv_open_loop',
           'tiny_vectorenv_inference', 'tiny_vectorenv_amp', 'vectorenv_preprocess']
    which = sys.argv[1:] or ALL
    EV, DV = 'wm.encoder.encoder_vecobs.model', 'wm.decoder.vecobs.model.model'
    if 'tiny_vectorenv' in which:
        # the first and the last Linear of both vecobs MLPs, the embedding's way into the posterior, the reward head's last Linear
        run('tiny_vectorenv', {}, steps=2, grads_file=True,
            full_grads=(f'{EV}.0.weight', f'{EV}.6.weight', f'{DV}.0.weight', f'{DV}.12.weight', 'wm.core.cell.post_mlp_e.weight',
                        'wm.decoder.reward.model.model.12.weight'))
    if 'tiny_vectorenv_iwae' in which:
        run('tiny_vectorenv_iwae', dict(iwae_samples=2, reward_input=True, gru_type='gru_layernorm'), steps=1)
    if 'tiny_vectorenv_cont' in which:
        run('tiny_vectorenv_cont', dict(actor_dist='tanh_normal', action_dim=3, stoch_discrete=0, aux_critic=True), steps=1)
    if 'tiny_vectorenv_eval' in which:
        run_eval('tiny_vectorenv_eval', {})
    if 'tiny_vectorenv_open_loop' in which:
        run_eval('tiny_vectorenv_open_loop', {}, do_open_loop=True)
    if 'tiny_vectorenv_inference' in which:
        run_inference('tiny_vectorenv_inference', {})
    if 'tiny_vectorenv_amp' in which:
        run_amp('tiny_vectorenv_amp', {})
    if 'vectorenv_preprocess' in which:
        run_preprocess('vectorenv_preprocess')
