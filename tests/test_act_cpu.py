"""The acting path without a GPU: the two dm_policy_draw symbols (exported, declared, bound; the ABI version unchanged), every
host-side refusal of dm_policy_draw, NetworkPolicy over a stub model (state carry, action shapes, reset_state, metrics as Python
floats, the single-step preprocessing adapter) and Dreamer.act's refusals, which come before any library call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import dreamer_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['dm_policy_draw_ws_floats', 'dm_policy_draw']
DM_E_SHAPE, DM_E_WORKSPACE, DM_E_NULL = -1, -2, -5


def test_new_symbols_and_host_side_argument_checks(hip):
    assert set(NEW_SYMBOLS) <= set(hip.exported_symbols())
    hdr = open(os.path.join(ROOT, 'include', 'dreamer_hip.h')).read()
    declared = set(re.findall(r'\b(dm_[a-z0-9_]+)\s*\(', hdr))
    lib = hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name)
    assert lib.dm_version() == hip.DM_ABI_VERSION == 17
    assert lib.dm_policy_draw_ws_floats(0) == 0 and lib.dm_policy_draw_ws_floats(-3) == 0
    rows, A = 5, 6
    wsb = 4 * lib.dm_policy_draw_ws_floats(rows)
    assert wsb >= 4 * 2 * rows
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its host-side checks

    def draw(kind=0, rows=rows, A=A, params=fake, ldp=None, noise=fake, value=fake, action=fake, lda=None, stats=fake, ws=fake,
             wsb=wsb):
        width = A if kind == 0 else 2 * A
        return lib.dm_policy_draw(kind, rows, A, params, width if ldp is None else ldp, noise, value, action, A if lda is None else lda,
                                  None, None, None, stats, ws, wsb, None)

    for kw in (dict(params=None), dict(noise=None), dict(action=None), dict(stats=None), dict(ws=None)):
        assert draw(**kw) == DM_E_NULL, kw
        assert b'null' in lib.dm_last_error()
    for kw in (dict(rows=0), dict(rows=-1), dict(A=0), dict(kind=3), dict(kind=-1), dict(ldp=A - 1), dict(kind=1, ldp=2 * A - 1),
               dict(kind=2, ldp=A), dict(lda=A - 1)):
        assert draw(**kw) == DM_E_SHAPE, kw
        assert lib.dm_last_error()
    for kind in (0, 1, 2):
        assert draw(kind=kind, wsb=wsb - 4) == DM_E_WORKSPACE
        assert b'workspace' in lib.dm_last_error()
        assert draw(kind=kind, wsb=0) == DM_E_WORKSPACE


# ------------------------------------------------------------------------------------------------ NetworkPolicy over a stub
class _StubModel:
    """act() returns fixed tensors that depend on the call count and records what it was given."""

    def __init__(self, A=3, D=4):
        self.A, self.D, self.calls = A, D, []

    def init_state(self, batch_size):
        return (torch.zeros(batch_size, self.D), torch.zeros(batch_size, 2))

    def act(self, obs, in_state, noise=None, return_rows=False):
        n = len(self.calls) + 1
        self.calls.append((obs, in_state))
        B = obs['action'].shape[1]
        action = torch.zeros(1, B, self.A)
        action[0, torch.arange(B), (torch.arange(B) + n) % self.A] = 1.0
        stats = torch.tensor([0.5 * n, 0.25, 1.0 + n, 0.0])
        out_state = (in_state[0] + n, in_state[1] + 10 * n + torch.arange(B).float().view(B, 1))
        return action, out_state, dict(policy_value=stats[0], action_prob=stats[1], policy_entropy=stats[2])


def _env_obs(B, A, step):
    return dict(action=np.eye(A, dtype=np.float32)[np.arange(B) % A][None], reward=np.full((1, B), float(step), np.float32),
                reset=np.zeros((1, B), bool), terminal=np.zeros((1, B), np.float32))


@pytest.mark.parametrize('B', [1, 3])
def test_network_policy_carries_state_and_shapes_the_action(B):
    from pydreamer_amd import NetworkPolicy
    model = _StubModel()
    policy = NetworkPolicy(model, lambda obs: obs, batch_size=B, device='cpu')
    assert all(float(s.abs().max()) == 0.0 and s.shape[0] == B for s in policy.state)
    for step in (1, 2):
        action, metrics = policy(_env_obs(B, model.A, step))
        assert isinstance(action, np.ndarray) and action.dtype == np.float32
        assert action.shape == ((model.A,) if B == 1 else (B, model.A))
        want = np.zeros((B, model.A), np.float32)
        want[np.arange(B), (np.arange(B) + step) % model.A] = 1.0
        assert np.array_equal(action.reshape(B, model.A), want)
        assert set(metrics) == {'policy_value', 'action_prob', 'policy_entropy'}
        assert all(type(v) is float for v in metrics.values())
        assert metrics == dict(policy_value=0.5 * step, action_prob=0.25, policy_entropy=1.0 + step)
    # the second call was given the state the first one returned; the fields reached the model as (1, B, ...) tensors
    obs2, state2 = model.calls[1]
    assert float(state2[0].max()) == 1.0 and torch.equal(state2[1], 10.0 + torch.arange(B).float().view(B, 1).expand(B, 2))
    assert torch.equal(policy.state[0], torch.full((B, model.D), 3.0))
    assert obs2['action'].shape == (1, B, model.A) and obs2['reset'].dtype == torch.bool and float(obs2['reward'][0, 0]) == 2.0
    with pytest.raises(ValueError):
        policy(_env_obs(B + 1, model.A, 3))


def test_network_policy_reset_state():
    from pydreamer_amd.policy import NetworkPolicy
    model = _StubModel()
    policy = NetworkPolicy(model, lambda obs: obs, batch_size=3, device='cpu')
    policy(_env_obs(3, model.A, 1))
    before = tuple(s.clone() for s in policy.state)
    assert all(float(s.abs().min()) > 0 for s in before)
    policy.reset_state(np.array([False, True, False]))
    for s, b in zip(policy.state, before):
        assert float(s[1].abs().max()) == 0.0 and torch.equal(s[[0, 2]], b[[0, 2]])
    with pytest.raises(ValueError):
        policy.reset_state([True, False])
    policy.reset_state()
    assert all(float(s.abs().max()) == 0.0 for s in policy.state)


def test_step_preprocessor_single_and_batched():
    from pydreamer_amd.policy import StepPreprocessor
    A = 4
    one = dict(image=np.zeros((64, 64, 3), np.uint8), action=np.eye(A, dtype=np.float32)[2], reward=np.float32(3.0),
               terminal=np.bool_(False), reset=np.bool_(True), policy_value=np.float32(7.0), action_prob=np.float32(0.5))
    out = StepPreprocessor(A, clip_rewards='tanh')(one)
    assert 'policy_value' not in out and 'action_prob' not in out
    assert out['image'].shape == (1, 1, 64, 64, 3) and out['image'].dtype == np.uint8
    assert out['action'].shape == (1, 1, A) and out['reset'].shape == (1, 1) and bool(out['reset'][0, 0])
    assert abs(float(out['reward'][0, 0]) - np.tanh(3.0)) < 1e-6 and out['terminal'].dtype == np.float32
    many = dict(vecobs=np.ones((5, 7)), action=np.arange(5) % A, reward=np.zeros(5), terminal=np.zeros(5), reset=np.zeros(5, bool))
    out = StepPreprocessor(A, image_key=None, batched=True)(many)
    assert 'image' not in out and out['vecobs'].shape == (1, 5, 7) and out['vecobs'].dtype == np.float32
    assert out['action'].shape == (1, 5, A) and np.array_equal(out['action'][0].argmax(-1), np.arange(5) % A)


# ------------------------------------------------------------------------------------------------ Dreamer.act's refusals
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f'Dreamer.act reached the library ({name}) before refusing its arguments')


@pytest.mark.parametrize('actor_dist', ['onehot', 'tanh_normal'])
def test_act_refuses_bad_arguments_before_any_library_call(monkeypatch, actor_dist):
    from pydreamer_amd import config, hip as H
    from pydreamer_amd.models import Dreamer
    oconf = O.tiny_conf()
    conf = config.load_config('defaults', 'atari', **{**vars(oconf), 'actor_dist': actor_dist})
    with torch.device('meta'):
        model = Dreamer(conf)
    monkeypatch.setattr(H, '_lib', _NoLibrary())
    monkeypatch.setattr(H, 'call', lambda *a, **k: (_ for _ in ()).throw(AssertionError('library call')))
    B, A = 3, conf.action_dim
    state = model.init_state(B)
    with pytest.raises(AssertionError, match='previous action'):
        model.act({}, state)
    for shape in ((2, B, A), (B, A)):      # T != 1, no time axis
        with pytest.raises(AssertionError, match='Expected shape'):
            model.act(dict(action=torch.zeros(shape, device='meta')), state)
    obs = dict(action=torch.zeros(1, B, A, device='meta'))
    good = (B,) if actor_dist == 'onehot' else (B, A)
    for bad in ((B, A) if actor_dist == 'onehot' else (B,), (B + 1,) + good[1:], (1,) + good):
        with pytest.raises(ValueError, match='actor noise'):
            model.act(obs, state, noise=dict(u_act=torch.zeros(bad)))
