"""CPU (-m "not gpu"): the host side of the two-hot symlog critic and the percentile return normalisation - the
three entry points of csrc/twohot.hip are declared and bound and refuse bad arguments on the host with nothing launched, the
config keys are inert by default in every section, ActorCritic refuses bad values at construction (on the meta device, before
anything is allocated), the default model's state_dict is unchanged while the switches add the K-wide critic layers and
ac.return_range, and the fp32 percentile rule of tests/twohot_case.py agrees with numpy's float64 linear percentile."""
import os
import re

import numpy as np
import pytest
import torch

from pydreamer_amd import config, hip
from tests import twohot_case as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DM_E_SHAPE, DM_E_NULL = -1, -5
P = 64      # a placeholder pointer a launch would fault on
KEYS = dict(critic_dist='mse', critic_bins=255, critic_bin_range=20.0, return_norm='none', return_norm_lo=0.05, return_norm_hi=0.95,
            return_norm_decay=0.99, return_norm_limit=1.0)


def _rc(name, *args):
    return getattr(hip.lib(), name)(*args)


def _err():
    return hip.lib().dm_last_error().decode()


def _meta(conf):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'):
        return Dreamer(conf)


def test_symbols_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'dreamer_hip.h')).read()
    declared = set(re.findall(r'\b(dm_[a-z0-9_]+)\s*\(', hdr))
    lib = hip.lib()
    for n in ('dm_twohot_decode', 'dm_twohot_loss', 'dm_return_norm'):
        assert n in declared and n in hip.exported_symbols() and hasattr(lib, n), n
    assert lib.dm_version() == hip.DM_ABI_VERSION == 17
    src = open(os.path.join(ROOT, 'pydreamer_amd', 'csrc', 'twohot.hip')).read()
    assert '#pragma clang fp contract(off)' in src and 'atomicAdd(&hist' in src      # integer LDS adds only
    from pydreamer_amd import models as M
    assert M.METRIC_BUF_FLOATS == 48 and not set(M.RETURN_METRIC_SLOTS) & set(M.METRIC_SLOTS)
    assert sorted(M.RETURN_METRIC_SLOTS.values()) == [42, 43, 44]
    assert not set(M.RETURN_METRIC_SLOTS.values()) & (set(M.METRIC_SLOTS.values()) | set(M.GOALS_METRIC_SLOTS.values()))


def test_twohot_decode_checks_arguments_on_the_host():
    """dm_twohot_decode(rows, K, logits, ld, bins, value, stream): every failing call returns before a launch."""
    ok = dict(rows=3, K=255, logits=P, ld=255, bins=P, value=P, stream=None)
    call = lambda **kw: _rc('dm_twohot_decode', *{**ok, **kw}.values())
    for K in (1, 0, -3, 257):
        assert call(K=K, ld=300) == DM_E_SHAPE and f'K={K}' in _err() and 'twohot_decode' in _err()
    assert call(rows=-1) == DM_E_SHAPE and 'rows=-1' in _err()
    assert call(ld=254) == DM_E_SHAPE and 'ld=254' in _err()
    for gone in ('logits', 'bins', 'value'):
        assert call(**{gone: None}) == DM_E_NULL and 'null' in _err() and 'twohot_decode' in _err(), gone
    assert call(rows=0) == 0      # nothing to do, nothing launched
    with pytest.raises(hip.DreamerHipError, match='twohot_decode'):
        hip.call('dm_twohot_decode', 3, 300, P, 300, P, P, None)


def test_twohot_loss_checks_arguments_on_the_host():
    """dm_twohot_loss(rows, rows_total, K, logits, ld, bins, target, weight, scale, loss, dlogits, value, stream)."""
    ok = dict(rows=3, rows_total=5, K=7, logits=P, ld=7, bins=P, target=P, weight=P, scale=1.0, loss=P, dlogits=P, value=P, stream=None)
    call = lambda **kw: _rc('dm_twohot_loss', *{**ok, **kw}.values())
    for K in (1, 257):
        assert call(K=K, ld=300) == DM_E_SHAPE and f'K={K}' in _err() and 'twohot_loss' in _err()
    assert call(rows=-1) == DM_E_SHAPE and call(rows_total=2) == DM_E_SHAPE and 'rows_total=2' in _err()
    assert call(ld=6) == DM_E_SHAPE and 'ld=6' in _err()
    for gone in ('logits', 'bins', 'target', 'weight', 'loss'):
        assert call(**{gone: None}) == DM_E_NULL and 'null' in _err() and 'twohot_loss' in _err(), gone
    assert call(rows=0, rows_total=0) == 0 and call(rows=0, rows_total=4, dlogits=None) == 0
    with pytest.raises(hip.DreamerHipError, match='twohot_loss'):
        hip.call('dm_twohot_loss', 3, 2, 7, P, 7, P, P, P, 1.0, P, P, None, None)


def test_return_norm_checks_arguments_on_the_host():
    """dm_return_norm(n, x, q_lo, q_hi, decay, limit, update, state, out, adv, n_adv, stream)."""
    ok = dict(n=100, x=P, q_lo=0.05, q_hi=0.95, decay=0.99, limit=1.0, update=1, state=P, out=P, adv=P, n_adv=100, stream=None)
    call = lambda **kw: _rc('dm_return_norm', *{**ok, **kw}.values())
    for n in (0, -5):
        assert call(n=n) == DM_E_SHAPE and f'n={n}' in _err() and 'return_norm' in _err()
    assert call(n_adv=-1) == DM_E_SHAPE and 'n_adv=-1' in _err()
    for q in (dict(q_lo=-0.1), dict(q_hi=1.5), dict(q_lo=0.6, q_hi=0.4), dict(q_lo=float('nan')), dict(q_hi=float('nan'))):
        assert call(**q) == DM_E_SHAPE and 'q_lo' in _err(), q
    for decay in (-0.1, 1.0, 1.5, float('nan')):
        assert call(decay=decay) == DM_E_SHAPE and 'decay' in _err()
    for limit in (0.0, -1.0, float('inf'), float('nan')):
        assert call(limit=limit) == DM_E_SHAPE and 'limit' in _err()
    for gone in ('x', 'state', 'out', 'adv'):
        assert call(**{gone: None}) == DM_E_NULL and 'null' in _err() and 'return_norm' in _err(), gone
    with pytest.raises(hip.DreamerHipError, match='return_norm'):
        hip.call('dm_return_norm', 0, P, 0.05, 0.95, 0.99, 1.0, 1, P, P, P, 0, None)


def test_config_defaults_and_overrides():
    for name in config.SECTIONS:
        c = config.load_config('defaults', name) if name != 'defaults' else config.load_config('defaults')
        assert {k: getattr(c, k) for k in KEYS} == KEYS, name
        over = dict(critic_dist='twohot', critic_bins=31, critic_bin_range=10.0, return_norm='percentile', return_norm_lo=0.1,
                    return_norm_hi=0.9, return_norm_decay=0.5, return_norm_limit=2.0)
        c = config.load_config('defaults', name, **over)
        assert {k: getattr(c, k) for k in over} == over, name
    ac = _meta(config.load_config('defaults', 'atari', **over)).ac
    assert (ac.critic_dist, ac.critic_bins, ac.critic_bin_range, ac.return_norm, ac.return_norm_q, ac.return_norm_decay,
            ac.return_norm_limit) == ('twohot', 31, 10.0, 'percentile', (0.1, 0.9), 0.5, 2.0)
    # the auxiliary critic keeps the defaults
    aux = _meta(config.load_config('defaults', 'atari', aux_critic=True, **over)).wm.ac_aux
    assert (aux.critic_dist, aux.return_norm, aux.critic.out_dim) == ('mse', 'none', 1)


@pytest.mark.parametrize('bad', [dict(critic_bins=1), dict(critic_bins=257), dict(critic_bins=0), dict(critic_bin_range=0.0),
                                 dict(critic_bin_range=-1.0), dict(critic_bin_range=float('inf')), dict(critic_bin_range=float('nan')),
                                 dict(critic_dist='gauss'), dict(return_norm='ema'), dict(return_norm_lo=-0.1),
                                 dict(return_norm_hi=1.1), dict(return_norm_lo=0.6, return_norm_hi=0.4), dict(return_norm_decay=1.0),
                                 dict(return_norm_decay=-0.5), dict(return_norm_limit=0.0), dict(return_norm_limit=-1.0)])
def test_refusals_at_construction(bad):
    from pydreamer_amd.models import ActorCritic
    key = next(iter(bad))
    with pytest.raises(ValueError, match=key):
        _meta(config.load_config('defaults', 'atari', **bad))
    with torch.device('meta'), pytest.raises(ValueError, match=key):
        ActorCritic(in_dim=40, out_actions=3, **bad)
    # ... whatever the other switch says: the values are checked even while the feature they belong to is off
    with torch.device('meta'), pytest.raises(ValueError, match=key):
        ActorCritic(in_dim=40, out_actions=3, **{**dict(critic_dist='twohot', return_norm='percentile'), **bad})


def test_state_dict_keys():
    from pydreamer_amd.models import ActorCritic, MLP
    base = _meta(config.load_config('defaults', 'atari'))
    keys = list(base.state_dict())
    # today's list: the three MLPs of the actor-critic, four hidden layers each, and nothing else under `ac.`
    mlp_keys = [f'model.{3 * i + j}.{w}' for i in range(4) for j in (0, 1) for w in ('weight', 'bias')] + ['model.12.weight', 'model.12.bias']
    assert [k for k in keys if k.startswith('ac.')] == [f'ac.{m}.{k}' for m in ('actor', 'critic', 'critic_target') for k in mlp_keys]
    assert base.state_dict()['ac.critic.model.12.weight'].shape == (1, 400)
    assert not hasattr(base.ac, 'bins') and not hasattr(base.ac, 'return_range')
    on = _meta(config.load_config('defaults', 'atari', critic_dist='twohot', critic_bins=31, return_norm='percentile'))
    sd = on.state_dict()
    assert [k for k in sd if k != 'ac.return_range'] == keys and sd['ac.return_range'].shape == (2,)
    for m in ('critic', 'critic_target'):
        assert sd[f'ac.{m}.model.12.weight'].shape == (31, 400) and sd[f'ac.{m}.model.12.bias'].shape == (31,)
    assert 'ac.bins' not in sd and on.ac.bins.shape == (31,)
    assert list(_meta(config.load_config('defaults', 'atari', critic_dist='twohot')).state_dict()) == keys
    # a real (CPU) module: the output layer is zero, the bins are the fp32 linspace, the range starts at zero
    ac = ActorCritic(in_dim=24, out_actions=3, critic_dist='twohot', critic_bins=7, critic_bin_range=5.0, return_norm='percentile')
    assert isinstance(ac.critic, MLP) and ac.critic.out_dim == 7 and ac.critic_target.out_dim == 7
    assert not ac.critic.model[12].weight.any() and not ac.critic.model[12].bias.any() and ac.critic.model[9].weight.any()
    assert torch.equal(ac.bins, torch.linspace(-5.0, 5.0, 7)) and torch.equal(ac.return_range, torch.zeros(2))
    assert all(not p.requires_grad for p in ac.critic_target.parameters())


def test_packed_metric_names_follow_the_switch():
    from pydreamer_amd import models as M
    from pydreamer_amd.train import default_slots
    off, on = _meta(config.load_config('defaults', 'atari')), _meta(config.load_config('defaults', 'atari', return_norm='percentile'))
    off.metric_buffer = on.metric_buffer = None
    assert off.packed_metrics()[0] == list(M.METRIC_SLOTS)
    names, _, idx = on.packed_metrics()
    assert names == list(M.METRIC_SLOTS) + list(M.RETURN_METRIC_SLOTS) and idx[-3:] == [42, 43, 44]
    assert 'policy_return_scale' not in default_slots(off) and default_slots(on)['policy_return_scale'][0] == 44


def test_data_parallel_refusal(monkeypatch):
    from pydreamer_amd import dist as DD
    on, off = _meta(config.load_config('defaults', 'atari', return_norm='percentile')), _meta(config.load_config('defaults', 'atari'))
    monkeypatch.setattr(DD.dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(DD.dist, 'get_world_size', lambda group=None: 2)
    with pytest.raises(NotImplementedError, match='percentile'):
        DD.attach([], 3, 6, model=on)
    DD.attach([], 3, 6, model=off)      # (no optimizers, no _opt: nothing to attach, nothing refused)
    monkeypatch.setattr(DD.dist, 'get_world_size', lambda group=None: 1)
    DD.attach([], 3, 3, model=on, force=True)


@pytest.mark.parametrize('n', [1, 2, 3, 65, 1025, 37500])
def test_fp32_percentile_rule_against_numpy(n):
    rs = np.random.RandomState(n)
    # (values away from zero: the bound is relative to the percentile itself)
    for x in (rs.randn(n).astype(np.float32) * 30 - 200, np.abs(rs.randn(n)).astype(np.float32) + 5):
        s = TC.sort_total(x)
        assert np.array_equal(s, np.sort(x))
        for q in (0.0, 0.05, 0.5, 0.95, 1.0):
            got, want = float(TC.percentile_f32(s, q)), float(np.percentile(x.astype(np.float64), 100 * q, method='linear'))
            assert abs(got - want) <= 1e-5 * abs(want), (n, q, got, want)
    # the total order puts -0 below +0 and keeps ties together
    z = np.array([0.0, -0.0, 1.0, -1.0, -0.0, 0.0], np.float32)
    assert np.signbit(TC.sort_total(z)).tolist() == [True, True, True, False, False, False]
    out, st, adv = TC.return_norm_f32(np.array([1.0, 3.0], np.float32), 0.0, 1.0, 0.5, 1.0, 1, np.array([0.0, 0.0], np.float32),
                                      np.array([4.0], np.float32))
    assert out.tolist() == [1.0, 3.0, 0.5, 1.5, 1.0] and st.tolist() == [0.5, 1.5] and adv.tolist() == [4.0]
