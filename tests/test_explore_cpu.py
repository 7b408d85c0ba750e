"""CPU (-m "not gpu"): the host side of Plan2Explore - the two entry points of csrc/disag.hip are exported, declared
and bound and refuse bad arguments on the host, the config keys are inert by default, Plan2Explore builds on `meta` with K heads
of the stated shapes without touching the Dreamer's state_dict, and a greedy run() never imports the module."""
import os
import re
import sys

import pytest
import torch

from pydreamer_amd import config, hip, replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DM_E_SHAPE, DM_E_NULL = -1, -5
ENTRIES = ('dm_disag_reward', 'dm_ensemble_mse')


def _rc(name, *args):
    return getattr(hip.lib(), name)(*args)


def _err():
    return hip.lib().dm_last_error().decode()


def test_entries_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'dreamer_hip.h')).read()
    assert re.search(r'#define DM_E_SHAPE \(-1\)', hdr) and re.search(r'#define DM_E_NULL \(-5\)', hdr)
    declared = set(re.findall(r'\b(dm_[a-z0-9_]+)\s*\(', hdr))
    lib = hip.lib()
    for n in ENTRIES:
        assert n in declared and n in hip.exported_symbols() and hasattr(lib, n), n
    assert lib.dm_version() == hip.DM_ABI_VERSION == 17
    assert os.path.exists(os.path.join(ROOT, 'pydreamer_amd', 'csrc', 'disag.hip'))


def test_disag_reward_checks_arguments_on_the_host():
    """dm_disag_reward(K, rows, D, means, head_stride, ld, scale, reward, stream).  Nothing is launched: every pointer is NULL or a
    placeholder a launch would fault on."""
    P = 64
    ok = dict(K=3, rows=4, D=5, means=P, head_stride=20, ld=5, scale=1.0, reward=P, stream=None)
    call = lambda **kw: _rc('dm_disag_reward', *{**ok, **kw}.values())
    for K in (1, 0, -3, 17, 100):
        assert call(K=K) == DM_E_SHAPE and f'K={K}' in _err(), K
    assert call(rows=-1) == DM_E_SHAPE and 'rows=-1' in _err()
    for D in (0, -2):
        assert call(D=D) == DM_E_SHAPE and f'D={D}' in _err()
    assert call(ld=4) == DM_E_SHAPE and 'ld=4' in _err()
    assert call(means=None) == DM_E_NULL and 'null' in _err()
    assert call(reward=None) == DM_E_NULL
    for K in (2, 16):      # the ends of the range pass the checks: zero rows, nothing launched
        assert call(K=K, rows=0) == 0
    assert call(rows=0, ld=9, head_stride=1 << 40) == 0
    with pytest.raises(hip.DreamerHipError, match='disag_reward'):
        hip.call('dm_disag_reward', 1, 4, 5, P, 20, 5, 1.0, P, None)


def test_ensemble_mse_checks_arguments_on_the_host():
    """dm_ensemble_mse(K, rows, D, means, head_stride, ld, target, ldt, skip, scale, loss, dmeans, stream)."""
    P = 64
    ok = dict(K=3, rows=4, D=5, means=P, head_stride=20, ld=5, target=P, ldt=5, skip=P, scale=1.0, loss=P, dmeans=P, stream=None)
    call = lambda **kw: _rc('dm_ensemble_mse', *{**ok, **kw}.values())
    for K in (1, 0, -1, 17):
        assert call(K=K) == DM_E_SHAPE and f'K={K}' in _err(), K
    assert call(rows=-1) == DM_E_SHAPE and 'rows=-1' in _err()
    assert call(D=0) == DM_E_SHAPE and 'D=0' in _err()
    assert call(ld=4) == DM_E_SHAPE and 'ld=4' in _err()
    assert call(ldt=4) == DM_E_SHAPE and 'ldt=4' in _err()
    for gone in ('means', 'target', 'loss'):
        assert call(**{gone: None}) == DM_E_NULL and 'null' in _err(), gone
    # skip and dmeans are optional; zero rows: nothing launched
    assert call(rows=0) == 0 and call(rows=0, skip=None, dmeans=None) == 0 and call(rows=0, K=16, ldt=1000) == 0
    with pytest.raises(hip.DreamerHipError, match='ensemble_mse'):
        hip.call('dm_ensemble_mse', 3, 4, 5, P, 20, 5, P, 4, None, 1.0, P, None, None)


def test_config_defaults_are_inert():
    want = dict(expl_behavior='greedy', disag_models=10, disag_action_cond=True, expl_intr_scale=1.0, expl_extr_scale=0.0,
                expl_until=0, adam_lr_expl=3.0e-4)
    for sections in (('defaults',), ('defaults', 'atari'), ('defaults', 'minigrid'), ('defaults', 'vectorenv')):
        c = config.load_config(*sections)
        assert {k: getattr(c, k) for k in want} == want, sections
    assert config.load_config('defaults', expl_behavior='plan2explore', disag_models=5).disag_models == 5


def _meta(conf):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'):
        return Dreamer(conf)


@pytest.mark.parametrize('section,K,cond', [('atari', 10, True), ('minigrid', 3, True), ('vectorenv', 16, False)])
def test_builds_on_meta_and_leaves_the_dreamer_alone(section, K, cond):
    from pydreamer_amd.models import MLP_HIDDEN, ActorCritic
    conf = config.load_config('defaults', section, disag_models=K, disag_action_cond=cond)
    d = _meta(conf)
    keys = list(d.state_dict())
    from pydreamer_amd.explore import EXPLORE_METRIC_SLOTS, Plan2Explore
    assert list(d.state_dict()) == keys, 'importing explore changed the Dreamer'
    with torch.device('meta'):
        p = Plan2Explore(conf, d)
    assert list(d.state_dict()) == keys and list(_meta(conf).state_dict()) == keys, 'constructing Plan2Explore changed the Dreamer'
    assert p.dreamer is d and not [k for k in p.state_dict() if 'dreamer' in k or k.startswith('wm.')]
    assert not [n for n, _ in p.named_modules() if 'dreamer' in n]
    F_ = conf.deter_dim + conf.stoch_dim * conf.stoch_discrete
    Dt = conf.stoch_dim * conf.stoch_discrete
    in_dim = F_ + (conf.action_dim if cond else 0)
    assert len(p.heads) == K == p.K and (p.in_dim, p.target_dim) == (in_dim, Dt)
    for k, h in enumerate(p.heads):
        assert (h.in_dim, h.out_dim, h.hidden_dim, h.hidden_layers, h.layer_norm) == (in_dim, Dt, MLP_HIDDEN, 4, bool(conf.layer_norm))
        assert tuple(h.model[0].weight.shape) == (MLP_HIDDEN, in_dim) and tuple(h.model[12].weight.shape) == (Dt, MLP_HIDDEN)
        assert f'ensemble.heads.{k}.model.0.weight' in p.state_dict()
    assert isinstance(p.ac, ActorCritic) and p.ac is not d.ac
    assert [(n, tuple(v.shape)) for n, v in p.ac.state_dict().items()] == [(n, tuple(v.shape)) for n, v in d.ac.state_dict().items()]
    assert p.ac.sparse_cols == d.ac.sparse_cols and (p.ac.gamma, p.ac.lambda_, p.ac.entropy_weight) == (d.ac.gamma, d.ac.lambda_, d.ac.entropy_weight)
    assert max(EXPLORE_METRIC_SLOTS.values()) + 2 <= 48 and len(set(EXPLORE_METRIC_SLOTS.values())) == len(EXPLORE_METRIC_SLOTS)


def test_gaussian_latents_and_amp_build():
    from pydreamer_amd.explore import Plan2Explore
    from pydreamer_amd.models import MLP
    conf = config.load_config('defaults', 'atari', stoch_discrete=0, amp=True, disag_models=2)
    with torch.device('meta'):
        p = Plan2Explore(conf, _meta(conf))
    assert p.target_dim == conf.stoch_dim and p.in_dim == conf.deter_dim + conf.stoch_dim + conf.action_dim
    assert all(m.precision == 1 for m in p.modules() if isinstance(m, MLP))


def test_refusals_at_construction():
    from pydreamer_amd.explore import Plan2Explore
    conf = config.load_config('defaults', 'atari', iwae_samples=2)
    d = _meta(conf)
    with pytest.raises(NotImplementedError, match='iwae_samples'):
        Plan2Explore(conf, d)
    for K in (1, 17):
        with pytest.raises(ValueError, match='disag_models'):
            Plan2Explore(config.load_config('defaults', 'atari', disag_models=K), d)


def test_a_greedy_run_never_imports_explore(tmp_path, monkeypatch):
    """run() stops where it builds its optimizers (no device here) - behind the point where a plan2explore run imports the module."""
    from pydreamer_amd.train import run
    repo = R.LocalEpisodeRepository(str(tmp_path))
    conf = config.load_config('defaults', 'vectorenv', device='cpu')
    assert conf.expl_behavior == 'greedy'
    for name in [n for n in sys.modules if n == 'pydreamer_amd.explore']:
        monkeypatch.delitem(sys.modules, name)
    with pytest.raises(hip.DreamerHipError):
        run(conf, repo, logdir=str(tmp_path / 'log'))
    assert 'pydreamer_amd.explore' not in sys.modules
    with pytest.raises(ValueError, match='expl_behavior'):
        run(config.load_config('defaults', 'vectorenv', device='cpu', expl_behavior='random'), repo, logdir=str(tmp_path / 'log'))
    with pytest.raises(ValueError, match='plan2explore'):
        run(config.load_config('defaults', 'vectorenv', device='cpu', expl_behavior='plan2explore', model='gru_probe'), repo,
            logdir=str(tmp_path / 'log'))
    assert 'pydreamer_amd.explore' not in sys.modules
    with pytest.raises(hip.DreamerHipError):
        run(config.load_config('defaults', 'vectorenv', device='cpu', expl_behavior='plan2explore'), repo, logdir=str(tmp_path / 'log'))
    assert 'pydreamer_amd.explore' in sys.modules
