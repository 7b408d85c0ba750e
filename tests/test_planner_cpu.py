"""CPU (-m "not gpu"): the host side of latent-space planning - CEMPlanner and PlannerPolicy are exported, the two
entry points of csrc/cem.hip are declared and bound and refuse bad arguments on the host with nothing launched, the plan_* config
keys are inert by default, the planner refuses sizes outside the kernels' bounds at construction, and a run() with the default
eval_behavior never imports the module."""
import os
import re
import sys

import pytest
import torch

from pydreamer_amd import config, hip, replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DM_E_SHAPE, DM_E_NULL = -1, -5
P = 64      # a placeholder pointer a launch would fault on


def _rc(name, *args):
    return getattr(hip.lib(), name)(*args)


def _err():
    return hip.lib().dm_last_error().decode()


def _meta(conf):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'):
        return Dreamer(conf)


def test_symbols_are_exported_declared_and_bound():
    import pydreamer_amd
    from pydreamer_amd import planner
    assert pydreamer_amd.CEMPlanner is planner.CEMPlanner and pydreamer_amd.PlannerPolicy is planner.PlannerPolicy
    from pydreamer_amd.policy import CarriedStatePolicy, NetworkPolicy
    assert issubclass(planner.PlannerPolicy, CarriedStatePolicy) and issubclass(NetworkPolicy, CarriedStatePolicy)
    assert planner.PlannerPolicy.reset_state is NetworkPolicy.reset_state, 'the carried-state code is shared, not copied'
    hdr = open(os.path.join(ROOT, 'include', 'dreamer_hip.h')).read()
    declared = set(re.findall(r'\b(dm_[a-z0-9_]+)\s*\(', hdr))
    lib = hip.lib()
    for n in ('dm_cem_draw', 'dm_cem_update'):
        assert n in declared and n in hip.exported_symbols() and hasattr(lib, n), n
    assert lib.dm_version() == hip.DM_ABI_VERSION == 17
    assert os.path.exists(os.path.join(ROOT, 'pydreamer_amd', 'csrc', 'cem.hip'))


def test_cem_draw_checks_arguments_on_the_host():
    """dm_cem_draw(kind, B, J, Hp, A, prop, noise, actions, act_idx, stream): every failing call returns before a launch."""
    ok = dict(kind=0, B=2, J=5, Hp=3, A=4, prop=P, noise=P, actions=P, act_idx=P, stream=None)
    call = lambda **kw: _rc('dm_cem_draw', *{**ok, **kw}.values())
    for kind in (-1, 3):
        assert call(kind=kind) == DM_E_SHAPE and f'kind {kind}' in _err()
    for B in (0, -1):
        assert call(B=B) == DM_E_SHAPE and f'B={B}' in _err()
    for J in (0, -2, 1025):
        assert call(J=J) == DM_E_SHAPE and f'J={J}' in _err()
    for Hp in (0, 65):
        assert call(Hp=Hp) == DM_E_SHAPE and f'Hp={Hp}' in _err()
    for A in (0, 65):
        assert call(A=A) == DM_E_SHAPE and f'A={A}' in _err()
    assert call(B=1 << 30, J=1024) == DM_E_SHAPE and 'rows' in _err()
    for gone in ('prop', 'noise', 'actions'):
        assert call(**{gone: None}) == DM_E_NULL and 'null' in _err() and 'cem_draw' in _err(), gone
    assert call(act_idx=None) == DM_E_NULL and 'act_idx' in _err()      # kind 0 writes it
    with pytest.raises(hip.DreamerHipError, match='cem_draw'):
        hip.call('dm_cem_draw', 1, 2, 5, 3, 4, None, P, P, None, None)


def test_cem_update_checks_arguments_on_the_host():
    """dm_cem_update(kind, B, J, K, Hp, A, gamma, reward, terminal, value, actions, act_idx, prop_in, alpha, floor, prop_out, ret,
    elite, first_action, stats, stream)."""
    ok = dict(kind=0, B=2, J=5, K=2, Hp=3, A=4, gamma=0.99, reward=P, terminal=P, value=P, actions=P, act_idx=P, prop_in=P, alpha=0.0,
              floor=0.01, prop_out=P, ret=P, elite=P, first_action=P, stats=P, stream=None)
    call = lambda **kw: _rc('dm_cem_update', *{**ok, **kw}.values())
    assert call(kind=3) == DM_E_SHAPE and 'kind 3' in _err()
    assert call(B=0) == DM_E_SHAPE and call(J=1025, K=3) == DM_E_SHAPE and call(Hp=65) == DM_E_SHAPE and call(A=65) == DM_E_SHAPE
    for K in (0, -1, 6):
        assert call(K=K) == DM_E_SHAPE and f'K={K}' in _err()
    for alpha in (-0.1, 1.5, float('nan')):
        assert call(alpha=alpha) == DM_E_SHAPE and 'alpha' in _err()
    for floor in (-1.0, 1.5, float('nan')):
        assert call(floor=floor) == DM_E_SHAPE and 'floor' in _err()
    assert call(gamma=float('inf')) == DM_E_SHAPE and 'gamma' in _err()
    for gone in ('reward', 'terminal', 'actions', 'prop_in', 'prop_out', 'ret', 'elite', 'first_action', 'stats'):
        assert call(**{gone: None}) == DM_E_NULL and 'cem_update' in _err(), gone
    assert call(act_idx=None) == DM_E_NULL and 'act_idx' in _err()
    with pytest.raises(hip.DreamerHipError, match='cem_update'):
        hip.call('dm_cem_update', 1, 2, 5, 6, 3, 4, 0.99, P, P, None, P, None, P, 0.0, 0.1, P, P, P, P, P, None)


def test_config_defaults_and_overrides():
    want = dict(plan_horizon=12, plan_candidates=1000, plan_elites=100, plan_iters=10, plan_alpha=0.0, plan_floor=0.01, plan_value=True,
                eval_behavior='actor')
    for sections in (('defaults',), ('defaults', 'atari'), ('defaults', 'dmc'), ('defaults', 'vectorenv')):
        c = config.load_config(*sections)
        assert {k: getattr(c, k) for k in want} == want, sections
    c = config.load_config('defaults', 'atari', plan_candidates=64, plan_elites=8, eval_behavior='plan')
    assert (c.plan_candidates, c.plan_elites, c.eval_behavior) == (64, 8, 'plan')
    from pydreamer_amd.planner import CEMPlanner
    p = CEMPlanner(_meta(c))
    assert (p.horizon, p.candidates, p.elites, p.iters, p.alpha, p.floor, p.use_value) == (12, 64, 8, 10, 0.0, 0.01, True)
    p = CEMPlanner(_meta(c), horizon=3, iters=2, use_value=False)
    assert (p.horizon, p.candidates, p.iters, p.use_value) == (3, 64, 2, False)


@pytest.mark.parametrize('bad', [dict(candidates=1025), dict(candidates=0), dict(candidates=8, elites=9), dict(elites=0),
                                 dict(elites=-1), dict(horizon=65), dict(horizon=0), dict(iters=0), dict(alpha=1.5), dict(floor=-0.1)])
def test_refusals_at_construction(bad):
    from pydreamer_amd.planner import CEMPlanner, PlannerPolicy
    d = _meta(config.load_config('defaults', 'atari'))
    with pytest.raises(ValueError, match=next(iter(bad))):
        CEMPlanner(d, **bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        PlannerPolicy(d, lambda obs: obs, batch_size=2, device='meta', **bad)
    with pytest.raises(ValueError, match=next(iter(bad))):      # ... and from the config keys
        CEMPlanner(_meta(config.load_config('defaults', 'atari', **{'plan_' + k: v for k, v in bad.items()})))


def test_the_default_run_never_imports_the_planner(tmp_path, monkeypatch):
    """run() stops where it builds its optimizers (no device here) - behind the point where eval_behavior='plan' imports the module."""
    from pydreamer_amd.train import run
    repo = R.LocalEpisodeRepository(str(tmp_path))
    conf = config.load_config('defaults', 'vectorenv', device='cpu')
    for name in [n for n in sys.modules if n == 'pydreamer_amd.planner']:
        monkeypatch.delitem(sys.modules, name)
    with pytest.raises(hip.DreamerHipError):
        run(conf, repo, logdir=str(tmp_path / 'log'))
    assert 'pydreamer_amd.planner' not in sys.modules
    with pytest.raises(ValueError, match='eval_behavior'):
        run(config.load_config('defaults', 'vectorenv', device='cpu', eval_behavior='mpc'), repo, logdir=str(tmp_path / 'log'))
    with pytest.raises(ValueError, match="eval_behavior='plan'"):
        run(config.load_config('defaults', 'vectorenv', device='cpu', eval_behavior='plan', model='gru_probe'), repo,
            logdir=str(tmp_path / 'log'))
    assert 'pydreamer_amd.planner' not in sys.modules
    with pytest.raises(hip.DreamerHipError):
        run(config.load_config('defaults', 'vectorenv', device='cpu', eval_behavior='plan'), repo, logdir=str(tmp_path / 'log'))
    assert 'pydreamer_amd.planner' in sys.modules
