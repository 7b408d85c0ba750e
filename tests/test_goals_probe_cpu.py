"""CPU (-m "not gpu"): the host side of the goals probe (probe_model='goals' and 'map+goals'): the parameter trees against the
three reference-written fixtures, what is refused, the metric slots, the host-side argument checks of dm_goals_stats (nothing
is launched), and the goal fields of replay.preprocess_batch / ReplayFeed / DeviceReplay against a numpy restatement of
preprocessing.py:171-178."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_form_params as CFP                     # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402
from pydreamer_amd import config, hip, replay        # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
DM_E_SHAPE, DM_E_WORKSPACE, DM_E_NULL = -1, -2, -5
FIXTURES = ['tiny_goals_probe', 'tiny_goals_probe_iwae', 'tiny_map_goals_probe']
MLP_IDX = (0, 1, 3, 4, 6, 7, 9, 10, 12)              # Linear / LayerNorm slots of a 4-layer MLP


def _conf(g=None, **more):
    if g is None:
        g = np.load(os.path.join(GOLD, 'tiny_goals_probe.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    return config.load_config('defaults', 'atari', **{**vars(oconf), **extra, **more})


def _goal_keys(prefix):
    return [f'{prefix}decoders.{h}.model.model.{i}.{p}' for h in ('goal_direction', 'goals_direction') for i in MLP_IDX
            for p in ('weight', 'bias')]


@pytest.mark.parametrize('name', FIXTURES)
def test_state_dict_matches_the_reference(name):
    from pydreamer_amd.models import Dreamer, GoalsProbe, MapGoalsProbe
    g = np.load(os.path.join(GOLD, name + '.npz'))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    both = name == 'tiny_map_goals_probe'
    assert extra['goals_size'] == 3 and extra['probe_model'] == ('map+goals' if both else 'goals')
    with torch.device('meta'):
        model = Dreamer(_conf(g))
    want = CFP.shapes_of_fixture(g)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert list(got.items()) == list(want.items())
    probe = [k for k in got if k.startswith('probe_model.')]
    if both:
        assert isinstance(model.probe_model, MapGoalsProbe)
        map_keys = [f'probe_model.map_probe.decoder.model.{i}.{p}' for i in (0, 1, 3, 4, 6) for p in ('weight', 'bias')]
        assert probe == map_keys + _goal_keys('probe_model.goals_probe.')
        F_ = got['probe_model.goals_probe.decoders.goal_direction.model.model.0.weight'][1]
        assert got['probe_model.map_probe.decoder.model.0.weight'][1] == F_ + 4, 'only the map probe sees map_coord'
    else:
        assert isinstance(model.probe_model, GoalsProbe)
        assert probe == _goal_keys('probe_model.')
    pre = 'probe_model.goals_probe.' if both else 'probe_model.'
    assert got[pre + 'decoders.goal_direction.model.model.12.weight'] == (2, 400)
    assert got[pre + 'decoders.goals_direction.model.model.12.weight'] == (6, 400)
    groups = model.param_groups()
    assert [id(p) for p in groups['probe']] == [id(p) for p in model.probe_model.parameters()]
    assert len(groups['probe']) == len(probe) and not {id(p) for p in groups['probe']} & {id(p) for p in groups['wm']}


def test_layer_norm_and_depth_are_fixed_and_init_is_torch_default():
    """probes.py:94-95: hidden_layers=4, layer_norm=True whatever conf.layer_norm says; dreamer.py:283 applies init_weights_tf2 to
    the world model only, so the probe's biases are not zero."""
    from pydreamer_amd.models import Dreamer
    torch.manual_seed(0)
    model = Dreamer(_conf(layer_norm=False))
    for mlp in model.probe_model.heads():
        assert mlp.layer_norm and mlp.hidden_layers == 4 and mlp.hidden_dim == 400
    assert not model.wm.decoder.reward.model.layer_norm
    assert float(model.probe_model.decoders.goal_direction.model.model[0].bias.detach().abs().sum()) > 0


@pytest.mark.parametrize('kw', [dict(probe_model='goals', goals_size=0), dict(probe_model='map+goals', goals_size=0),
                                dict(probe_model='goals', probe_gradients=True),
                                dict(probe_model='map+goals', probe_gradients=True, map_size=5, map_channels=6)], ids=str)
def test_refused_values_raise(kw):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'), pytest.raises(NotImplementedError):
        Dreamer(_conf(**kw))


def test_metric_slots_and_config():
    from pydreamer_amd.models import Dreamer, GOALS_METRIC_SLOTS, METRIC_BUF_FLOATS, METRIC_SLOTS
    names = ['loss_goal_direction', 'loss_goals_direction', 'mse_goals', 'var_goals'] + [f'mse_goal_age{a}' for a in (0, 5, 10, 50, 200, 1000)]
    assert list(GOALS_METRIC_SLOTS) == names and list(GOALS_METRIC_SLOTS.values()) == list(range(32, 42))
    assert not set(GOALS_METRIC_SLOTS) & set(METRIC_SLOTS) and not set(GOALS_METRIC_SLOTS.values()) & set(METRIC_SLOTS.values())
    assert max(METRIC_SLOTS.values()) < min(GOALS_METRIC_SLOTS.values()) and max(GOALS_METRIC_SLOTS.values()) < METRIC_BUF_FLOATS == 48
    m = config.load_config('defaults', 'miniworld')
    assert (m.probe_model, m.goals_size) == ('none', 0)
    with torch.device('meta'):
        goals, none = Dreamer(_conf()), Dreamer(_conf(probe_model='none'))
    for model, has in ((goals, True), (none, False)):
        model.metric_buffer = torch.zeros(METRIC_BUF_FLOATS)
        got, _, idx = model.packed_metrics()
        assert got[:len(METRIC_SLOTS)] == list(METRIC_SLOTS)
        assert (got[len(METRIC_SLOTS):] == names) if has else (len(got) == len(METRIC_SLOTS))
        assert len(idx) == len(got) and max(idx) < METRIC_BUF_FLOATS


@pytest.mark.parametrize('kw,heads', [(dict(), 1), (dict(probe_model='map+goals', map_size=5, map_channels=6), 2),
                                      (dict(probe_model='map', map_size=5, map_channels=6), 1), (dict(probe_model='none'), 0)], ids=str)
def test_dist_attach_weights_every_probe_head(monkeypatch, kw, heads):
    """dist.attach(model=...) hands the shard weight B_r / B to every probe head - the goals probe, both heads of map+goals, the
    map probe - and marks the probe group as folded; NoProbeHead's group is weighted before the collective instead.  Host only:
    the process group is pretended, the optimizers are stand-ins."""
    from types import SimpleNamespace
    from pydreamer_amd import dist as D
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'):
        real = Dreamer(_conf(**kw))
    monkeypatch.setattr(D.dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(D.dist, 'get_world_size', lambda group=None: 2)
    opts = {k: SimpleNamespace(dp=None) for k in ('wm', 'probe', 'actor', 'critic')}
    model = SimpleNamespace(wm=SimpleNamespace(), ac=SimpleNamespace(), probe_model=real.probe_model, _opt=opts)
    D.attach(list(opts.values()), 1, 2, model=model)
    pm = real.probe_model
    got = [pm.map_probe, pm.goals_probe] if heads == 2 else [pm] if heads == 1 else []
    assert all(h.grad_weight == 0.5 for h in got) and opts['probe'].dp_folded == (heads > 0)
    assert heads > 0 or not hasattr(pm, 'grad_weight')
    assert model.wm.grad_weight == 0.5 and all(o.dp == (None, 0.5) for o in opts.values())


def _rc(name, *args):
    return getattr(hip.lib(), name)(*args)


def test_entry_point_is_bound_and_checks_arguments_on_the_host():
    """Nothing is launched: every pointer below is either NULL or a dummy that a launch would fault on."""
    lib = hip.lib()
    for n in ('dm_goals_stats', 'dm_goals_stats_ws_floats'):
        assert n in hip.exported_symbols() and hasattr(lib, n)
    P = 64      # a non-null placeholder; only calls that fail their checks (or have no rows) get it
    big = 1 << 30
    assert _rc('dm_goals_stats', 4, 3, None, P, None, P, P, big, None) == DM_E_NULL
    assert _rc('dm_goals_stats', 4, 3, P, None, None, P, P, big, None) == DM_E_NULL
    assert _rc('dm_goals_stats', 4, 3, P, P, None, None, P, big, None) == DM_E_NULL
    assert _rc('dm_goals_stats', 4, 3, P, P, P, P, None, big, None) == DM_E_NULL
    assert 'null' in lib.dm_last_error().decode()
    assert _rc('dm_goals_stats', -1, 3, P, P, None, P, P, big, None) == DM_E_SHAPE
    assert 'rows=-1' in lib.dm_last_error().decode()
    assert _rc('dm_goals_stats', 4, 0, P, P, None, P, P, big, None) == DM_E_SHAPE
    assert 'G=0' in lib.dm_last_error().decode()
    assert _rc('dm_goals_stats', 4, -2, P, P, P, P, P, big, None) == DM_E_SHAPE
    assert 'G=-2' in lib.dm_last_error().decode()
    need = int(lib.dm_goals_stats_ws_floats(2500, 6))
    assert need >= 40 * (13 + 24) and int(lib.dm_goals_stats_ws_floats(0, 6)) == 0
    assert _rc('dm_goals_stats', 2500, 6, P, P, None, P, P, 4 * need - 4, None) == DM_E_WORKSPACE
    with pytest.raises(hip.DreamerHipError):
        hip.call('dm_goals_stats', 4, 0, P, P, None, P, P, big, None)
    # zero rows: nothing to do, nothing launched (no workspace needed either)
    assert _rc('dm_goals_stats', 0, 3, P, P, None, P, None, 0, None) == 0
    assert _rc('dm_goals_stats', 0, 3, P, P, P, P, P, big, None) == 0


# ------------------------------------------------------------------------------------------------ the feeds
def _raw_batch(T=3, B=2, G=4, visage=True):
    rs = np.random.RandomState(3)
    d = dict(image=rs.randint(0, 256, (T, B, 8, 8, 3)).astype(np.uint8), action=rs.randint(0, 4, (T, B)),
             reward=rs.randn(T, B), terminal=np.zeros((T, B)), reset=np.zeros((T, B), bool),
             targets_vec=rs.randn(T, B, G, 2), target_vec=rs.randn(T, B, 2))
    if visage:
        d['goals_visage'] = rs.randint(0, 300, (T, B, G))
    return d


def test_preprocess_batch_goal_fields():
    T, B, G = 3, 2, 4
    raw = _raw_batch(T, B, G)
    plain = replay.preprocess_batch(dict(raw), 4, 'tanh')
    assert set(plain) == {'image', 'action', 'terminal', 'reward', 'reset'}, 'without goals=True nothing new is emitted'
    off = replay.preprocess_batch(dict(raw), 4, 'tanh', goals=False)
    assert list(off) == list(plain) and all(off[k].dtype == plain[k].dtype and np.array_equal(off[k], plain[k]) for k in plain)
    out = replay.preprocess_batch(dict(raw), 4, 'tanh', goals=True)
    for k in plain:
        assert out[k].dtype == plain[k].dtype and np.array_equal(out[k], plain[k]), k
    want = np.zeros((T, B, 2 * G), np.float32)      # preprocessing.py:173-176: (*,G,2) => (*,2G)
    for g in range(G):
        want[..., 2 * g], want[..., 2 * g + 1] = raw['targets_vec'][..., g, 0], raw['targets_vec'][..., g, 1]
    assert out['goals_direction'].dtype == np.float32 and np.array_equal(out['goals_direction'], want)
    assert out['goal_direction'].dtype == np.float32 and np.array_equal(out['goal_direction'], raw['target_vec'].astype(np.float32))
    assert out['goals_visage'].dtype == np.float32 and np.array_equal(out['goals_visage'], raw['goals_visage'].astype(np.float32))
    assert set(out) == set(plain) | {'goals_direction', 'goal_direction', 'goals_visage'}
    assert 'goals_visage' not in replay.preprocess_batch(_raw_batch(visage=False), 4, goals=True)
    for gone in ('targets_vec', 'target_vec'):
        with pytest.raises(ValueError, match=gone):
            replay.preprocess_batch({k: v for k, v in raw.items() if k != gone}, 4, goals=True)


def _episode(n, ep, rs, G=3, visage=True, goals=True):
    d = dict(image=rs.randint(0, 256, (n, 8, 8, 3)).astype(np.uint8), action=rs.randint(0, 3, n),
             reward=(ep * 1000 + np.arange(n)).astype(np.float32), terminal=np.zeros(n, bool), reset=np.zeros(n, bool))
    if goals:
        d.update(targets_vec=rs.randn(n, G, 2), target_vec=rs.randn(n, 2).astype(np.float32))
    if visage:
        d['goals_visage'] = rs.randint(0, 1200, (n, G))
    return d


@pytest.mark.parametrize('visage', [True, False])
def test_goal_fields_of_both_feeds(tmp_path, visage):
    """ReplayFeed's slot and the batch DeviceReplay's plan describes (assembled byte-wise from its tables, as the gather does) both
    equal preprocess_batch(goals=True) of the identically seeded plain reader; goals=False leaves both feeds as they are."""
    from test_device_replay_cpu import _gather
    rs = np.random.RandomState(2)
    repo = replay.LocalEpisodeRepository(str(tmp_path))
    for ep, n in enumerate([19, 26, 33]):
        repo.save_data(_episode(n, ep + 1, rs, visage=visage), ep, ep)
    kw = dict(batch_length=6, batch_size=3, allow_mid_reset=True, reset_interval=8, seed=3)
    new = {'goals_direction', 'goal_direction'} | ({'goals_visage'} if visage else set())
    plain = iter(replay.SequentialReplay(repo, **kw))
    dr = replay.DeviceReplay(replay.SequentialReplay(repo, **kw), 3, clip_rewards='log1p', goals=True)
    feed = replay.ReplayFeed(replay.SequentialReplay(repo, **kw), 3, clip_rewards='log1p', goals=True)
    off = replay.ReplayFeed(replay.SequentialReplay(repo, **kw), 3, clip_rewards='log1p')
    assert dr.spec() == feed.spec() and set(feed.spec()) - set(off.spec()) == new
    assert {k: v for k, v in feed.spec().items() if k not in new} == off.spec()
    assert replay.DeviceReplay(replay.SequentialReplay(repo, **kw), 3, clip_rewards='log1p').spec() == off.spec()
    assert feed.spec()['goals_direction'] == ((6, 3, 6), np.float32) and feed.spec()['goal_direction'] == ((6, 3, 2), np.float32)
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in feed.spec().items()}
    slot_off = {k: np.zeros(shape, dt) for k, (shape, dt) in off.spec().items()}
    for i in range(7):
        want = replay.preprocess_batch(next(plain), 3, 'log1p', goals=True)
        got_feed, got_dr, got_off = feed.fill(slot), _gather(dr, dr.plan()), off.fill(slot_off)
        for k in new:
            for got in (got_feed, got_dr):
                assert got[k].dtype == np.float32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (i, k)
        for k in got_off:
            assert np.array_equal(got_off[k], got_feed[k]) and np.array_equal(got_off[k], got_dr[k]), (i, k)


def test_feeds_without_goal_sources_raise_at_construction(tmp_path):
    rs = np.random.RandomState(4)
    repo = replay.LocalEpisodeRepository(str(tmp_path))
    for ep, n in enumerate([19, 26]):
        repo.save_data(_episode(n, ep + 1, rs, goals=False), ep, ep)
    kw = dict(batch_length=6, batch_size=2, seed=3)
    with pytest.raises(ValueError, match='targets_vec'):
        replay.ReplayFeed(replay.SequentialReplay(repo, **kw), 3, goals=True)
    with pytest.raises(ValueError, match='targets_vec'):
        replay.DeviceReplay(replay.SequentialReplay(repo, **kw), 3, goals=True)
    replay.ReplayFeed(replay.SequentialReplay(repo, **kw), 3)
