"""CPU (-m "not gpu"): the host side of the map probe (probe_model='map'): the parameter tree against the reference-written
fixture, what is still refused, the config keys, the C-ABI's host-side argument checks, and the map fields of
replay.preprocess_batch against a numpy restatement of preprocessing.py:115-131,152-158."""
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
DM_E_SHAPE, DM_E_NULL = -1, -5


def _conf(g=None, **more):
    if g is None:
        g = np.load(os.path.join(GOLD, 'tiny_map_probe.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    return config.load_config('defaults', 'atari', **{**vars(oconf), **extra, **more})


@pytest.mark.parametrize('name', ['tiny_map_probe', 'tiny_map_probe_iwae'])
def test_state_dict_matches_the_reference(name):
    from pydreamer_amd.models import Dreamer, MapProbeHead
    g = np.load(os.path.join(GOLD, name + '.npz'))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    assert extra == dict(probe_model='map', map_size=5, map_channels=6, map_hidden_dim=128, map_hidden_layers=2)
    with torch.device('meta'):
        model = Dreamer(_conf(g))
    want = CFP.shapes_of_fixture(g)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert list(got.items()) == list(want.items())
    probe = [k for k in got if k.startswith('probe_model.')]
    assert probe == [f'probe_model.decoder.model.{i}.{p}' for i in (0, 1, 3, 4, 6) for p in ('weight', 'bias')]
    assert isinstance(model.probe_model, MapProbeHead)
    groups = model.param_groups()
    assert [id(p) for p in groups['probe']] == [id(p) for p in model.probe_model.decoder.parameters()]
    assert len(groups['probe']) == 10 and not {id(p) for p in groups['probe']} & {id(p) for p in groups['wm']}


def test_probe_keeps_torch_default_linear_init():
    """dreamer.py:283 applies init_weights_tf2 to the world model only: the probe's biases are NOT zero."""
    from pydreamer_amd.models import Dreamer
    torch.manual_seed(0)
    model = Dreamer(_conf())
    assert float(model.probe_model.decoder.model[0].bias.detach().abs().sum()) > 0
    assert float(model.wm.decoder.reward.model.model[0].bias.detach().abs().sum()) == 0


@pytest.mark.parametrize('kw', [dict(probe_model='map+goals'), dict(probe_model='goals'), dict(map_decoder='cnn'),
                                dict(probe_gradients=True), dict(map_hidden_layers=0)], ids=str)
def test_still_refused_values_raise(kw):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'), pytest.raises(NotImplementedError):
        Dreamer(_conf(**kw))


@pytest.mark.parametrize('kw', [dict(map_size=0), dict(map_channels=0)], ids=str)
def test_degenerate_map_shapes_raise(kw):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'), pytest.raises(ValueError):
        Dreamer(_conf(**kw))


def test_none_is_unchanged_and_config_keys():
    from pydreamer_amd.models import Dreamer, NoProbeHead, METRIC_SLOTS, METRIC_BUF_FLOATS
    with torch.device('meta'):
        model = Dreamer(_conf(probe_model='none'))
    assert isinstance(model.probe_model, NoProbeHead) and [k for k in model.state_dict() if k.startswith('probe_model.')] == ['probe_model.dummy']
    d = config.load_config('defaults')
    assert (d.map_key, d.map_size, d.map_channels, d.map_categorical, d.goals_size, d.map_decoder, d.map_hidden_layers,
            d.map_hidden_dim) == (None, 0, 0, True, 0, 'dense', 4, 1024)
    m = config.load_config('defaults', 'miniworld')
    assert (m.map_key, m.map_size, m.map_channels, m.probe_model) == ('map', 9, 14, 'none')
    slots = [METRIC_SLOTS[k] for k in ('loss_map', 'acc_map', 'acc_map_seen')]
    assert len(set(METRIC_SLOTS.values())) == len(METRIC_SLOTS) and max(METRIC_SLOTS.values()) < METRIC_BUF_FLOATS
    assert min(slots) > max(v for k, v in METRIC_SLOTS.items() if k not in ('loss_map', 'acc_map', 'acc_map_seen')), 'appended'


def _rc(name, *args):
    return getattr(hip.lib(), name)(*args)


def test_entry_points_are_bound_and_check_arguments_on_the_host():
    """Nothing is launched: every pointer below is either NULL or a dummy that a launch would fault on."""
    lib = hip.lib()
    for n in ('dm_cat_target_index', 'dm_cat_image_loss', 'dm_cat_image_pred', 'dm_cat_concat_rows'):
        assert n in hip.exported_symbols() and hasattr(lib, n)
    P = 64      # a non-null placeholder; only calls that fail their checks get it
    # null required pointers
    assert _rc('dm_cat_target_index', 4, 3, 5, None, P, None) == DM_E_NULL
    assert _rc('dm_cat_target_index', 4, 3, 5, P, None, None) == DM_E_NULL
    assert _rc('dm_cat_image_loss', 4, 1, 3, 5, None, 15, P, P, None, None) == DM_E_NULL
    assert _rc('dm_cat_image_loss', 4, 1, 3, 5, P, 15, None, P, None, None) == DM_E_NULL
    assert _rc('dm_cat_image_loss', 4, 1, 3, 5, P, 15, P, None, None, None) == DM_E_NULL
    assert 'null' in lib.dm_last_error().decode()
    assert _rc('dm_cat_image_pred', 4, 1, 3, 5, None, 15, P, None, None, P, None, None) == DM_E_NULL
    assert _rc('dm_cat_image_pred', 4, 1, 3, 5, P, 15, None, None, None, P, None, None) == DM_E_NULL
    assert _rc('dm_cat_image_pred', 4, 1, 3, 5, P, 15, P, None, None, None, None, None) == DM_E_NULL
    assert _rc('dm_cat_image_pred', 4, 1, 3, 5, P, 15, P, None, None, P, P, None) == DM_E_NULL      # acc_seen without seen
    # shapes
    assert _rc('dm_cat_target_index', 4, 0, 5, P, P, None) == DM_E_SHAPE
    assert _rc('dm_cat_target_index', 4, 3, 0, P, P, None) == DM_E_SHAPE
    for C, cells, I, rows, ld in ((0, 5, 1, 4, 15), (3, 0, 1, 4, 15), (3, 5, 0, 4, 15), (3, 5, 3, 4, 15), (3, 5, 1, 4, 14)):
        assert _rc('dm_cat_image_loss', rows, I, C, cells, P, ld, P, P, None, None) == DM_E_SHAPE, (C, cells, I, rows, ld)
    for C, cells, I, ld in ((0, 5, 1, 15), (3, 0, 1, 15), (3, 5, 0, 15), (3, 5, 1, 14)):
        assert _rc('dm_cat_image_pred', 4, I, C, cells, P, ld, P, None, None, P, None, None) == DM_E_SHAPE, (C, cells, I, ld)
    assert 'ld=14' in lib.dm_last_error().decode()
    with pytest.raises(hip.DreamerHipError):
        hip.call('dm_cat_image_loss', 4, 3, 3, 5, P, 15, P, P, None, None)
    # zero rows: nothing to do, nothing launched
    assert _rc('dm_cat_image_loss', 0, 1, 3, 5, P, 15, P, P, None, None) == 0


def _raw_batch(T=3, B=2, S=4, C=5):
    rs = np.random.RandomState(3)
    return dict(image=rs.randint(0, 256, (T, B, 8, 8, 3)).astype(np.uint8), action=rs.randint(0, 4, (T, B)),
                reward=rs.randn(T, B), terminal=np.zeros((T, B)), reset=np.zeros((T, B), bool),
                map=rs.randint(0, C, (T, B, S, S)), map_seen=rs.randint(0, 3, (T, B, S, S)),
                map_vis=rs.randint(400, 600, (T, B, S, S)), agent_pos=rs.rand(T, B, 2) * S, agent_dir=rs.randn(T, B, 2))


def test_preprocess_batch_map_fields():
    T, B, S, C = 3, 2, 4, 5
    raw = _raw_batch(T, B, S, C)
    plain = replay.preprocess_batch(dict(raw), 4, 'tanh')
    assert set(plain) == {'image', 'action', 'terminal', 'reward', 'reset'}, 'without the map keywords nothing new is emitted'
    out = replay.preprocess_batch(dict(raw), 4, 'tanh', map_key='map', map_categorical=C)
    for k in plain:
        assert out[k].dtype == plain[k].dtype and np.array_equal(out[k], plain[k]), k
    want = np.zeros((T, B, C, S, S), np.float32)
    for t in range(T):
        for b in range(B):
            for y in range(S):
                for x in range(S):
                    want[t, b, raw['map'][t, b, y, x], y, x] = 1.0
    assert out['map'].dtype == np.float32 and out['map'].flags['C_CONTIGUOUS'] and np.array_equal(out['map'], want)
    assert np.array_equal(out['map_seen_mask'], (raw['map_seen'] > 0).astype(int)) and out['map_seen_mask'].shape == (T, B, S, S)
    coord = np.concatenate([raw['agent_pos'] / float(S) * 2 - 1.0, raw['agent_dir']], -1).astype(np.float32)
    assert out['map_coord'].dtype == np.float32 and out['map_coord'].shape == (T, B, 4) and np.array_equal(out['map_coord'], coord)
    # map_vis when there is no map_seen; no agent pose: no map_coord
    raw2 = {k: v for k, v in raw.items() if k not in ('map_seen', 'agent_dir')}
    out2 = replay.preprocess_batch(raw2, 4, 'tanh', map_key='map', map_categorical=C)
    assert np.array_equal(out2['map_seen_mask'], (raw['map_vis'] < 500).astype(int)) and 'map_coord' not in out2
    # a float (T,B,H,W,C) image under map_key, not categorical: to_image
    img = np.random.RandomState(5).randint(0, 256, (T, B, S, S, 3)).astype(np.uint8)
    out3 = replay.preprocess_batch(dict(raw, top=img), 4, map_key='top')
    assert np.array_equal(out3['map'], (img.astype(np.float32) / 255.0 - 0.5).transpose(0, 1, 4, 2, 3))
