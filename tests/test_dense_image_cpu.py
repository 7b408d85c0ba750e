"""CPU side of the dense categorical image path (the `minigrid` section): construction on `meta`, the reference's
state_dict layout as the fixtures of scripts/gen_minigrid_golden.py record it, the gate, the config section, the replay's
one-hot image, the new symbols' host-side argument checks, and the reference's own float32-vs-float64 deviation against the
bars of tests/test_gpu_minigrid.py."""
import ast
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_form_params as CFP                     # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402
from pydreamer_amd import config                     # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
FIXTURES = ['tiny_minigrid', 'tiny_minigrid_minprob', 'tiny_minigrid_eval', 'tiny_minigrid_inference']
NEW_SYMBOLS = ['dm_dense_image_rows', 'dm_elu_rows_fwd', 'dm_elu_rows_bwd', 'dm_cat_image_loss_mix']
TINY = dict(deter_dim=64, hidden_dim=64, stoch_dim=8, stoch_discrete=8, batch_length=5, batch_size=3, imag_horizon=4)


def _conf(**kw):
    return config.load_config('defaults', 'minigrid', **{**TINY, **kw})


def _fixture_conf(g):
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    return config.load_config('defaults', 'minigrid', **{**vars(oconf), **dict(ast.literal_eval(str(g['extra_conf_json'])))})


def _meta(conf):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'):
        return Dreamer(conf)


def test_minigrid_section_constructs():
    c = config.load_config('defaults', 'minigrid')
    assert (c.image_size, c.image_channels, c.image_categorical, c.map_key, c.map_size, c.map_channels, c.map_categorical) == \
        (7, 4, True, 'map', 11, 4, True)
    assert (c.action_dim, c.reward_input, c.image_encoder, c.image_encoder_layers, c.image_decoder, c.image_decoder_layers,
            c.probe_model, c.imag_horizon) == (7, True, 'dense', 3, 'dense', 2, 'map', 1)
    assert set(config.SECTIONS['minigrid']) <= set(config.SECTIONS['defaults'])
    m = _meta(_conf())
    assert m.wm.dense and m.wm.encoder.out_dim == 256
    sd = m.state_dict()
    assert tuple(sd['wm.encoder.encoder_image.model.1.weight'].shape) == (400, 294)          # 7 * 7 * (4 + 2)
    assert tuple(sd['wm.encoder.encoder_image.model.10.weight'].shape) == (256, 400)
    assert tuple(sd['wm.decoder.image.model.6.weight'].shape) == (196, 400)
    assert [k for k in sd if k.startswith('wm.encoder.encoder_image.')] == \
        [f'wm.encoder.encoder_image.model.{i}.{n}' for i in (1, 2, 4, 5, 7, 8, 10) for n in ('weight', 'bias')]
    assert [k for k in sd if k.startswith('wm.decoder.image.')] == \
        [f'wm.decoder.image.model.{i}.{n}' for i in (0, 1, 3, 4, 6) for n in ('weight', 'bias')]
    full = _meta(config.load_config('defaults', 'minigrid'))          # the section as it stands (map 11 x 11, deter 2048)
    assert tuple(full.state_dict()['wm.decoder.image.model.0.weight'].shape) == (400, 2048 + 32 * 32)


@pytest.mark.parametrize('name', FIXTURES)
def test_state_dict_equals_the_reference(name):
    g = np.load(os.path.join(GOLD, name + '.npz'))
    sd = _meta(_fixture_conf(g)).state_dict()
    shapes = CFP.shapes_of_fixture(g)
    assert list(sd.keys()) == list(shapes.keys())
    assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for s in shapes.values()]


def test_layer_norm_off_and_layer_counts():
    sd = _meta(_conf(layer_norm=False, image_encoder_layers=1, image_decoder_layers=7)).state_dict()
    assert [k for k in sd if k.startswith('wm.encoder.encoder_image.')] == \
        [f'wm.encoder.encoder_image.model.{i}.{n}' for i in (1, 4) for n in ('weight', 'bias')]
    assert [k for k in sd if k.startswith('wm.decoder.image.') and k.endswith('weight')] == \
        [f'wm.decoder.image.model.{3 * i}.weight' for i in range(8)]


@pytest.mark.parametrize('kw', [
    dict(image_decoder='cnn'), dict(image_encoder='cnn'), dict(image_categorical=False), dict(image_size=64), dict(image_size=17),
    dict(vecobs_size=5), dict(amp=True), dict(image_encoder_layers=0), dict(image_decoder_layers=0), dict(image_encoder_layers=8),
    dict(image_decoder_layers=8), dict(image_channels=1), dict(image_decoder_min_prob=1.0), dict(image_size=32),
    dict(image_encoder=None), dict(reward_decoder_categorical=[-1.0, 0.0, 1.0]), dict(actor_grad='dynamics'),
], ids=lambda kw: ','.join(f'{k}={v}' for k, v in kw.items()))
def test_outside_the_gate_raises(kw):
    with pytest.raises(NotImplementedError) as e:
        _meta(_conf(**kw))
    if not {'reward_decoder_categorical', 'actor_grad'} & set(kw):
        assert 'gate' in str(e.value)


@pytest.mark.parametrize('kw', [dict(image_size=16), dict(image_size=1), dict(image_channels=2), dict(reward_input=False),
                                dict(image_decoder_min_prob=0.05), dict(probe_model='none'), dict(layer_norm=False),
                                dict(probe_model='map+goals', goals_size=3)],
                         ids=lambda kw: ','.join(f'{k}={v}' for k, v in kw.items()))
def test_inside_the_gate_constructs(kw):
    m = _meta(_conf(**kw))
    S, C = m.conf.image_size, m.conf.image_channels
    assert m.wm.encoder.encoder_image.in_dim == S * S * (C + (2 if m.conf.reward_input else 0))
    assert m.wm.decoder.image.out_dim == S * S * C


def test_iwae_is_refused_before_any_device_is_touched():
    from pydreamer_amd.models import Dreamer
    m = Dreamer(_conf(probe_model='none'))            # real CPU parameters: a launch would fail with DreamerHipError instead
    T, B = 5, 3
    obs = dict(image=torch.zeros(T, B, 4, 7, 7), action=torch.zeros(T, B, 7), reward=torch.zeros(T, B), terminal=torch.zeros(T, B),
               reset=torch.zeros(T, B, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match='iwae_samples'):
        m.training_step(obs, m.init_state(B * 2), iwae_samples=2)
    with pytest.raises(NotImplementedError, match='iwae_samples'):
        m.wm.training_step(obs, m.init_state(B * 2), iwae_samples=2)
    assert not hasattr(m, 'metric_buffer')
    m2 = Dreamer(_conf(probe_model='none', iwae_samples=2))
    with pytest.raises(NotImplementedError, match='iwae_samples'):
        m2.training_step(obs, m2.init_state(B * 2))


def test_preprocess_batch_image_categorical():
    from pydreamer_amd.replay import preprocess_batch
    rs = np.random.RandomState(0)
    T, B, S, C = 3, 2, 7, 4
    classes = rs.randint(0, C, (T, B, S, S)).astype(np.uint8)
    batch = dict(image=classes, action=rs.randint(0, 7, (T, B)), reward=rs.randn(T, B), terminal=np.zeros((T, B)), reset=np.zeros((T, B), bool))
    out = preprocess_batch(batch, 7, image_categorical=C)
    # img_to_onehot (preprocessing.py:10-18): np.eye(C, dtype=float32)[x].transpose(0, 1, 4, 2, 3)
    want = np.zeros((T, B, C, S, S), np.float32)
    for c in range(C):
        want[:, :, c] = classes == c
    assert out['image'].dtype == np.float32 and out['image'].shape == (T, B, C, S, S) and np.array_equal(out['image'], want)
    assert out['image'].flags['C_CONTIGUOUS']
    # the default path: uint8 frames as they are, and still an assertion for anything else
    frames = rs.randint(0, 256, (T, B, 8, 8, 3)).astype(np.uint8)
    plain = preprocess_batch(dict(batch, image=frames), 7)
    assert plain['image'].dtype == np.uint8 and np.array_equal(plain['image'], frames)
    with pytest.raises(AssertionError):
        preprocess_batch(batch, 7)
    for k in ('action', 'reward', 'terminal', 'reset'):
        assert np.array_equal(out[k], plain[k])


def test_new_symbols_and_host_side_argument_checks(hip):
    assert set(NEW_SYMBOLS) <= set(hip.exported_symbols())
    lib = hip.lib()
    assert lib.dm_version() == 17 and hip.DM_ABI_VERSION == 17
    from pydreamer_amd.models import METRIC_BUF_FLOATS, METRIC_SLOTS
    assert METRIC_BUF_FLOATS == 48 and METRIC_SLOTS['loss_image'] == 1
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its host-side checks
    DM_E_SHAPE, DM_E_NULL = -1, -5

    def rows(rows=3, C=4, cells=49, img=fake, cls=None, r=fake, t=fake, out=fake, ldo=294):
        return lib.dm_dense_image_rows(rows, C, cells, img, cls, r, t, out, ldo, None)
    for kw in (dict(img=None), dict(cls=fake), dict(out=None), dict(r=None), dict(t=None)):      # none or both sources; half the planes
        assert rows(**kw) == DM_E_NULL, kw
        assert lib.dm_last_error()
    for kw in (dict(rows=-1), dict(C=0), dict(cells=0), dict(ldo=293), dict(r=None, t=None, ldo=195)):
        assert rows(**kw) == DM_E_SHAPE, kw
    assert rows(rows=0) == 0 and rows(rows=0, r=None, t=None, ldo=196) == 0          # nothing to do, nothing launched

    def elu_f(rows=3, n=256, x=fake, ldx=256, y=fake, ldy=256):
        return lib.dm_elu_rows_fwd(rows, n, x, ldx, y, ldy, None)

    def elu_b(rows=3, n=256, y=fake, ldy=256, dy=fake, lddy=256, dx=fake, lddx=256):
        return lib.dm_elu_rows_bwd(rows, n, y, ldy, dy, lddy, dx, lddx, None)
    for kw in (dict(x=None), dict(y=None)):
        assert elu_f(**kw) == DM_E_NULL, kw
    for kw in (dict(y=None), dict(dy=None), dict(dx=None)):
        assert elu_b(**kw) == DM_E_NULL, kw
    for kw in (dict(rows=-1), dict(n=0), dict(ldx=255), dict(ldy=255)):
        assert elu_f(**kw) == DM_E_SHAPE, kw
    for kw in (dict(rows=-1), dict(n=0), dict(ldy=255), dict(lddy=255), dict(lddx=255)):
        assert elu_b(**kw) == DM_E_SHAPE, kw
    assert elu_f(rows=0) == 0 and elu_b(rows=0) == 0

    def mix(rows=6, I=1, C=4, cells=49, x=fake, ld=196, tg=fake, m=0.05, loss=fake, d=fake):
        return lib.dm_cat_image_loss_mix(rows, I, C, cells, x, ld, tg, m, loss, d, None)
    for kw in (dict(x=None), dict(tg=None), dict(loss=None)):
        assert mix(**kw) == DM_E_NULL, kw
    for kw in (dict(rows=-1), dict(C=0), dict(cells=0), dict(I=0), dict(rows=7, I=2), dict(ld=195), dict(m=0.0), dict(m=1.0), dict(m=-0.1)):
        assert mix(**kw) == DM_E_SHAPE, kw
        assert lib.dm_last_error()
    assert mix(rows=0) == 0 and mix(rows=0, d=None) == 0


@pytest.mark.parametrize('name', FIXTURES)
def test_the_reference_alone_is_far_inside_the_bars(name):
    """scripts/gen_minigrid_golden.py reran every fixture in float64 and stored, per class of compared quantity, the float32
    reference's largest deviation as a fraction of the bar tests/test_gpu_minigrid.py applies to that class.  A bar the reference
    itself used up would test nothing: every fraction stays under a quarter."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    devs = {k: float(g[k]) for k in g.files if k.startswith('fp64_dev_')}
    want = {'tiny_minigrid_eval': {'fp64_dev_eval'}, 'tiny_minigrid_inference': {'fp64_dev_inference'}}.get(
        name, {'fp64_dev_' + k for k in ('losses', 'metrics', 'tensors', 'grad_norms', 'full_grads', 'param_abs_sums')})
    assert set(devs) == want
    for k, v in devs.items():
        print(f'{name} {k}: {v:.3e} of the bar')
        assert 0.0 <= v <= 0.25, (k, v)
    assert float(g['min_edge_distance']) > 1e-5
    if 'min_map_rec_gap' in g.files:
        assert float(g['min_map_rec_gap']) > 1e-4
