"""WorldModelProbe(model='gru_probe') without a GPU: the parameter tree against the reference-written fixtures
(scripts/gen_gru_probe_golden.py), initialisation, the one-optimizer form, every refusal, the host-side argument checks of the
dm_gru_sequence_ entry points, and the fixtures' own fp32-vs-fp64 deviation against the bars tests/test_gpu_gru_probe.py applies."""
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

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
FIXTURES = ['tiny_gru_probe_map_goals', 'tiny_gru_probe_goals']
# the bars of tests/test_gpu_gru_probe.py, by the name of the fixture's fp64_dev_* record
BARS = dict(loss=2e-5, metrics=1e-4, tensors=1e-4, grad_norms=2e-3, full_grads=2e-3, param_abs_sums=2e-6)
NEW_SYMBOLS = ['dm_gru_sequence_acts_floats', 'dm_gru_sequence_ws_bytes', 'dm_gru_sequence_fwd', 'dm_gru_sequence_bwd',
               'dm_gru_sequence_last_schedule', 'dm_gru_sequence_fuse_enable']


def _conf(name=None, **more):
    from pydreamer_amd import config
    if name is None:
        base = dict(vars(O.tiny_conf()), model='gru_probe', probe_gradients=True, probe_model='goals', goals_size=3)
        return config.load_config('defaults', 'atari', **{**base, **more})
    g = np.load(os.path.join(GOLD, name + '.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    return config.load_config('defaults', 'atari', **{**vars(oconf), **dict(ast.literal_eval(str(g['extra_conf_json']))), **more}), g


@pytest.mark.parametrize('name', FIXTURES)
def test_state_dict_names_shapes_and_order_equal_the_reference(name):
    from pydreamer_amd.models import WorldModelProbe
    conf, g = _conf(name)
    with torch.device('meta'):
        model = WorldModelProbe(conf)
    want = CFP.shapes_of_fixture(g)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert list(got.items()) == list(want.items())
    assert [k for k, _ in model.named_parameters()] == list(want)      # every entry is a parameter, in optimizer order
    D_, A = conf.deter_dim, conf.action_dim
    assert got['wm.squeeze.weight'] == (32, 32 * conf.cnn_depth)
    assert got['wm.rnn.weight_ih_l0'] == (3 * D_, 32 + A) and got['wm.rnn.weight_hh_l0'] == (3 * D_, D_)
    assert got['wm.encoder.encoder_image.model.0.weight'][1] == (5 if conf.reward_input else 3)
    assert tuple(model.init_state(4).shape) == (1, 4, D_)


def test_initialisation_follows_the_reference():
    """baselines.py:54-55: init_weights_tf2 over ALL modules - the probe's Linears are Xavier with zero bias (under Dreamer they keep
    torch's default) - while nn.GRU keeps torch's U(-1/sqrt(D), 1/sqrt(D)) on all four tensors."""
    from pydreamer_amd.models import LinearP, WorldModelProbe
    torch.manual_seed(3)
    model = WorldModelProbe(_conf('tiny_gru_probe_map_goals')[0])
    linears = [m for m in model.probe_model.modules() if isinstance(m, LinearP)]
    assert len(linears) == 3 + 5 + 5
    model.requires_grad_(False)
    for m in linears + [model.wm.squeeze]:
        assert float(m.bias.abs().max()) == 0.0
        lim = (6.0 / (m.weight.shape[0] + m.weight.shape[1])) ** 0.5
        assert 0.9 * lim < float(m.weight.abs().max()) <= lim
    k = 1.0 / model.conf.deter_dim ** 0.5
    for p in model.wm.rnn.parameters():
        assert 0.8 * k < float(p.abs().max()) <= k and float(p.abs().min()) > 0.0


def test_one_optimizer_over_all_parameters_in_module_order(monkeypatch):
    from pydreamer_amd import baselines

    class Recorder:
        def __init__(self, params, lr, eps):
            self.params, self.lr, self.eps = list(params), lr, eps

    monkeypatch.setattr(baselines, 'FusedAdamW', Recorder)
    model = baselines.WorldModelProbe(_conf())
    opts = model.init_optimizers(3e-4, 1e-4, 1e-4, 1e-5)
    assert isinstance(opts, tuple) and len(opts) == 1
    assert [id(p) for p in opts[0].params] == [id(p) for p in model.parameters()]
    assert (opts[0].lr, opts[0].eps) == (3e-4, 1e-5)


def test_refusals():
    from pydreamer_amd.models import WorldModelProbe
    for model in ('vae', 'gru_vae', 'transformer_vae'):
        with pytest.raises(NotImplementedError):
            WorldModelProbe(_conf(model=model))
    for bad in (dict(probe_gradients=False), dict(probe_model='none'), dict(vecobs_size=5), dict(amp=True)):
        with pytest.raises(NotImplementedError):
            WorldModelProbe(_conf(**bad))
    for model in ('dreamer', 'no_such_model'):
        with pytest.raises(ValueError):
            WorldModelProbe(_conf(model=model))
    m = WorldModelProbe(_conf())
    with pytest.raises(AssertionError):
        m.training_step({}, m.init_state(3), iwae_samples=2)
    with pytest.raises(ValueError):          # (checked before anything touches a device)
        m.training_step(dict(image=torch.zeros(1), reset=torch.zeros(1)), m.init_state(3))


def test_new_symbols_and_host_side_argument_checks(hip):
    assert set(NEW_SYMBOLS) <= set(hip.exported_symbols())
    lib = hip.lib()
    assert lib.dm_version() == 17
    assert lib.dm_gru_sequence_fuse_enable(-1) == 1 and lib.dm_gru_sequence_fuse_enable(7) == 1      # default; a bad value changes nothing
    assert lib.dm_gru_sequence_fuse_enable(2) == 2 and lib.dm_gru_sequence_fuse_enable(1) == 1
    T, B, In, D = 3, 2, 7, 8
    assert lib.dm_gru_sequence_acts_floats(T, B, In, D) >= 2 * T * B * 3 * D + B * D
    wsb = lib.dm_gru_sequence_ws_bytes(T, B, In, D)
    assert wsb >= 4 * (2 * T * B * 3 * D + 2 * B * D)
    assert lib.dm_gru_sequence_acts_floats(0, B, In, D) == 0 and lib.dm_gru_sequence_ws_bytes(T, B, In, 0) == 0
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its host-side checks
    params = hip.dm_gru_params()
    params.w_ih = params.w_hh = params.b_ih = params.b_hh = fake.value
    P = ctypes.byref(params)

    def fwd(T=T, B=B, In=In, D=D, x=fake, h0=fake, p=P, H=fake, ws=fake, wsb=wsb):
        return lib.dm_gru_sequence_fwd(T, B, In, D, x, In, h0, None, p, None, H, D, ws, wsb, None)

    def bwd(T=T, B=B, In=In, D=D, acts=fake, dH=fake, g=P, ws=fake, wsb=wsb):
        return lib.dm_gru_sequence_bwd(T, B, In, D, fake, In, P, acts, fake, D, dH, D, g, None, 0, ws, wsb, None)

    DM_E_SHAPE, DM_E_WORKSPACE, DM_E_NULL = -1, -2, -5
    for call in (fwd, bwd):
        for kw in (dict(T=0), dict(B=0), dict(In=0), dict(D=0), dict(D=6)):
            assert call(**kw) == DM_E_SHAPE, kw
            assert lib.dm_last_error()
        assert call(wsb=wsb - 4) == DM_E_WORKSPACE
        assert b'workspace' in lib.dm_last_error()
        assert call(ws=None) == DM_E_NULL
    for kw in (dict(x=None), dict(h0=None), dict(p=None), dict(H=None)):
        assert fwd(**kw) == DM_E_NULL, kw
    for kw in (dict(acts=None), dict(dH=None), dict(g=None)):
        assert bwd(**kw) == DM_E_NULL, kw
    empty = hip.dm_gru_params()
    assert fwd(p=ctypes.byref(empty)) == DM_E_NULL and bwd(g=ctypes.byref(empty)) == DM_E_NULL


@pytest.mark.parametrize('name', FIXTURES)
def test_the_reference_alone_is_far_inside_the_bars(name):
    """For every compared quantity the fp32 reference's own deviation from the same iterations in float64, stored by the generator,
    is at most a quarter of the bar the GPU test applies to it."""
    _, g = _conf(name)
    for k, bar in BARS.items():
        dev = float(g['fp64_dev_' + k])
        print(f'{name} {k}: reference fp32-vs-fp64 deviation {dev:.2e}, bar {bar:.0e}')
        assert 0.0 < dev <= bar / 4, (k, dev, bar)
    if 'map' in name:
        assert float(g['min_map_rec_gap']) > 1e-4
    for s in range(2):
        assert g[f's{s}_in_reset'][1:].any(), 'the fixture keeps its mid-sequence reset'
        assert np.isnan(float(g[f's{s}_metric_mse_goal_age1000']))
