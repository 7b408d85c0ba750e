"""CPU (-m "not gpu"): the config surface of reward_input and vecobs_size - state_dict names, order and shapes against the lists
the reference-written fixtures recorded, what is still refused, the `miniworld` and `minecraft` sections, vecobs through the
replay and the batch sharding, and the new entry points' argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_form_params as CFP                     # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402
from pydreamer_amd import config, hip                # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
DM_E_NULL_TEXT = 'null pointer'


def _conf(**kw):
    return config.load_config('defaults', 'atari', **{**vars(O.tiny_conf()), **kw})


FIXTURES = {'tiny_reward_input': dict(reward_input=True), 'tiny_vecobs': dict(vecobs_size=27),
            'tiny_obs_combo': dict(reward_input=True, vecobs_size=27, iwae_samples=2),
            'tiny_obs_eval': dict(reward_input=True, vecobs_size=27), 'tiny_obs_open_loop': dict(reward_input=True, vecobs_size=27),
            'tiny_obs_inference': dict(reward_input=True, vecobs_size=27), 'tiny_obs_amp': dict(reward_input=True, vecobs_size=27)}


@pytest.mark.parametrize('fixture', list(FIXTURES))
def test_state_dict_matches_the_reference_list(fixture):
    """Names, ORDER and shapes of the reference's state_dict with reward_input, with vecobs_size, and with both, as
    scripts/gen_obs_golden.py recorded them: encoder_vecobs behind encoder_image, decoder.vecobs behind decoder.terminal."""
    from pydreamer_amd.models import Dreamer
    g = np.load(os.path.join(GOLD, fixture + '.npz'))
    assert float(g['min_edge_distance']) > 1e-5
    kw = FIXTURES[fixture]
    shapes = CFP.shapes_of_fixture(g)
    with torch.device('meta'):
        sd = Dreamer(_conf(**kw)).state_dict()
    assert list(sd.keys()) == list(shapes.keys())
    for k, sh in shapes.items():
        assert tuple(sd[k].shape) == sh, k
    d, keys = O.tiny_conf().cnn_depth, list(shapes)
    assert shapes['wm.encoder.encoder_image.model.0.weight'] == (d, 5 if kw.get('reward_input') else 3, 4, 4)
    if kw.get('vecobs_size'):
        ev = [k for k in keys if k.startswith('wm.encoder.encoder_vecobs.')]
        dv = [k for k in keys if k.startswith('wm.decoder.vecobs.')]
        assert [k.split('model.')[-1].split('.')[0] for k in ev[::2]] == ['0', '1', '3', '4', '6']
        assert sorted({int(k.split('model.model.')[1].split('.')[0]) for k in dv}) == [0, 1, 3, 4, 6, 7, 9, 10, 12]
        assert keys.index(ev[0]) == keys.index('wm.encoder.encoder_image.model.6.bias') + 1
        assert keys.index(dv[0]) == max(i for i, k in enumerate(keys) if k.startswith('wm.decoder.terminal.')) + 1
        assert shapes['wm.core.cell.post_mlp_e.weight'][1] == 32 * d + 256 and shapes[dv[-1]] == (27,)


def test_closed_form_rule_is_the_oracles():
    oconf = O.tiny_conf()
    a, b = O.make_params(oconf), CFP.make_params(O.param_shapes(oconf))
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('kw', [dict(image_encoder='dense'), dict(image_decoder='dense'), dict(image_encoder=None, vecobs_size=27),
                                dict(reward_decoder_categorical=[-1, 0, 1]), dict(probe_model='goals'),
                                dict(image_size=32), dict(actor_grad='dynamics'), dict(reward_input=True, cnn_depth=24),
                                dict(reward_input=True, image_channels=1)],
                         ids=lambda kw: ','.join(f'{k}={v}' for k, v in kw.items()))
def test_still_refused_configs_raise(kw):
    from pydreamer_amd.models import Dreamer
    with pytest.raises(NotImplementedError):
        with torch.device('meta'):
            Dreamer(_conf(**kw))


@pytest.mark.parametrize('depth', [8, 16, 32, 48, 64])
def test_reward_input_depths_construct(depth):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'):
        m = Dreamer(_conf(reward_input=True, cnn_depth=depth))
    assert tuple(m.wm.encoder.encoder_image.model[0].weight.shape) == (depth, 5, 4, 4)
    assert m.wm.encoder.out_dim == 32 * depth


def test_miniworld_section():
    from pydreamer_amd.models import Dreamer
    c = config.load_config('defaults', 'miniworld')
    assert (c.reward_input, c.cnn_depth, c.action_dim, c.probe_model, c.image_size) == (True, 32, 3, 'none', 64)
    assert set(config.SECTIONS['miniworld']) <= set(config.SECTIONS['defaults'])
    with torch.device('meta'):
        sd = Dreamer(c).state_dict()
    assert tuple(sd['wm.encoder.encoder_image.model.0.weight'].shape) == (32, 5, 4, 4)


def test_minecraft_section():
    from pydreamer_amd.models import Dreamer
    c = config.load_config('defaults', 'minecraft')
    assert (c.vecobs_size, c.action_dim, c.clip_rewards, c.reward_input) == (27, 29, 'log1p', False)
    assert set(config.SECTIONS['minecraft']) <= set(config.SECTIONS['defaults'])
    with torch.device('meta'):
        m = Dreamer(c)
    assert m.wm.encoder.out_dim == 32 * c.cnn_depth + 256
    assert tuple(m.state_dict()['wm.decoder.vecobs.model.model.12.weight'].shape) == (27, 400)


def test_vecobs_through_replay_and_sharding(tmp_path):
    """preprocess_batch passes `vecobs` through as float32 (preprocessing.py:162-163; DeviceRing ships every key of such a batch),
    dist.shard_obs slices it on the batch axis."""
    from pydreamer_amd import dist as DP, replay
    T, B, V = 6, 4, 27
    rs = np.random.RandomState(0)
    batch = dict(image=rs.randint(0, 256, (T, B, 64, 64, 3)).astype(np.uint8), action=rs.randint(0, 5, (T, B)),
                 reward=rs.randn(T, B), terminal=np.zeros((T, B)), reset=np.zeros((T, B), bool), vecobs=rs.randn(T, B, V))
    out = replay.preprocess_batch(batch, 5)
    assert out['vecobs'].dtype == np.float32 and np.array_equal(out['vecobs'], batch['vecobs'].astype(np.float32))
    assert 'vecobs' not in replay.preprocess_batch({k: v for k, v in batch.items() if k != 'vecobs'}, 5)
    obs = {k: torch.from_numpy(v) for k, v in out.items()}
    for rank in range(3):
        shard, (lo, hi) = DP.shard_obs(obs, 3, rank)
        assert torch.equal(shard['vecobs'], obs['vecobs'][:, lo:hi]) and shard['vecobs'].is_contiguous()


def test_planes_entry_points_check_their_arguments():
    """Bound with the declared signatures; null pointers are refused on the host (DM_E_NULL), nothing is launched."""
    shp = hip.make_shape(T=1, B=2, I=1, H=1, D=64, Hd=64, S=8, C=8, E=256, A=6, mlp_hidden=400, mlp_layers=4, cnn_depth=8, img=64,
                         img_ch=3, flags=0)
    import ctypes
    for name, args in (('dm_conv_encoder_fwd_planes', (ctypes.byref(shp), None, None, None, None, None, None, 256, None, 0, None)),
                       ('dm_conv_encoder_bwd_planes', (ctypes.byref(shp), None, None, None, None, None, None, 256, None, None, 0, None))):
        with pytest.raises(hip.DreamerHipError) as e:
            hip.call(name, *args)
        assert DM_E_NULL_TEXT in str(e.value), str(e.value)
    with pytest.raises(hip.DreamerHipError) as e:
        hip.call('dm_head_loss_normal_nd', 15, 27, None, None, 1.0, 0.0, None, None, None, None)
    assert DM_E_NULL_TEXT in str(e.value), str(e.value)
