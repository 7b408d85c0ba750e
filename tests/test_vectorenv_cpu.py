"""CPU (-m "not gpu"): the host side of image-less world models - the `vectorenv` section: construction on `meta`
against the state_dict tables the fixtures of scripts/gen_vectorenv_golden.py recorded from the reference, the gate, the
optimizer groups, preprocess_batch(image_key=None) against the reference Preprocessor's own output, and both replay feeds over
episode files that hold no frames."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_form_params as CFP                     # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402
from pydreamer_amd import config                     # noqa: E402
from pydreamer_amd import replay as R                # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
FIXTURES = ['tiny_vectorenv', 'tiny_vectorenv_iwae', 'tiny_vectorenv_cont', 'tiny_vectorenv_eval', 'tiny_vectorenv_open_loop',
            'tiny_vectorenv_inference', 'tiny_vectorenv_amp']
TINY = dict(deter_dim=64, hidden_dim=64, stoch_dim=8, stoch_discrete=8, batch_length=5, batch_size=3, imag_horizon=4)


def _conf(**kw):
    return config.load_config('defaults', 'vectorenv', **{**TINY, **kw})


def _fixture_conf(g, **more):
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    return oconf, config.load_config('defaults', 'vectorenv', **{**vars(oconf), **dict(ast.literal_eval(str(g['extra_conf_json']))), **more})


def _meta(conf):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'):
        return Dreamer(conf)


@pytest.mark.parametrize('name', FIXTURES)
def test_state_dict_equals_the_reference(name):
    g = np.load(os.path.join(GOLD, name + '.npz'))
    _, conf = _fixture_conf(g)
    assert conf.image_encoder is None and conf.image_decoder is None and conf.image_key is None and conf.vecobs_size == 4
    sd = _meta(conf).state_dict()
    shapes = CFP.shapes_of_fixture(g)
    assert list(sd.keys()) == list(shapes.keys())
    assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for s in shapes.values()]
    assert not [k for k in sd if 'image' in k]
    assert shapes['wm.encoder.encoder_vecobs.model.0.weight'] == (400, 4)
    assert shapes['wm.core.cell.post_mlp_e.weight'] == (conf.hidden_dim, 256)


def test_vectorenv_section_constructs():
    c = config.load_config('defaults', 'vectorenv')
    assert (c.action_dim, c.vecobs_size, c.image_key, c.image_encoder, c.image_decoder) == (2, 4, None, None, None)
    assert set(config.SECTIONS['vectorenv']) <= set(config.SECTIONS['defaults'])
    m = _meta(c)
    assert m.wm.imageless and not m.wm.dense and m.wm.encoder.encoder_image is None and m.wm.decoder.image is None
    assert m.wm.encoder.out_dim == 256
    sd = m.state_dict()
    assert len(sd) == 141 and not [k for k in sd if 'image' in k]
    assert tuple(sd['wm.encoder.encoder_vecobs.model.0.weight'].shape) == (400, 4)
    assert tuple(sd['wm.core.cell.post_mlp_e.weight'].shape) == (c.hidden_dim, 256)
    shp = m.wm.shape(c.batch_length, c.batch_size, c.imag_horizon)
    assert (shp.E, shp.cnn_depth, shp.img, shp.img_ch) == (256, 0, 0, 0)


@pytest.mark.parametrize('empty', [None, ''])
def test_the_gate(empty):
    both = dict(image_encoder=empty, image_decoder=empty)
    assert _meta(_conf(**both)).wm.imageless
    with pytest.raises(ValueError, match='vecobs_size'):
        _meta(_conf(vecobs_size=0, **both))
    for kw in (dict(image_encoder=empty, image_decoder='cnn'), dict(image_encoder='cnn', image_decoder=empty)):
        with pytest.raises(NotImplementedError, match='both or neither'):
            _meta(_conf(**kw))
    for probe in ('map', 'goals', 'map+goals'):
        with pytest.raises(NotImplementedError):
            _meta(_conf(probe_model=probe, goals_size=3, map_size=5, map_channels=4, **both))
    # image_size, image_channels and cnn_depth are not read: nothing about them can refuse the model
    assert _meta(_conf(image_size=17, image_channels=1, cnn_depth=24, **both)).wm.imageless


@pytest.mark.parametrize('kw', [dict(gru_type='gru_layernorm_dv2', gru_layers=2), dict(layer_norm=False), dict(stoch_discrete=0),
                                dict(iwae_samples=3), dict(aux_critic=True), dict(actor_dist='normal_tanh'), dict(amp=True),
                                dict(kl_balance=0.5)], ids=lambda kw: ','.join(f'{k}={v}' for k, v in kw.items()))
def test_everything_beside_the_image_constructs(kw):
    assert _meta(_conf(**kw)).wm.imageless


def test_reward_input_is_ignored():
    """encoders.py:49-59 reads reward_input inside the image branch only: no planes, the same keys and shapes."""
    a, b = _meta(_conf()), _meta(_conf(reward_input=True))
    assert not b.wm.encoder.reward_input
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape for k in sa)


def test_optimizer_groups_are_the_references():
    """dreamer.py:60-66: wm / probe / actor / critic by name prefix; critic_target belongs to no optimizer."""
    m = _meta(_conf(aux_critic=True))
    names = {id(p): n for n, p in m.named_parameters()}
    groups = {k: [names[id(p)] for p in v] for k, v in m.param_groups().items()}
    for k, got in groups.items():
        assert got == [n for n in names.values() if O.group_of(n) == k], k
    assert groups['probe'] == ['probe_model.dummy']
    assert any(n.startswith('wm.encoder.encoder_vecobs.') for n in groups['wm']) and not [n for n in groups['wm'] if 'image' in n]
    grouped = {n for v in groups.values() for n in v}
    assert {n for n in names.values() if n not in grouped} == {n for n in names.values() if n.startswith('ac.critic_target.')}


def test_preprocess_batch_equals_the_reference():
    g = np.load(os.path.join(GOLD, 'vectorenv_preprocess.npz'))
    raw = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    want = {k[4:]: g[k] for k in g.files if k.startswith('out_')}
    assert 'image' not in want and want['vecobs'].dtype == np.float32
    for key in (None, ''):
        got = R.preprocess_batch(raw, 2, clip_rewards='tanh', image_key=key)
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, want[k].dtype)
            assert np.array_equal(got[k], want[k]), k


def test_shard_obs_names_no_image():
    from pydreamer_amd import dist as DP
    T, B = 5, 7
    obs = dict(action=torch.zeros(T, B, 2), reward=torch.arange(T * B).float().view(T, B), terminal=torch.zeros(T, B),
               reset=torch.zeros(T, B, dtype=torch.bool), vecobs=torch.arange(T * B * 4).float().view(T, B, 4))
    cols = []
    for rank in range(3):
        part, (lo, hi) = DP.shard_obs(obs, 3, rank)
        assert sorted(part) == sorted(obs) and torch.equal(part['vecobs'], obs['vecobs'][:, lo:hi])
        cols += list(range(lo, hi))
    assert cols == list(range(B))


def _write_episodes(tmp_path, A=2, V=4, vecobs=True):
    """Episode files without frames: integer actions, vecobs, one file without `terminal`."""
    rs = np.random.RandomState(11)
    repo = R.LocalEpisodeRepository(str(tmp_path))
    for ep, n in enumerate([23, 37, 29, 41]):
        d = dict(action=rs.randint(0, A, n), reward=np.abs(rs.randn(n)).astype(np.float32) * 3, terminal=np.zeros(n, bool),
                 reset=np.zeros(n, bool))
        if vecobs:
            d['vecobs'] = rs.randn(n, V)
        d['terminal'][-1] = True
        if ep == 1:
            del d['terminal']
        repo.save_data(d, ep, ep)
    return repo


KW = dict(batch_length=6, batch_size=4, allow_mid_reset=True, reset_interval=10, seed=21)


def test_replay_feed_without_frames(tmp_path):
    repo = _write_episodes(tmp_path)
    feed = R.ReplayFeed(R.SequentialReplay(repo, **KW), 2, clip_rewards='tanh', image_key=None)
    plain = iter(R.SequentialReplay(repo, **KW))
    spec = feed.spec()
    assert 'image' not in spec and spec['vecobs'] == ((6, 4, 4), np.float32)
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in spec.items()}
    wrapped = 0
    for i in range(30):
        got = feed.fill(slot)
        want = R.preprocess_batch(next(plain), 2, clip_rewards='tanh', image_key=None)
        assert sorted(got) == sorted(want) and 'image' not in got
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (i, k)
        wrapped += int(got['reset'][1:].any())
    assert wrapped > 0, 'no window wrapped an episode boundary'


def test_feeds_refuse_files_without_vecobs(tmp_path):
    repo = _write_episodes(tmp_path, vecobs=False)
    for make in (lambda: R.ReplayFeed(R.SequentialReplay(repo, **KW), 2, image_key=None),
                 lambda: R.DeviceReplay(R.SequentialReplay(repo, **KW), 2, image_key=None)):
        with pytest.raises(ValueError, match='vecobs'):
            make()


def test_device_replay_plans_no_image_field(tmp_path):
    repo = _write_episodes(tmp_path)
    dr = R.DeviceReplay(R.SequentialReplay(repo, **KW), 2, clip_rewards='tanh', image_key=None)
    feed = R.ReplayFeed(R.SequentialReplay(repo, **KW), 2, clip_rewards='tanh', image_key=None)
    assert dr.spec() == feed.spec() and 'image' not in dr.names and 'vecobs' in dr.names
    from tests.test_device_replay_cpu import _gather, _same      # the gather kernel restated in numpy, driven by the tables alone
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in feed.spec().items()}
    for i in range(20):
        plan = dr.plan()
        assert plan.offsets.shape == (4, 2, len(dr.names)) and len(dr.names) == 6
        for e in plan.entries():
            assert sorted(e.offsets) == sorted(dr.names)
        _same(_gather(dr, plan), feed.fill(slot), i)
