"""The trainer loop without a GPU: the four logging symbols are exported, declared and refuse bad arguments on the
host; prepare_batch_npz on host tensors against the rule restated here; the checkpoint file; Collector over scripted environments
against collect(); episode chunking against the cut rule; run()'s argument errors."""
import os
import re

import numpy as np
import pytest
import torch

from pydreamer_amd import config, hip, replay as R
from pydreamer_amd.collect import Collector, EpisodeRecorder, collect
from tests.test_collect_cpu import A, ScriptEnv, ScriptPolicy, _load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dm_metric_accum', 'dm_batch_stats', 'dm_masked_mean', 'dm_export_image_u8')


def test_new_symbols_are_exported_declared_and_checked_on_the_host():
    from pydreamer_amd import train as TR
    hdr = open(os.path.join(ROOT, 'include', 'dreamer_hip.h')).read()
    lib = hip.lib()
    for name in NEW:
        assert re.search(r'\bint ' + name + r'\(', hdr), name
        assert name in hip.exported_symbols() and hasattr(lib, name), name
    assert lib.dm_version() == 17 and TR.METRIC_BUF_FLOATS == 48
    one = lambda: __import__('ctypes').c_void_p(64)      # a non-null pointer nothing dereferences: every call below fails its host check
    E = hip.DreamerHipError
    with pytest.raises(E, match='code -5'):
        hip.call('dm_metric_accum', 4, None, one(), one(), one(), one(), None)
    with pytest.raises(E, match='code -1'):
        hip.call('dm_metric_accum', 257, one(), one(), one(), one(), one(), None)
    with pytest.raises(E, match='code -5'):
        hip.call('dm_batch_stats', 4, one(), None, None, one(), None)
    with pytest.raises(E, match='code -1'):
        hip.call('dm_masked_mean', 2, 4, one(), 3, 5, None, 1, one(), None)
    with pytest.raises(E, match='code -1'):
        hip.call('dm_masked_mean', 2, 4, one(), 4, 5, None, 2, one(), None)
    with pytest.raises(E, match='code -1'):
        hip.call('dm_export_image_u8', 1, 1, 1, 2, 4, 4, one(), one(), None)
    with pytest.raises(E, match='code -1'):
        hip.call('dm_export_image_u8', 1, 1, 1, 3, 4, 5, one(), one(), None)
    with pytest.raises(E, match='code -5'):
        hip.call('dm_export_image_u8', 1, 1, 1, 3, 4, 4, one(), None, None)
    with pytest.raises(ValueError):
        TR.rules_tensor([1, 5], 'cpu')
    with pytest.raises(ValueError):
        TR.rules_tensor([1] * 257, 'cpu')
    with pytest.raises(E):      # no CPU path: a host tensor is refused before anything is called
        TR.batch_stats(torch.zeros(4), torch.zeros(4, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------ prepare_batch_npz
def _rule(key, x, take_b):
    """train.py:423-465 restated on numpy arrays."""
    if take_b < x.shape[1]:
        x = x[:, :take_b]
    if x.dtype in (np.float16, np.float64):
        x = x.astype(np.float32)
    if x.ndim == 5:
        if x.shape[-1] == x.shape[-2]:
            x = x.transpose(0, 1, 3, 4, 2)
        if x.shape[-1] in (1, 3):
            x = ((x + 0.5) * 255.0).clip(0, 255).astype('uint8')
        elif np.allclose(x.sum(-1), 1.0) and np.allclose(x.max(-1), 1.0):
            x = x.argmax(-1)
        else:
            e = np.exp(x - x.max(-1, keepdims=True))
            x = e / e.sum(-1, keepdims=True)
    return x.swapaxes(0, 1)


@pytest.mark.parametrize('take_b', [1, 2, 999])
def test_prepare_batch_npz_on_host_tensors(take_b):
    from pydreamer_amd.train import prepare_batch_npz
    rs = np.random.RandomState(take_b)
    T, B = 3, 2
    classes = rs.randint(0, 4, (T, B, 7, 7))
    data = dict(
        image=rs.uniform(-0.7, 0.7, (T, B, 3, 8, 8)).astype(np.float32),
        image_gray=rs.uniform(-0.7, 0.7, (T, B, 1, 8, 8)).astype(np.float64),
        map=np.eye(4, dtype=np.float32)[classes].transpose(0, 1, 4, 2, 3).copy(),
        map_rec=rs.randn(T, B, 4, 7, 7).astype(np.float32),
        image_pred=rs.randn(T, B, 4, 7, 7).astype(np.float16),
        reward=rs.randn(T, B).astype(np.float32), reset=rs.rand(T, B) < 0.5,
        action=rs.randn(T, B, 5).astype(np.float64), vecobs=rs.randn(T, B, 4).astype(np.float16),
        map_coord=rs.randn(T, B, 2, 2).astype(np.float32), frames=rs.randint(0, 256, (T, B, 8, 8, 3)).astype(np.uint8))
    out = prepare_batch_npz({k: torch.from_numpy(v) for k, v in data.items()}, take_b=take_b)
    assert list(out) == list(data)
    nb = min(take_b, B)
    for k, v in data.items():
        ref = v[:, :take_b].swapaxes(0, 1) if k == 'frames' else _rule(k, v, take_b)
        assert out[k].shape == ref.shape and out[k].shape[:2] == (nb, T), (k, out[k].shape, ref.shape)
        assert out[k].dtype == ref.dtype, (k, out[k].dtype, ref.dtype)
        if k in ('map_rec', 'image_pred'):
            np.testing.assert_allclose(out[k], ref, rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(out[k].sum(-1), 1.0, rtol=1e-5)
        else:
            assert np.array_equal(out[k], ref), k
    assert out['image'].dtype == np.uint8 and out['image'].shape == (nb, T, 8, 8, 3)
    assert out['map'].shape == (nb, T, 7, 7) and np.array_equal(out['map'], classes[:, :take_b].swapaxes(0, 1))
    assert out['vecobs'].dtype == np.float32 and out['action'].dtype == np.float32 and out['reset'].dtype == bool
    with pytest.raises(AssertionError):
        prepare_batch_npz({'weird': torch.zeros(T, B, 3, 8, 8)})


# ------------------------------------------------------------------------------------------------ checkpoints
def test_checkpoint_layout_and_round_trip(tmp_path):
    from pydreamer_amd.train import load_checkpoint, save_checkpoint
    torch.manual_seed(0)
    make = lambda: torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    model = make()
    opts = [torch.optim.Adam(model[0].parameters()), torch.optim.Adam(model[1].parameters())]
    model(torch.randn(5, 3)).sum().backward()
    for o in opts:
        o.step()
    path = str(tmp_path / 'checkpoints' / 'latest.pt')
    assert load_checkpoint(path, model, opts) is None
    save_checkpoint(path, model, opts, 17)
    assert os.listdir(os.path.dirname(path)) == ['latest.pt']      # the temporary name is gone
    ck = torch.load(path)
    assert list(ck) == ['epoch', 'model_state_dict', 'optimizer_0_state_dict', 'optimizer_1_state_dict'] and ck['epoch'] == 17
    fresh = make()
    fopts = [torch.optim.Adam(fresh[0].parameters()), torch.optim.Adam(fresh[1].parameters())]
    assert load_checkpoint(path, fresh, fopts) == 17
    for (k, a), b in zip(model.state_dict().items(), fresh.state_dict().values()):
        assert torch.equal(a, b), k
    for o, f in zip(opts, fopts):
        for sa, sb in zip(o.state_dict()['state'].values(), f.state_dict()['state'].values()):
            assert all(torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])) for k in sa)
    assert load_checkpoint(path, make()) == 17      # without optimizers


# ------------------------------------------------------------------------------------------------ Collector, chunking
def _files(d):
    return {n: _load(os.path.join(d, n)) for n in sorted(os.listdir(d)) if n.endswith('.npz')}


def _same_files(a, b):
    assert list(a) == list(b), (list(a), list(b))
    for n in a:
        assert list(a[n]) == list(b[n]), n
        for k in a[n]:
            assert a[n][k].dtype == b[n][k].dtype and np.array_equal(a[n][k], b[n][k], equal_nan=a[n][k].dtype.kind == 'f'), (n, k)


@pytest.mark.parametrize('lengths,k', [([[3, 3], [2, 4], [6]], 6),       # every environment closes an episode on step k: none spans
                                       ([[4, 5], [7, 3], [5, 4, 6]], 6)])   # episodes span the split
def test_collector_runs_add_up_to_collect(tmp_path, lengths, k):
    da, db = str(tmp_path / 'a'), str(tmp_path / 'b')
    os.makedirs(da), os.makedirs(db)
    envs_a = [ScriptEnv(i, l) for i, l in enumerate(lengths)]
    out = collect(envs_a, ScriptPolicy(3), EpisodeRecorder(R.LocalEpisodeRepository(da), 3, steps_per_npz=1), 2 * k)
    envs_b = [ScriptEnv(i, l) for i, l in enumerate(lengths)]
    rec = EpisodeRecorder(R.LocalEpisodeRepository(db), 3, steps_per_npz=1)
    col = Collector(envs_b, ScriptPolicy(3), rec)
    o1 = col.run(k)
    open_rows = [len(r) for r in rec.rows]
    o2 = col.run(k)
    col.close()
    assert o1['steps'] == o2['steps'] == 3 * k and o1['episodes'] + o2['episodes'] == out['episodes'] > 0
    assert len(envs_b[0].episodes) == len(envs_a[0].episodes)      # reset once, by the first run() only
    _same_files(_files(da), _files(db))
    spans = [(i, e) for i, env in enumerate(envs_b) for e, s in enumerate(env.starts)
             if s < k < s + env.lengths[e % len(env.lengths)] <= 2 * k]
    if lengths[0] == [3, 3]:
        assert not spans and open_rows == [1, 1, 1]      # only the fresh reset rows were open at the split
    else:
        assert spans and max(open_rows) > 1
        tags = [f['tag'] for f in _files(db).values()]
        for i, e in spans:      # the spanning episode is in a file, whole
            L = envs_b[i].lengths[e % len(envs_b[i].lengths)]
            assert any(((t[:, 0] == i) & (t[:, 1] == e)).sum() == L + 1 for t in tags), (i, e)


def test_collector_flush_keeps_open_episodes(tmp_path):
    envs = [ScriptEnv(0, [5])]
    rec = EpisodeRecorder(R.LocalEpisodeRepository(str(tmp_path)), 1, steps_per_npz=10 ** 6)
    col = Collector(envs, ScriptPolicy(1), rec)
    col.run(7)
    assert col.flush() is not None and rec.steps_saved == 5 and len(rec.rows[0]) == 3
    col.run(3)
    col.close()
    assert rec.steps_saved == 10 and rec.files and rec.rows == [[]]
    with pytest.raises(ValueError):
        Collector(envs, ScriptPolicy(1), EpisodeRecorder(R.LocalEpisodeRepository(str(tmp_path)), 2))


@pytest.mark.parametrize('chunk', [False, True])
def test_episode_chunking_follows_the_cut_rule(tmp_path, chunk):
    spn, steps = 4, 10      # a queue of 2.5 steps_per_npz
    env = ScriptEnv(0, [steps])
    rec = EpisodeRecorder(R.LocalEpisodeRepository(str(tmp_path)), 1, steps_per_npz=spn, chunk=chunk)
    collect([env], ScriptPolicy(1), rec, steps)
    files = _files(str(tmp_path))
    whole = {k: np.array([r[k] for r in env.episodes[0]]) for k in ('reward', 'reset', 'tag')}
    assert rec.steps_saved == steps
    if not chunk:
        assert list(files) == [f'ep000000_000000-r{whole["reward"].sum():.0f}-{steps:04}.npz']
        assert np.array_equal(files[list(files)[0]]['tag'], whole['tag'])
        return
    pieces = steps // spn
    bounds = [0] + [steps * (i + 1) // pieces + 1 for i in range(pieces)]
    assert pieces == 2 and bounds == [0, 6, 11] and len(files) == pieces
    for i, (a, z) in enumerate(zip(bounds, bounds[1:])):
        n_steps = (z - a) - int(whole['reset'][a:z].sum())
        name = f'ep000000_000000-{i}-r{whole["reward"][a:z].sum():.0f}-{n_steps:04}.npz'
        assert name in files, (name, list(files))
        assert np.array_equal(files[name]['tag'], whole['tag'][a:z]) and 'image_t' in files[name]
        assert files[name]['image_t'].shape[-1] == z - a
    assert R.LocalEpisodeRepository(str(tmp_path)).count_steps() == (2, steps, 1)
    # below 2 steps_per_npz nothing is cut
    d2 = str(tmp_path / 'short')
    os.makedirs(d2)
    rec2 = EpisodeRecorder(R.LocalEpisodeRepository(d2), 1, steps_per_npz=spn, chunk=True)
    collect([ScriptEnv(0, [7])], ScriptPolicy(1), rec2, 7)
    assert len(_files(d2)) == 1 and re.fullmatch(r'ep000000_000000-r\d+-0007\.npz', list(_files(d2))[0])


# ------------------------------------------------------------------------------------------------ run()
def test_run_argument_errors(tmp_path):
    from pydreamer_amd.train import run
    repo = R.LocalEpisodeRepository(str(tmp_path))
    conf = config.load_config('defaults', 'vectorenv')
    assert conf.limit_step_ratio == 0
    with pytest.raises(ValueError, match='env_steps_per_grad_step'):
        run(conf, repo, envs=[ScriptEnv(0, [4])], logdir=str(tmp_path / 'log'))
    with pytest.raises(ValueError, match='model'):
        run(config.load_config('defaults', 'vectorenv', model='rssm_probe'), repo, logdir=str(tmp_path / 'log'))
    assert not os.path.exists(str(tmp_path / 'log'))
