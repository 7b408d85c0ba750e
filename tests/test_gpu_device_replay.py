"""-m gpu: the device-resident replay (csrc/replay_gather.hip, pydreamer_amd/replay.py DeviceReplay).

Every comparison is exact equality of bytes: the feed moves data, it computes nothing on the device.
  1. dm_replay_gather alone against numpy on synthetic sources: every access width (16 B, 4 B, bytes), a row wider than one
     workgroup sweep, the split between two pieces at every t, single-piece columns, marks on either piece, T = B = 1.
  2. DeviceReplay against an identically seeded SequentialReplay -> preprocess_batch for more batches than `depth`, with and
     without a capacity that forces evictions.
  3. Nine optimizer steps fed by DeviceReplay (with and without prefetch() after the step) against the DeviceRing-fed run.
  4. The map probe fed DeviceReplay's integer map against preprocess_batch's one-hot map."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import dreamer_oracle as O
from pydreamer_amd import replay as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
CANARY = 0xA5
ROW_BYTES = [12288, 196, 81, 1, 72, 4]            # 16-B path (768 chunks > 256 lanes), 4-B, bytes, the reset column, 4-B, 4-B
RESET_FIELD = 3


def _gather_case(hip, T, B, columns, seed):
    """columns: per batch column [(start, length, mark), ...] (one or two pieces).  Sources: per (column, piece, field) a tensor of
    its own with `rows` random rows; destinations start as CANARY with a guard row behind them."""
    rs = np.random.RandomState(seed)
    F = len(ROW_BYTES)
    rows = 11
    src_np = [[[rs.randint(0, 2 if f == RESET_FIELD else 256, (rows, rb)).astype(np.uint8) for f, rb in enumerate(ROW_BYTES)]
               for _ in range(2)] for _ in range(B)]
    src = [[[torch.from_numpy(a).to(DEV) for a in piece] for piece in col] for col in src_np]
    pieces = np.zeros((B, 2, 3), np.int32)
    ptrs = np.zeros((B, 2, F), np.int64)
    want = [np.full((T * B + 1, rb), CANARY, np.uint8) for rb in ROW_BYTES]
    for b, col in enumerate(columns):
        assert sum(n for _, n, _ in col) == T
        t = 0
        for p in range(2):
            q = p if p < len(col) else 0
            ptrs[b, p] = [src[b][q][f].data_ptr() for f in range(F)]
            assert all(v % 16 == 0 for v in ptrs[b, p])
            if p < len(col):
                start, n, mark = col[p]
                assert start + n <= rows
                pieces[b, p] = (start, n, mark)
                for f in range(F):
                    want[f].reshape(-1, ROW_BYTES[f])[[(t + i) * B + b for i in range(n)]] = src_np[b][p][f][start:start + n]
                if mark:
                    want[RESET_FIELD][t * B + b] = 1
                t += n
    dst = [torch.full((T * B + 1, rb), CANARY, dtype=torch.uint8, device=DEV) for rb in ROW_BYTES]
    fields = (hip.dm_replay_field * F)()
    for f in range(F):
        fields[f].dst, fields[f].row_bytes, fields[f].is_reset = dst[f].data_ptr(), ROW_BYTES[f], int(f == RESET_FIELD)
    table = torch.from_numpy(np.concatenate([ptrs.ravel(), pieces.ravel().view(np.int64)])).to(DEV)
    hip.call('dm_replay_gather', T, B, F, fields, ctypes.c_void_p(table.data_ptr() + 8 * ptrs.size), ctypes.c_void_p(table.data_ptr()),
             hip.stream())
    torch.cuda.synchronize()
    for f in range(F):
        got = dst[f].cpu().numpy()
        assert np.array_equal(got, want[f]), (columns, f, ROW_BYTES[f], np.argwhere(got != want[f])[:4])


@pytest.mark.parametrize('split', [1, 2, 3, 4])
def test_gather_entry_point_against_numpy(hip, split):
    """T=5, B=3: column 0 split at `split` (pieces from two episodes, starting mid-episode), column 1 a single piece, column 2 split
    at 5 - split; marks on the first piece, on the second, on both and on none (a single-piece column marked and unmarked)."""
    T, B = 5, 3
    for m0, m1 in ((1, 0), (0, 1), (1, 1), (0, 0)):
        cols = [[(3, split, m0), (0, T - split, m1)], [(6, T, m1)], [(11 - (T - split), T - split, m1), (2, split, m0)]]
        _gather_case(hip, T, B, cols, seed=10 * split + 2 * m0 + m1)


def test_gather_entry_point_single_row(hip):
    _gather_case(hip, 1, 1, [[(4, 1, 0)]], seed=1)
    _gather_case(hip, 1, 1, [[(10, 1, 1)]], seed=2)


# ------------------------------------------------------------------------------------------------ the feed
def _write_mixed_episodes(tmp_path, A=4, S=5, C=6):
    """Stored one-hot actions, vecobs, map fields; one file without `terminal`, one with time-last frames."""
    rs = np.random.RandomState(11)
    repo = R.LocalEpisodeRepository(str(tmp_path))
    for ep, n in enumerate([23, 37, 29, 41]):
        d = dict(image=rs.randint(0, 256, (n, 8, 8, 3)).astype(np.uint8), action=np.eye(A, dtype=np.float32)[rs.randint(0, A, n)],
                 reward=np.abs(rs.randn(n)).astype(np.float32) * 3, terminal=np.zeros(n, bool), reset=np.zeros(n, bool),
                 vecobs=rs.randn(n, 7), map=rs.randint(0, C, (n, S, S)).astype(np.uint8), agent_pos=rs.rand(n, 2) * S,
                 agent_dir=rs.randn(n, 2))
        d['map_seen'] = (d['map'] * (rs.rand(n, S, S) < 0.5)).astype(np.uint8)
        d['terminal'][-1] = True
        if ep == 1:
            del d['terminal']
        if ep == 2:
            d['image_t'] = d.pop('image').transpose(1, 2, 3, 0)
        repo.save_data(d, ep, ep)
    return repo


@pytest.mark.parametrize('evict', [False, True])
@pytest.mark.parametrize('clip', ['tanh', 'log1p'])
def test_device_replay_matches_the_host_reader(hip, tmp_path, clip, evict):
    A, C, depth, nb = 4, 6, 3, 14
    repo = _write_mixed_episodes(tmp_path, A=A, C=C)
    kw = dict(batch_length=6, batch_size=4, allow_mid_reset=True, reset_interval=10, seed=21)
    mk = dict(map_key='map', map_categorical=C)
    plain = iter(R.SequentialReplay(repo, **kw))
    probe = R.DeviceReplay(R.SequentialReplay(repo, **kw), A, **mk)
    for _ in range(nb):
        sizes = [e.nbytes for e in probe.plan().entries()]
    dr = R.DeviceReplay(R.SequentialReplay(repo, **kw), A, DEV, depth=depth, clip_rewards=clip,
                        capacity_bytes=int(1.5 * max(sizes)) if evict else 0, **mk)
    handed = []
    for i in range(nb):
        got = dr.next()
        if i % 2:
            dr.prefetch()                                      # staged ahead, while `got` is still being read
        assert all(v.is_cuda for v in got.values())
        handed.append({k: v.clone() for k, v in got.items()})
    torch.cuda.synchronize()
    dr.close()
    assert (len(dr._cache) < len(dr.replay.files)) == evict
    for i, got in enumerate(handed):
        raw = next(plain)
        want = R.preprocess_batch(raw, A, clip_rewards=clip, **mk)
        onehot = want.pop('map')
        want['map'] = raw['map']
        assert sorted(got) == sorted(want)
        for k, w in want.items():
            g = got[k].cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape, (i, k, g.dtype, w.dtype)
            assert g.tobytes() == np.ascontiguousarray(w).tobytes(), (i, k)
        assert np.array_equal(np.eye(C, dtype=np.float32)[got['map'].cpu().numpy()].transpose(0, 1, 4, 2, 3), onehot)


def test_device_replay_surfaces_producer_errors(hip, tmp_path):
    repo = _write_mixed_episodes(tmp_path)
    dr = R.DeviceReplay(R.SequentialReplay(repo, 6, 2, seed=1), 4, DEV)
    dr.next()
    dr.replay.files = []                                       # the next file choice fails in the producer thread
    with pytest.raises(RuntimeError, match='producer failed'):
        for _ in range(200):
            dr.next()
    dr.close()


def test_device_replay_feeds_training_step(hip, tmp_path):
    """The DeviceRing(ReplayFeed)-fed run of tests/test_gpu_replay.py, and the same nine steps fed by DeviceReplay - staged by
    next(), and staged ahead by prefetch() right after training_step() returned: losses and flat parameters bit-identical."""
    from tests.test_gpu_replay import _train, _write_episodes
    from tests.test_gpu_training_step import _build, _hip_conf
    oconf = O.tiny_conf()
    conf = _hip_conf(oconf)
    repo = _write_episodes(tmp_path, oconf.action_dim)
    nsteps = 9
    noises = [{k: v.to(DEV) for k, v in O.make_noise(oconf, seed=100 + s).items()} for s in range(nsteps)]
    replay = lambda: R.SequentialReplay(repo, oconf.batch_length, oconf.batch_size, allow_mid_reset=True, seed=7)

    ring = R.DeviceRing(R.ReplayFeed(replay(), oconf.action_dim, clip_rewards='tanh'), DEV, depth=3)
    a = _train(_build(oconf, O.make_params(oconf, seed=2)), conf, ring.next, noises, nsteps, after_step=ring.prefetch)
    ring.close()
    assert torch.isfinite(a[0]).all()
    for ahead in (False, True):
        dr = R.DeviceReplay(replay(), oconf.action_dim, DEV, depth=3, clip_rewards='tanh')
        b = _train(_build(oconf, O.make_params(oconf, seed=2)), conf, dr.next, noises, nsteps, after_step=dr.prefetch if ahead else None)
        dr.close()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f'prefetch={ahead}'


def test_map_probe_takes_the_integer_map_of_the_feed(hip, tmp_path):
    """probe_model='map' at the tiny fixture's configuration: loss_map, acc_map and acc_map_seen on DeviceReplay's batch (integer
    class map) are the bits of the same step on preprocess_batch's batch (one-hot map)."""
    from tests.test_gpu_map_probe import _model, _obs
    g = np.load(os.path.join(GOLD, 'tiny_map_probe.npz'))
    oconf, model = _model(g)
    C, S = model.probe_model.map_channels, model.probe_model.map_size
    _, noise = _obs(g, 's0_', oconf, C)
    rs = np.random.RandomState(6)
    repo = R.LocalEpisodeRepository(str(tmp_path))
    for ep, n in enumerate([17, 22]):
        d = dict(image=rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8), action=rs.randint(0, oconf.action_dim, n),
                 reward=rs.randn(n).astype(np.float32), terminal=np.zeros(n, bool), reset=np.zeros(n, bool),
                 map=rs.randint(0, C, (n, S, S)).astype(np.uint8), agent_pos=rs.rand(n, 2) * S, agent_dir=rs.randn(n, 2))
        d['map_seen'] = (d['map'] * (rs.rand(n, S, S) < 0.5)).astype(np.uint8)
        repo.save_data(d, ep, ep)
    kw = dict(batch_length=oconf.batch_length, batch_size=oconf.batch_size, allow_mid_reset=True, seed=3)
    mk = dict(map_key='map', map_categorical=C)
    dr = R.DeviceReplay(R.SequentialReplay(repo, **kw), oconf.action_dim, DEV, **mk)
    plain = iter(R.SequentialReplay(repo, **kw))
    state = model.init_state(oconf.batch_size)
    for _ in range(2):
        fed = dr.next()
        host = {k: torch.from_numpy(v).to(DEV) for k, v in R.preprocess_batch(next(plain), oconf.action_dim, **mk).items()}
        assert not fed['map'].is_floating_point() and host['map'].is_floating_point()
        with torch.no_grad():
            _, _, ma, ta, _ = model.training_step(fed, state, noise=noise)
            _, _, mb, tb, _ = model.training_step(host, state, noise=noise)
        for k in ('loss_map', 'acc_map', 'acc_map_seen'):
            assert float(ma[k]) == float(mb[k]), (k, float(ma[k]), float(mb[k]))
        assert torch.equal(ta['loss_map'], tb['loss_map']) and torch.equal(ta['acc_map'], tb['acc_map'])
    dr.close()
