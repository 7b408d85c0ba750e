"""CPU (-m "not gpu"): the host half of the device-resident replay (pydreamer_amd/replay.py DeviceReplay).

DeviceReplay.plan() turns the planner's windows into the two tables dm_replay_gather reads (pieces, byte offsets) plus the
cached episodes they refer to.  `_gather` below is a numpy restatement of that kernel, BYTE-wise and driven by nothing but the
tables: what it assembles must equal - exactly, every field, every batch - the reference-written batches of
tests/golden/replay_reader.npz for all seven reader configurations, what ReplayFeed.fill writes into a slot, and for the map
fields the raw window plus preprocess_batch's mask and coord.  The cache's eviction must never drop an episode a cursor, a tail
or a plan still holds."""
import os

import numpy as np
import pytest

from pydreamer_amd import replay as R

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'replay_reader.npz')
CASES = ['default', 'no_skip_first', 'mid_reset', 'random_resets', 'random_resets_mid', 'buffer_size', 'long_window']


def _gather(dr, plan):
    """csrc/replay_gather.hip in numpy: destination row t*B + b of field f <- bytes of row start + t' of piece p of column b."""
    out = {k: np.zeros(shape, dt) for k, (shape, dt) in dr.spec().items()}
    T, B = out['reset'].shape
    for b in range(B):
        t = 0
        for p in range(2):
            start, n, mark = (int(v) for v in plan.pieces[b, p])
            if n == 0:
                assert p == 1 and plan.episodes[b][p] is None
                continue
            flat = np.asarray(plan.episodes[b][p].host).view(np.uint8)
            for f, k in enumerate(dr.names):
                rb, off = dr.row_bytes[k], int(plan.offsets[b, p, f])
                assert off % 16 == 0
                rows = flat[off + start * rb:off + (start + n) * rb].reshape(n, rb)
                out[k].reshape(T, B, -1).view(np.uint8).reshape(T, B, rb)[t:t + n, b] = rows
            if mark:
                out['reset'][t, b] = True
            t += n
        assert t == T
    return out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


@pytest.fixture
def gold_repo(gold, tmp_path):
    for i, name in enumerate(gold['episode_files']):
        d = {k.split('/', 1)[1]: gold[k] for k in gold.files if k.startswith(f'episode{i}/')}
        np.savez_compressed(os.path.join(str(tmp_path), str(name)), **d)
    return R.LocalEpisodeRepository(str(tmp_path))


@pytest.mark.parametrize('case', CASES)
def test_plan_tables_reproduce_reference_batches(gold, gold_repo, case):
    kw = eval(str(gold[f'case/{case}/kwargs']))                           # a dict literal written by the generator
    seed = int(gold[f'case/{case}/seed'])
    clip = str(gold[f'case/{case}/clip_rewards']) or None
    A = int(gold['action_dim'])
    dr = R.DeviceReplay(R.SequentialReplay(gold_repo, seed=seed, **kw), A, clip_rewards=clip)
    feed = R.ReplayFeed(R.SequentialReplay(gold_repo, seed=seed, **kw), A, clip_rewards=clip)
    assert dr.spec() == feed.spec()
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in feed.spec().items()}
    nb = gold[f'case/{case}/raw/reward'].shape[0]
    for i in range(nb):
        plan = dr.plan()
        assert plan.pieces.dtype == np.int32 and plan.pieces.shape == (kw['batch_size'], 2, 3)
        assert plan.offsets.dtype == np.int64 and plan.offsets.shape == (kw['batch_size'], 2, len(dr.names))
        got = _gather(dr, plan)
        assert np.array_equal(got['image'], gold[f'case/{case}/raw/image'][i]), (case, i)
        for k in ('action', 'action_next', 'reward', 'terminal', 'reset'):
            want = gold[f'case/{case}/prep/{k}'][i]
            assert got[k].dtype == want.dtype and np.array_equal(got[k], want), (case, i, k)
        _same(got, feed.fill(slot), (case, i))


def _map_episode(n, ep, rs, seen_key, S=5, C=4):
    d = dict(image=rs.randint(0, 256, (n, 8, 8, 3)).astype(np.uint8), action=rs.randint(0, 3, n),
             reward=(ep * 1000 + np.arange(n)).astype(np.float32), terminal=np.zeros(n, bool), reset=np.zeros(n, bool),
             vecobs=rs.randn(n, 7),
             map=rs.randint(0, C, (n, S, S)).astype(np.uint8), agent_pos=rs.rand(n, 2) * S, agent_dir=rs.randn(n, 2))
    if seen_key == 'map_seen':
        d['map_seen'] = (d['map'] * (rs.rand(n, S, S) < 0.5)).astype(np.uint8)
    elif seen_key == 'map_vis':
        d['map_vis'] = rs.randint(0, 1000, (n, S, S))
    return d


@pytest.mark.parametrize('seen_key', ['map_seen', 'map_vis', None])
def test_map_fields_of_both_feeds(tmp_path, seen_key):
    """map = the raw class-map window; map_seen_mask / map_coord = preprocess_batch's, dtype included; one-hot of the carried map
    = preprocess_batch's map."""
    rs = np.random.RandomState(2)
    repo = R.LocalEpisodeRepository(str(tmp_path))
    for ep, n in enumerate([19, 26, 33]):
        repo.save_data(_map_episode(n, ep + 1, rs, seen_key), ep, ep)
    kw = dict(batch_length=6, batch_size=3, allow_mid_reset=True, reset_interval=8, seed=3)
    mk = dict(map_key='map', map_categorical=4)
    plain = iter(R.SequentialReplay(repo, **kw))
    dr = R.DeviceReplay(R.SequentialReplay(repo, **kw), 3, clip_rewards='log1p', **mk)
    feed = R.ReplayFeed(R.SequentialReplay(repo, **kw), 3, clip_rewards='log1p', **mk)
    assert dr.spec() == feed.spec()
    assert ('map_seen_mask' in dr.spec()) == (seen_key is not None) and 'map_coord' in dr.spec() and 'vecobs' in dr.spec()
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in feed.spec().items()}
    for i in range(12):
        raw = next(plain)
        want = R.preprocess_batch(raw, 3, clip_rewards='log1p', **mk)
        onehot = want.pop('map')
        want['map'] = raw['map']
        for got in (_gather(dr, dr.plan()), feed.fill(slot)):
            _same(got, want, (seen_key, i))
            assert np.array_equal(np.eye(4, dtype=np.float32)[got['map']].transpose(0, 1, 4, 2, 3), onehot)
    # without map_key nothing changes; a map that is not categorical is refused by both feeds
    assert 'map' not in R.ReplayFeed(R.SequentialReplay(repo, **kw), 3).spec()
    for cls in (R.ReplayFeed, R.DeviceReplay):
        with pytest.raises(ValueError, match='categorical'):
            cls(R.SequentialReplay(repo, **kw), 3, map_key='map')


def test_files_without_terminal_image_t_and_stored_onehot_actions(tmp_path):
    rs = np.random.RandomState(5)
    repo = R.LocalEpisodeRepository(str(tmp_path))
    for ep, n in enumerate([30, 40, 26]):
        d = _map_episode(n, ep + 1, rs, None)
        d['action'] = np.eye(3, dtype=np.float32)[d['action']]          # stored one-hot
        if ep == 0:
            del d['terminal']
        else:
            d['terminal'][-1] = True
        if ep == 1:
            d['image_t'] = d.pop('image').transpose(1, 2, 3, 0)
        repo.save_data(d, ep, ep)
    kw = dict(batch_length=8, batch_size=2, allow_mid_reset=True, seed=5)
    dr = R.DeviceReplay(R.SequentialReplay(repo, **kw), 3, clip_rewards='tanh')
    feed = R.ReplayFeed(R.SequentialReplay(repo, **kw), 3, clip_rewards='tanh')
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in feed.spec().items()}
    seen = 0.0
    for i in range(30):
        got = _gather(dr, dr.plan())
        _same(got, feed.fill(slot), i)
        seen += float(got['terminal'].sum())
    assert seen > 0


def test_lru_eviction_never_drops_a_held_episode(gold, gold_repo):
    """A budget of about one and a half files: the cache evicts all the time, yet every episode a cursor, a carried tail or the
    planned batch refers to keeps its data, the batches stay those of ReplayFeed, and the cache itself respects the budget (or
    is down to its newest entry)."""
    kw = dict(batch_length=10, batch_size=3, allow_mid_reset=True, reset_interval=20, seed=9)
    A = int(gold['action_dim'])
    free = R.DeviceReplay(R.SequentialReplay(gold_repo, **kw), A)
    feed = R.ReplayFeed(R.SequentialReplay(gold_repo, **kw), A)
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in feed.spec().items()}
    sizes = []
    for _ in range(40):
        plan = free.plan()
        sizes += [e.nbytes for e in plan.entries()]
    assert len(free._cache) <= len(free.replay.files) and free.cached_bytes == sum(e.nbytes for e in free._cache.values())
    budget = int(1.5 * max(sizes))
    dr = R.DeviceReplay(R.SequentialReplay(gold_repo, **kw), A, capacity_bytes=budget)
    generations = {}
    for i in range(40):
        plan = dr.plan()
        held = plan.entries() + [c.episode.entry for c in dr.replay.columns if c.episode is not None] \
            + [c.tail[0].entry for c in dr.replay.columns if c.tail is not None]
        for e in held:
            assert e.host is not None and e.reset is not None
            generations.setdefault(e.path, set()).add(id(e))
        assert dr.cached_bytes <= budget or len(dr._cache) == 1
        assert dr.cached_bytes == sum(e.nbytes for e in dr._cache.values())
        _same(_gather(dr, plan), feed.fill(slot), i)
    assert max(len(v) for v in generations.values()) > 1, 'nothing was evicted and read again'


def test_the_planner_hook_defaults_to_a_fresh_read(gold_repo):
    """SequentialReplay.load_episode / plan_batch: the default hook reads the file afresh, and plan_batch() + _copy is fill()."""
    a = R.SequentialReplay(gold_repo, 10, 2, allow_mid_reset=True, seed=4)
    b = R.SequentialReplay(gold_repo, 10, 2, allow_mid_reset=True, seed=4)
    seen = []
    c = R.SequentialReplay(gold_repo, 10, 2, allow_mid_reset=True, seed=4,
                           load_episode=lambda info: seen.append(info.path) or R._Episode(info.load_data()))
    for _ in range(10):
        want = a.fill()
        plans = b.plan_batch()
        assert len(plans) == 2 and all(sum(z - s for _, s, z in ps) == 10 for ps in plans)
        got = c.fill()
        for k in want:
            assert np.array_equal(got[k], want[k])
    assert len(seen) >= 2 and isinstance(a.load_episode(a.files[0]), R._Episode)


def test_device_replay_refuses_what_it_cannot_feed(gold_repo, tmp_path):
    used = R.SequentialReplay(gold_repo, 10, 2, seed=0)
    used.fill()
    with pytest.raises(ValueError, match='nothing has been drawn'):
        R.DeviceReplay(used, 4)
    with pytest.raises(ValueError):
        R.DeviceReplay(R.SequentialReplay(gold_repo, 10, 2), 4, clip_rewards='sqrt')
    (tmp_path / 'nothing').mkdir()
    empty = R.LocalEpisodeRepository(str(tmp_path / 'nothing'))
    with pytest.raises(ValueError, match='empty'):
        R.DeviceReplay(R.SequentialReplay(empty, 8, 2, check_nonempty=False), 4)
    with pytest.raises(ValueError, match='without a device'):
        R.DeviceReplay(R.SequentialReplay(gold_repo, 10, 2), 4).next()


def test_gather_entry_point_checks_its_arguments_on_the_host(hip):
    """dm_replay_gather validates what it can see on the host and returns DM_E_* with a message: no launch, no GPU needed."""
    import ctypes
    P = ctypes.c_void_p
    f = (hip.dm_replay_field * 2)()
    f[0].dst, f[0].row_bytes, f[0].is_reset = 4096, 12288, 0
    f[1].dst, f[1].row_bytes, f[1].is_reset = 8192, 1, 1
    bad = [((0, 1, 2, f, P(64), P(64), None), 'bad shape'), ((1, 1, 0, f, P(64), P(64), None), 'fields'),
           ((1, 1, 17, f, P(64), P(64), None), 'fields'), ((1, 1, 2, f, None, P(64), None), 'null'),
           ((1, 1, 2, f, P(64), None, None), 'null'), ((1, 1, 2, None, P(64), P(64), None), 'null'),
           ((1, 1, 2, f, P(66), P(64), None), 'aligned'), ((1, 1, 2, f, P(64), P(68), None), 'aligned')]
    for args, word in bad:
        with pytest.raises(hip.DreamerHipError, match=word):
            hip.call('dm_replay_gather', *args)
    f[0].dst = 4100
    with pytest.raises(hip.DreamerHipError, match='16-byte'):
        hip.call('dm_replay_gather', 1, 1, 2, f, P(64), P(64), None)
    f[0].dst, f[1].row_bytes = 4096, 4
    with pytest.raises(hip.DreamerHipError, match='reset column'):
        hip.call('dm_replay_gather', 1, 1, 2, f, P(64), P(64), None)
    f[1].row_bytes, f[0].row_bytes = 1, 0
    with pytest.raises(hip.DreamerHipError, match='bytes per row'):
        hip.call('dm_replay_gather', 1, 1, 2, f, P(64), P(64), None)
    f[0].row_bytes, f[0].is_reset = 1, 1
    with pytest.raises(hip.DreamerHipError, match='flagged'):
        hip.call('dm_replay_gather', 1, 1, 2, f, P(64), P(64), None)
    assert ctypes.sizeof(hip.dm_replay_field) == 24 and hip.DM_REPLAY_MAX_FIELDS == 16
