"""A small repository of MiniGrid-like episode files, shared by tests/test_class_image_feeds_cpu.py and
tests/test_gpu_class_image_feeds.py: the observation is an integer class image (n,S,S) uint8 in [0,4), beside a class map
(n,5,5), `map_seen`, agent_pos / agent_dir and integer actions.  Four files of 6, 7, 9 and 12 rows, read at T=5, B=3 with
allow_mid_reset (two-piece columns: no file is a multiple of 5 rows long) and reset_interval=11 (only the 12-row file can draw an
artificial reset: 12 // 11 + 1 = 2 spans of 5 rows fit in it, one span in every other file)."""
import numpy as np

from pydreamer_amd import replay as R

ROWS = (6, 7, 9, 12)
CLASSES, ACTIONS, MAP_SIZE, MAP_CLASSES = 4, 7, 5, 4
T, B = 5, 3
READER = dict(batch_length=T, batch_size=B, allow_mid_reset=True, reset_interval=11)
SEED = 5          # with this seed the first three batches hold a two-piece column AND an artificial reset mark (asserted by the tests)
FEED = dict(image_categorical=CLASSES, map_key='map', map_categorical=MAP_CLASSES)


def episode(n, ep, rs, S):
    m = rs.randint(0, MAP_CLASSES, (n, MAP_SIZE, MAP_SIZE)).astype(np.uint8)
    return dict(image=rs.randint(0, CLASSES, (n, S, S)).astype(np.uint8), action=rs.randint(0, ACTIONS, n),
                reward=(ep + 0.01 * np.arange(n)).astype(np.float32), terminal=np.arange(n) == n - 1, reset=np.zeros(n, bool),
                map=m, map_seen=(m * (rs.rand(n, MAP_SIZE, MAP_SIZE) < 0.5)).astype(np.uint8),
                agent_pos=rs.rand(n, 2) * MAP_SIZE, agent_dir=rs.randn(n, 2))


def write(dirpath, S=7):
    """The four files under `dirpath`; returns the repository."""
    rs = np.random.RandomState(100 + S)
    repo = R.LocalEpisodeRepository(str(dirpath))
    for ep, n in enumerate(ROWS):
        repo.save_data(episode(n, ep + 1, rs, S), ep, ep)
    return repo


def reference_batches(repo, count, seed=SEED):
    """`count` consecutive batches as preprocess_batch hands them over, with the two fields the feeds carry as stored put beside
    their one-hot forms: [(expected feed batch, one-hot image, one-hot map)]."""
    plain = iter(R.SequentialReplay(repo, seed=seed, **READER))
    out = []
    for _ in range(count):
        raw = next(plain)
        want = R.preprocess_batch(raw, ACTIONS, **FEED)
        image, map_ = want['image'], want['map']
        want['image'], want['map'] = image.argmax(2).astype(raw['image'].dtype), raw['map']
        assert np.array_equal(want['image'], raw['image'])
        out.append((want, image, map_))
    return out


def same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(got[k], want[k]), (what, k)
