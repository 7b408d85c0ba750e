"""CPU (-m "not gpu"): integer class-map frames through the feeds (image_categorical = C; the `minigrid` section).

The repository of tests/class_image_repo.py in tmp_path: four files of 6, 7, 9 and 12 rows with `image` (n,7,7) uint8 in [0,4), read
at T=5, B=3.  For three consecutive batches ReplayFeed.fill and DeviceReplay(device=None).plan() - resolved on the host by the numpy
restatement of dm_replay_gather in tests/test_device_replay_cpu.py - both equal preprocess_batch field for field, `image` being the
argmax over the class axis of its one-hot.  Also: spec(), both constructor refusals, and a file holding class 4 passed over."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_image_repo as CR                        # noqa: E402
from test_device_replay_cpu import _gather           # noqa: E402
from pydreamer_amd import replay as R                # noqa: E402


def _replay(repo):
    return R.SequentialReplay(repo, seed=CR.SEED, **CR.READER)


def test_both_feeds_equal_preprocess_batch(tmp_path):
    repo = CR.write(tmp_path)
    feed = R.ReplayFeed(_replay(repo), CR.ACTIONS, **CR.FEED)
    dr = R.DeviceReplay(_replay(repo), CR.ACTIONS, **CR.FEED)
    spec = feed.spec()
    assert dr.spec() == spec
    assert spec['image'] == ((CR.T, CR.B, 7, 7), np.uint8) and spec['map'] == ((CR.T, CR.B, 5, 5), np.uint8)
    assert dr.row_bytes['image'] == 49
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in spec.items()}
    two_piece = marked = False
    for i, (want, onehot, _) in enumerate(CR.reference_batches(repo, 3)):
        plan = dr.plan()
        two_piece |= bool((plan.pieces[:, 1, 1] > 0).any())
        marked |= bool(plan.pieces[:, :, 2].any())
        for who, got in (('ReplayFeed', feed.fill(slot)), ('DeviceReplay', _gather(dr, plan))):
            CR.same(got, want, (who, i))
            assert got['image'].shape == (CR.T, CR.B, 7, 7) and got['image'].dtype == np.uint8
            assert np.array_equal(got['image'], onehot.argmax(2))
            assert np.array_equal(np.eye(CR.CLASSES, dtype=np.float32)[got['image']].transpose(0, 1, 4, 2, 3), onehot)
    assert two_piece and marked, 'the three batches must hold a two-piece column and an artificial reset mark'


def test_stored_dtype_is_carried(tmp_path):
    """An int64 class image stays int64 in the slot (as `map` does): 392-byte rows."""
    rs = np.random.RandomState(1)
    repo = R.LocalEpisodeRepository(str(tmp_path))
    for ep, n in enumerate(CR.ROWS):
        d = CR.episode(n, ep + 1, rs, 7)
        d['image'] = d['image'].astype(np.int64)
        repo.save_data(d, ep, ep)
    feed = R.ReplayFeed(_replay(repo), CR.ACTIONS, **CR.FEED)
    dr = R.DeviceReplay(_replay(repo), CR.ACTIONS, **CR.FEED)
    assert feed.spec()['image'] == ((CR.T, CR.B, 7, 7), np.int64) and dr.row_bytes['image'] == 392
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in feed.spec().items()}
    for i, (want, _, _) in enumerate(CR.reference_batches(repo, 2)):
        CR.same(feed.fill(slot), want, ('ReplayFeed', i))
        CR.same(_gather(dr, dr.plan()), want, ('DeviceReplay', i))


def test_constructor_refusals(tmp_path):
    classes, frames = tmp_path / 'classes', tmp_path / 'frames'
    classes.mkdir(), frames.mkdir()
    repo = CR.write(classes)
    rs = np.random.RandomState(2)
    urepo = R.LocalEpisodeRepository(str(frames))
    for ep, n in enumerate(CR.ROWS):
        d = CR.episode(n, ep + 1, rs, 7)
        d['image'] = rs.randint(0, 256, (n, 8, 8, 3)).astype(np.uint8)
        urepo.save_data(d, ep, ep)
    for cls in (R.ReplayFeed, R.DeviceReplay):
        # integer (n,H,W) frames, image_categorical unset: the message names both facts
        with pytest.raises(ValueError, match=r'uint8 \(12, 7, 7\).*image_categorical.*not set'):
            cls(_replay(repo), CR.ACTIONS)
        # uint8 (n,H,W,C) frames, image_categorical set
        with pytest.raises(ValueError, match=r'image_categorical=4.*uint8 \(12, 8, 8, 3\)'):
            cls(_replay(urepo), CR.ACTIONS, image_categorical=4)
        # unset on uint8 frames: as before
        assert cls(_replay(urepo), CR.ACTIONS).spec()['image'] == ((CR.T, CR.B, 8, 8, 3), np.uint8)
    # float frames keep today's message
    d = CR.episode(6, 9, rs, 7)
    d['image'] = d['image'].astype(np.float32)
    frepo = R.LocalEpisodeRepository(str(tmp_path / 'floats'))
    os.mkdir(frepo.dirs[0])
    frepo.save_data(d, 0, 0)
    with pytest.raises(ValueError, match=r'^expected uint8 \(T,H,W,C\) frames in the episode files, got float32 \(6, 7, 7\)$'):
        R.ReplayFeed(_replay(frepo), CR.ACTIONS)


def test_device_replay_passes_over_a_file_with_a_class_out_of_range(tmp_path, capsys):
    """DeviceReplay._prepare checks [0, C) once per file; the file is passed over like one of another layout and never appears in a
    plan.  ReplayFeed.fill does not check (the hot path) and hands the class on as stored."""
    repo = CR.write(tmp_path)
    d = CR.episode(12, 7, np.random.RandomState(3), 7)
    d['image'][5, 3, 3] = 4
    bad = os.path.basename(repo.save_data(d, 9, 9))          # (the newest file: the one the slots are laid out from - shapes only)
    dr = R.DeviceReplay(_replay(repo), CR.ACTIONS, **CR.FEED)
    used = set()
    for _ in range(12):
        plan = dr.plan()
        got = _gather(dr, plan)
        assert int(got['image'].max()) < CR.CLASSES
        used |= {os.path.basename(e.path) for e in plan.entries()}
    assert bad not in used and len(used) == 4
    assert bad in capsys.readouterr().out, 'the planner reports the file it passed over'
    feed = R.ReplayFeed(_replay(repo), CR.ACTIONS, **CR.FEED)
    slot = {k: np.zeros(shape, dt) for k, (shape, dt) in feed.spec().items()}
    assert max(int(feed.fill(slot)['image'].max()) for _ in range(12)) == 4
