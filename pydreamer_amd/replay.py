"""Replay reader -> device ring: the caller side of the hot path.

The reference feeds `train.py` from `DataSequential` (data.py:128-304: B independent episode streams cut into
truncated-BPTT windows of `batch_length`, files chosen at random forever) through `Preprocessor.apply`
(preprocessing.py:87-180) in DataLoader workers, and the trainer moves every batch to the device as float32.
Here the same batches are produced as what the HIP path consumes directly:

  * `LocalEpisodeRepository`  - episode `.npz` files in local directories (the reference lists mlflow artifacts,
    data.py:53-122; the file-name grammar `ep{from}_{to}-r{reward}-{steps}.npz` is the same);
  * `SequentialReplay`        - a window planner: per batch column a cursor (episode, row) that cuts consecutive
    `batch_length`-row windows, planned as (episode, start, stop) pieces and copied once, straight into the (T, B, ...) arrays
    the caller hands it (the pinned slot of the device ring).  Same batches as DataSequential for the same files, arguments and
    seed (random start in a column's first file, tails carried into the next file with `allow_mid_reset`, artificial resets
    every `reset_interval`, `buffer_size` / `reload_interval` file selection); the random stream is an explicit
    `numpy.random.RandomState` (the reference uses the global one);
  * `ReplayFeed`              - planner + preprocessing writing IN PLACE into a ring slot; with image_categorical = C the frames
    are the files' integer class image (n,H,W), carried as stored (the `minigrid` section);
  * `preprocess_batch`        - the hot-path subset of Preprocessor.apply: one-hot float32 actions, float32 reward with
    `clip_rewards`, float32 terminal, bool reset - and the image is LEFT AS uint8 (T,B,H,W,C): x/255-0.5 and HWC->CHW
    happen inside the first conv's patch loader on the GPU (N1), so a batch crosses PCIe at 1 byte per pixel value;
  * `DeviceRing`              - a background thread fills pinned host buffers; the consumer enqueues the H2D copies on its
    own stream at a point where that stream is idle (`prefetch()` after `training_step()`), into a ring of device batches;
  * `DeviceReplay`            - the same batches from episodes kept RESIDENT on the device: the planner's windows become two
    small tables and one gather launch (csrc/replay_gather.hip), so a file's frames cross PCIe once, not once per visit.

parity: pinned against the reference's own DataSequential + Preprocessor run in the build container
(oracle/gen_replay_golden.py -> tests/golden/replay_reader.npz; tests/test_replay_cpu.py replays it: same episode files,
same arguments, same seed of numpy's legacy random stream => identical batches, byte for byte, for 7 reader configurations).
The limits of that pin, as the generator's header states them: data.py imports mlflow at module scope and mlflow is absent,
so the import statements were satisfied with empty placeholder modules (nothing in them is called), and the episode source
was a local subclass of the reference's abstract EpisodeRepository instead of MlflowEpisodeRepository.  `DeviceRing` has no
reference counterpart (the reference uses a DataLoader + `.to(device)`) and is covered by its own tests.
"""
import ctypes
import os
import queue
import threading
import time
from dataclasses import dataclass

import numpy as np
import torch


@dataclass
class FileInfo:
    path: str
    episode_from: int
    episode_to: int
    steps: int

    def load_data(self):
        with open(self.path, 'rb') as f:
            fdata = np.load(f)
            return {k: fdata[k] for k in fdata}


def parse_episode_name(fname):
    """data.py:103-122."""
    fname = os.path.basename(fname).split('.')[0]
    steps = fname.split('-')[-1]
    steps = int(steps) if steps.isnumeric() else 0
    if fname.startswith('ep'):
        body = fname.split('ep')[1].split('-')[0]
        ep_from, ep_to = body.split('_')[0], body.split('_')[-1]
        return (int(ep_from) if ep_from.isnumeric() else 0, int(ep_to) if ep_to.isnumeric() else 0, steps)
    return (0, 0, steps)


class LocalEpisodeRepository:
    def __init__(self, dirs):
        self.dirs = [dirs] if isinstance(dirs, str) else list(dirs)

    def list_files(self):
        files = []
        for d in self.dirs:
            for name in sorted(os.listdir(d)):
                if name.endswith('.npz'):
                    a, b, steps = parse_episode_name(name)
                    files.append(FileInfo(os.path.join(d, name), a, b, steps))
        return files

    def count_steps(self):
        """data.py:90-94: (files, steps, episodes) of the repository."""
        files = self.list_files()
        return len(files), sum(f.steps for f in files), (max(f.episode_to for f in files) + 1) if files else 0

    @staticmethod
    def build_episode_name(episode_from, episode, reward, steps, chunk_seq=None):
        """data.py:97-101 (chunk_seq: the generator's sequence number of a partial episode file)."""
        if chunk_seq is None:
            return f'ep{episode_from:06}_{episode:06}-r{reward:.0f}-{steps:04}.npz'
        return f'ep{episode_from:06}_{episode:06}-{chunk_seq}-r{reward:.0f}-{steps:04}.npz'

    def save_data(self, data, episode_from, episode_to, chunk_seq=None):
        """data.py:62-69 naming; written with np.savez_compressed like tools.py:200-207."""
        n_episodes = int(data['reset'].sum())
        steps = len(data['reset']) - n_episodes
        name = self.build_episode_name(episode_from, episode_to, float(data['reward'].sum()), steps, chunk_seq)
        path = os.path.join(self.dirs[0], name)
        np.savez_compressed(path, **data)
        return path


class _Episode:
    """One episode file, prepared once: frames as (T,H,W,C) (the generator may store them time-last, data.py:237-239), the
    action that FOLLOWS each step, and the two per-file fix-ups of data.py:256-260 (a file starts with a reset and carries no
    reward on its first row).  `marks` flags the rows where a window gets an artificial reset (scatter_resets)."""
    __slots__ = ('fields', 'rows', 'marks')

    def __init__(self, arrays):
        if 'image' not in arrays and 'image_t' in arrays:
            arrays['image'] = arrays.pop('image_t').transpose(3, 0, 1, 2)
        arrays['action_next'] = np.concatenate([arrays['action'][1:], np.zeros_like(arrays['action'][:1])])
        self.rows = arrays['reward'].shape[0]
        reset = arrays['reset'].copy() if 'reset' in arrays else np.zeros(self.rows, bool)
        reward = arrays['reward'].copy()
        reset[0], reward[0] = True, 0.0
        arrays['reset'], arrays['reward'] = reset, reward
        self.fields = arrays
        self.marks = None


class _Column:
    """Cursor of one batch column: where in which episode its next window starts, how long that window is (a window that
    completes a carried tail is shorter), and the tail of the previous episode waiting to be completed."""
    __slots__ = ('episode', 'pos', 'want', 'tail', 'random_start')

    def __init__(self, random_start):
        self.episode, self.pos, self.want, self.tail, self.random_start = None, 0, 0, None, random_start


class SequentialReplay:
    """Truncated-BPTT window planner over episode files: every batch column walks its own random sequence of episodes and
    cuts consecutive windows of `batch_length` rows out of them, so the recurrent state a trainer carries from batch to batch
    (train.py:168-178) stays aligned with the data.  The batches are those of the reference's DataSequential (data.py:128-304)
    BYTE FOR BYTE for the same files, arguments and seed of numpy's legacy random stream - it draws in the same order: file
    choice, random start inside a column's first file, reset scatter of the file - which tests/test_replay_cpu.py checks
    against batches written by the reference itself.

    What is different is where the rows go.  A window is planned as one or two (episode, start, stop) pieces and copied ONCE,
    straight into the (T, B, ...) arrays the caller hands to `fill()` - for the training loop the pinned slot of the device
    ring (`ReplayFeed`), from where the frames cross PCIe as uint8 - instead of slice dicts -> np.concatenate -> np.stack ->
    another copy.  `__iter__` (tests, small tools) allocates fresh arrays per batch and fills those."""

    def __init__(self, repository, batch_length, batch_size, skip_first=True, reload_interval=0, buffer_size=0, reset_interval=0,
                 allow_mid_reset=False, seed=0, check_nonempty=True, load_episode=None):
        self.repository = repository
        # how a chosen file becomes an episode object (`fields`, `rows`, `marks`): by default read and prepared afresh on every
        # visit; DeviceReplay installs its cache here.  Called once per visit, after the draw that chose the file.
        self.load_episode = load_episode or (lambda info: _Episode(info.load_data()))
        self.batch_length, self.batch_size = int(batch_length), int(batch_size)
        self.buffer_size = buffer_size                       # keep the newest files whose step counts fit (0: all)
        self.reload_interval = reload_interval               # seconds between re-listings of the repository (online training)
        self.reset_interval, self.allow_mid_reset = reset_interval, allow_mid_reset
        self.rs = np.random.RandomState(seed)
        self.columns = [_Column(bool(skip_first)) for _ in range(self.batch_size)]
        self.relist()
        if check_nonempty and not self.files:
            raise ValueError(f'no episode files in {getattr(repository, "dirs", repository)}')

    # ---- which files are in play
    def relist(self):
        listed = sorted(self.repository.list_files(), key=lambda f: -f.episode_to)      # newest first (data.py:164)
        kept, steps = [], 0
        for f in listed:
            steps += f.steps
            if not self.buffer_size or steps < self.buffer_size:
                kept.append(f)
        self.files, self.listed_steps, self.listed_at = kept, steps, time.time()

    def relist_due(self):
        return bool(self.reload_interval) and time.time() - self.listed_at > self.reload_interval

    # the names the reference trainer reads on its DataSequential (train.py:68-79, 227-229; data.py:147-170)
    @property
    def stats_steps(self):
        return self.listed_steps

    reload_files = relist
    should_reload_files = relist_due

    # ---- artificial resets: a long episode is cut into 1..steps/interval+1 backprop spans at random window-aligned rows
    def scatter_resets(self, resets, reset_interval, batch_length):
        """Same draws, same result as data.py:280-300."""
        if not resets[0]:
            raise ValueError('an episode file must start with a reset')
        starts = np.flatnonzero(resets).tolist() + [len(resets)]
        marks = np.zeros_like(resets)
        for a, b in zip(starts[:-1], starts[1:]):
            spans = self.rs.randint(1, (b - a) // reset_interval + 2)
            if spans > 1:
                gaps = np.sort(self.rs.choice(b - a - batch_length * spans, spans - 1))
                marks[a + gaps + np.arange(1, spans) * batch_length] = True
        return marks

    # ---- one column, one window
    def _open(self, col):
        """Next episode of a column: a random file; unreadable ones and ones shorter than a window are passed over (they cost
        the draw that chose them, nothing else)."""
        if self.relist_due():
            self.relist()
        info = self.files[self.rs.randint(len(self.files))]
        random_start, col.random_start = col.random_start, False
        try:
            ep = self.load_episode(info)
        except Exception as e:
            print('replay: skipping unreadable episode file', info.path, e)
            return
        L = self.batch_length
        if ep.rows < L:
            return
        col.pos = self.rs.randint(ep.rows - L + 1) if random_start else 0
        col.want = L - (col.tail[2] - col.tail[1]) if col.tail is not None else L
        ep.marks = self.scatter_resets(ep.fields['reset'], self.reset_interval, L) if self.reset_interval else None
        col.episode = ep

    def _plan(self, col):
        """The pieces [(episode, start, stop), ...] of the column's next window (their lengths add up to batch_length)."""
        while True:
            if col.episode is None:
                self._open(col)
                continue
            ep = col.episode
            if col.pos >= ep.rows:                           # the file ended on a window boundary
                col.episode = None
                continue
            stop = min(col.pos + col.want, ep.rows)
            piece = (ep, col.pos, stop)
            if stop - col.pos < col.want:                    # the file's last rows do not fill the window
                if col.tail is not None:
                    raise ValueError('an episode file is too short to complete the window carried over from the previous one')
                col.tail = piece if self.allow_mid_reset else None
                col.episode = None
                continue
            pieces = [piece] if col.tail is None else [col.tail, piece]
            col.tail, col.pos, col.want = None, stop, self.batch_length
            return pieces

    def _copy(self, pieces, out, b):
        t = 0
        for ep, a, z in pieces:
            n = z - a
            for k, dst in out.items():
                src = ep.fields.get(k)
                if src is None:
                    if k != 'terminal':
                        raise KeyError(f'an episode file lacks the field {k!r} the batch was laid out with')
                    dst[t:t + n, b] = 0                       # files written before `terminal` existed: no terminal rows
                else:
                    dst[t:t + n, b] = src[a:z]
            if ep.marks is not None and ep.marks[a:z].any():
                if ep.fields['reset'][a:z].any():
                    raise ValueError('an artificial reset fell into a window that holds a real one')
                out['reset'][t, b] = True                     # at the piece's first row: the longest backprop span
            t += n

    # ---- batches
    def plan_batch(self):
        """The planning half of fill(): per batch column the pieces [(episode, start, stop), ...] of its next window.  Advances
        the cursors and draws from the random stream exactly as fill() does; copies nothing."""
        return [self._plan(col) for col in self.columns]

    def fill(self, out=None):
        """Write the next batch into `out` ({key: (T, B, ...) array}; only the keys present are written - all of the files' keys
        when out is None or empty, in freshly allocated arrays).  Returns out."""
        plans = self.plan_batch()
        if not out:
            first = plans[0][0][0].fields
            out = {} if out is None else out
            for k, v in first.items():
                out[k] = np.empty((self.batch_length, self.batch_size) + v.shape[1:], v.dtype)
            if 'terminal' not in out:      # the first file predates `terminal` but another piece of this batch carries it: same
                for pieces in plans:       # column as ReplayFeed lays out (zeros for the files without it, _copy)
                    src = next((ep.fields['terminal'] for ep, _, _ in pieces if 'terminal' in ep.fields), None)
                    if src is not None:
                        out['terminal'] = np.empty((self.batch_length, self.batch_size) + src.shape[1:], src.dtype)
                        break
        for b, pieces in enumerate(plans):
            self._copy(pieces, out, b)
        return out

    def __iter__(self):
        while True:
            yield self.fill()


GOAL_SOURCES = ('targets_vec', 'target_vec')      # the files' fields behind goals_direction / goal_direction


def preprocess_batch(batch, action_dim, clip_rewards=None, image_key='image', map_key=None, map_categorical=None, goals=False,
                     image_categorical=None):
    """Hot-path subset of Preprocessor.apply (preprocessing.py:87-180), images left uint8 (T,B,H,W,C).
    image_categorical = C (preprocessing.py:108-109; the input of the dense categorical image path, models.dense_image_gate):
    `image` = the integer class image (T,B,H,W) as a one-hot (T,B,C,H,W) float32.  With the default the frames stay uint8.
    ReplayFeed / DeviceReplay(image_categorical=C) carry the class image as stored (integer (T,B,H,W): the argmax over the class
    axis of this one-hot), which the dense image path takes with the same bits.
    map_key / map_categorical (preprocessing.py:115-131,152-158; the inputs of the map probe, models.MapProbeHead): `map` =
    batch[map_key] as a one-hot (T,B,C,H,W) float32 with C = map_categorical, or - not categorical - a float image of that
    layout; `map_seen_mask` from `map_seen` or `map_vis`; `map_coord` (T,B,4) from `agent_pos`, `agent_dir` and the map's
    height.  Without map_key nothing of this is emitted.  ReplayFeed / DeviceReplay carry the class map as stored (integer
    (T,B,H,W), which MapProbeHead takes as it is) with the same mask and coord.
    goals=True (preprocessing.py:171-178; the targets of the goals probe, models.GoalsProbe): `goals_direction` = `targets_vec`
    (T,B,G,2) reshaped to (T,B,2G), `goal_direction` = `target_vec`, both float32, and `goals_visage` passed through as float32
    when the batch holds it.  With the default nothing of this is emitted.
    image_key=None (or ''; preprocessing.py:106, the `vectorenv` section): the result has no `image`; `vecobs` is float32 and the
    other fields are as always."""
    T, B = batch['reward'].shape[:2]
    out = {}
    img = batch[image_key] if image_key else None
    if not image_key:                                        # preprocessing.py:106: no `image` at all (an image-less world model)
        pass
    elif image_categorical:                                    # img_to_onehot (preprocessing.py:15-18)
        assert img.ndim == 4, f'expected a (T,B,H,W) class image under {image_key!r}, got {img.shape}'
        out['image'] = np.ascontiguousarray(np.eye(int(image_categorical), dtype=np.float32)[img].transpose(0, 1, 4, 2, 3))
    else:
        assert img.dtype == np.uint8 and img.ndim == 5, f'expected uint8 (T,B,H,W,C) frames, got {img.dtype} {img.shape}'
        out['image'] = np.ascontiguousarray(img)
    for k in ('action', 'action_next'):
        if k in batch:
            a = batch[k]
            if a.ndim == 2:
                a = np.eye(action_dim, dtype=np.float32)[a]
            assert a.ndim == 3
            out[k] = a.astype(np.float32)
    out['terminal'] = batch.get('terminal', np.zeros((T, B))).astype(np.float32)
    r = batch.get('reward', np.zeros((T, B))).astype(np.float32)
    if clip_rewards == 'tanh':
        r = np.tanh(r)
    elif clip_rewards == 'log1p':
        r = np.log1p(r)
    elif clip_rewards:
        raise ValueError(clip_rewards)
    out['reward'] = r
    out['reset'] = batch.get('reset', np.zeros((T, B), bool)).astype(bool)
    if 'vecobs' in batch:                                    # preprocessing.py:162-163
        out['vecobs'] = batch['vecobs'].astype(np.float32)
    if map_key:
        m = batch[map_key]
        if map_categorical:                                  # img_to_onehot (preprocessing.py:15-18)
            m = np.eye(int(map_categorical), dtype=np.float32)[m]
        elif m.dtype == np.uint8:                            # to_image (preprocessing.py:21-29)
            m = m.astype(np.float32) / 255.0 - 0.5
        else:
            assert 0.0 <= m[0, 0, 0, 0, 0] <= 1.0
            m = m.astype(np.float32)
        assert m.ndim == 5, f'expected a (T,B,H,W) class map or a (T,B,H,W,C) image under {map_key!r}, got {batch[map_key].shape}'
        out['map'] = np.ascontiguousarray(m.transpose(0, 1, 4, 2, 3))      # (T,B,H,W,C) => (T,B,C,H,W)
        if 'map_seen' in batch:                              # 0 where the cell is unseen, otherwise = map
            out['map_seen_mask'] = (batch['map_seen'] > 0).astype(int)
        elif 'map_vis' in batch:                             # steps since the cell was seen; never: max_steps = 500
            out['map_seen_mask'] = (batch['map_vis'] < 500).astype(int)
        if 'agent_pos' in batch and 'agent_dir' in batch:
            pos = batch['agent_pos'] / float(out['map'].shape[-2]) * 2 - 1.0
            out['map_coord'] = np.concatenate([pos, batch['agent_dir']], axis=-1).astype(np.float32)
    if goals:
        _require_goal_sources(batch, 'the batch')
        out.update(_goal_fields(batch))
    return out


def _require_goal_sources(fields, what):
    missing = [k for k in GOAL_SOURCES if k not in fields]
    if missing:
        raise ValueError(f'goals=True: {what} holds no {" / ".join(missing)} (the sources of goals_direction / goal_direction)')


def _goal_fields(fields):
    """preprocess_batch's goal fields of raw fields (any leading dimensions): (*,G,2) => (*,2G), float32."""
    tv = fields['targets_vec']
    out = {'goals_direction': tv.reshape(tv.shape[:-2] + (-1,)).astype(np.float32),
           'goal_direction': fields['target_vec'].astype(np.float32)}
    if 'goals_visage' in fields:
        out['goals_visage'] = fields['goals_visage'].astype(np.float32)
    return out


def _map_seen_mask(fields):
    """preprocess_batch's map_seen_mask of raw fields (any leading dimensions), or None when the files carry neither source."""
    if 'map_seen' in fields:
        return (fields['map_seen'] > 0).astype(int)
    if 'map_vis' in fields:
        return (fields['map_vis'] < 500).astype(int)
    return None


def _map_coord(fields, height):
    """preprocess_batch's map_coord of raw fields (any leading dimensions)."""
    pos = fields['agent_pos'] / float(height) * 2 - 1.0
    return np.concatenate([pos, fields['agent_dir']], axis=-1).astype(np.float32)


def _map_spec(probe, lead, map_key, map_categorical):
    """{field: (shape, dtype)} of the map probe's inputs as the feeds carry them; `probe`: the raw fields of one episode."""
    if not map_categorical:
        raise ValueError('the feeds carry categorical maps only (map_categorical = number of classes); a float map goes through '
                         'preprocess_batch')
    m = probe[map_key]
    if m.ndim != 3 or not np.issubdtype(m.dtype, np.integer):
        raise ValueError(f'expected an integer (T,H,W) class map under {map_key!r}, got {m.dtype} {m.shape}')
    spec = {'map': (lead + m.shape[1:], m.dtype.type)}
    seen = _map_seen_mask({k: probe[k][:1] for k in ('map_seen', 'map_vis') if k in probe})
    if seen is not None:
        spec['map_seen_mask'] = (lead + seen.shape[1:], seen.dtype.type)
    if 'agent_pos' in probe and 'agent_dir' in probe:
        spec['map_coord'] = (lead + (probe['agent_pos'].shape[-1] + probe['agent_dir'].shape[-1],), np.float32)
    return spec


def _feed_layout(replay, action_dim, image_key, map_key, map_categorical, who, goals=False, image_categorical=None):
    """(raw fields of the repository's first file, {field: ((T, B, ...) shape, dtype)} of a batch as the feeds hand it over).
    image_categorical = C: the files hold an integer class image (n,H,W), carried as stored (T,B,H,W), not one-hot."""
    if not replay.files:
        raise ValueError(f'{who} needs at least one episode file to lay out its slots (the repository is empty)')
    probe = _Episode(replay.files[0].load_data()).fields      # shapes only; draws nothing from the random stream
    T, B = replay.batch_length, replay.batch_size
    spec = {}
    if image_key and image_categorical:
        img = probe[image_key]
        if img.ndim != 3 or not np.issubdtype(img.dtype, np.integer):
            raise ValueError(f'image_categorical={image_categorical}: expected an integer (T,H,W) class image in the episode files, '
                             f'got {img.dtype} {img.shape}')
        spec['image'] = ((T, B) + img.shape[1:], img.dtype.type)
    elif image_key:
        img = probe[image_key]
        if img.dtype != np.uint8 or img.ndim != 4:
            hint = ''
            if img.ndim == 3 and np.issubdtype(img.dtype, np.integer):
                hint = ' - an integer (T,H,W) class image, and image_categorical (the number of classes) is not set'
            raise ValueError(f'expected uint8 (T,H,W,C) frames in the episode files, got {img.dtype} {img.shape}' + hint)
        spec['image'] = ((T, B) + img.shape[1:], np.uint8)
    elif 'vecobs' not in probe:      # image_key=None: an image-less world model, whose only observation is the vector
        raise ValueError(f"{who}(image_key=None): the episode files hold no 'vecobs' field - the only observation of an image-less "
                         'world model')
    spec.update({'action': ((T, B, action_dim), np.float32),
                 'action_next': ((T, B, action_dim), np.float32), 'terminal': ((T, B), np.float32),
                 'reward': ((T, B), np.float32), 'reset': ((T, B), np.bool_)})
    if 'vecobs' in probe:
        spec['vecobs'] = ((T, B) + probe['vecobs'].shape[1:], np.float32)
    if map_key:
        spec.update(_map_spec(probe, (T, B), map_key, map_categorical))
    if goals:
        _require_goal_sources(probe, f'the first episode file of {who}')
        for k, v in _goal_fields({k: probe[k][:1] for k in GOAL_SOURCES + ('goals_visage',) if k in probe}).items():
            spec[k] = ((T, B) + v.shape[1:], np.float32)
    return probe, spec


class ReplayFeed:
    """Planner + hot-path preprocessing writing IN PLACE into a slot of host arrays (DeviceRing hands it the numpy views of a
    pinned slot): the uint8 frame windows and the reset flags go from the episode arrays straight into the slot - one copy
    between the file and PCIe - and the small per-step fields (actions, reward, terminal) through a reused scratch batch.
    Field for field what `preprocess_batch(next(iter(replay)), ...)` returns (tests/test_replay_cpu.py compares the two).
    With map_key / map_categorical the slot also carries the map probe's inputs: `map` as the stored integer class map
    (T,B,H,W) - not preprocess_batch's one-hot; MapProbeHead takes either - and preprocess_batch's `map_seen_mask` and
    `map_coord` when the files hold their sources.  With goals=True it carries preprocess_batch's `goals_direction`,
    `goal_direction` and (when the files hold it) `goals_visage`; files without targets_vec / target_vec raise at construction.
    image_key=None (an image-less world model, the `vectorenv` section): the slot has no `image`, and files without `vecobs` - the
    only observation then - raise ValueError at construction.
    image_categorical = C (the number of classes, as in preprocess_batch; the `minigrid` section): the files hold an integer class
    image (n,H,W) and the slot carries it as stored, (T,B,H,W) in the stored dtype - the argmax over the class axis of
    preprocess_batch's one-hot, which WorldModel and the gru_probe baseline take with the same bits as the one-hot.  Integer
    (n,H,W) frames without it, or uint8 (n,H,W,C) frames with it, raise ValueError at construction.  fill() is the hot path and
    does NOT check that the classes lie in [0, C) (DeviceReplay does, once per file): a class outside is safe on the device -
    dm_dense_image_rows writes a zero column for it and dm_cat_image_loss reads nothing out of bounds - but is not a one-hot."""

    def __init__(self, replay, action_dim, clip_rewards=None, image_key='image', map_key=None, map_categorical=None, goals=False,
                 image_categorical=None):
        if clip_rewards not in (None, '', False, 'tanh', 'log1p'):
            raise ValueError(clip_rewards)
        self.replay, self.action_dim, self.clip_rewards, self.image_key = replay, int(action_dim), clip_rewards, image_key
        self.map_key = map_key
        probe, self._spec = _feed_layout(replay, self.action_dim, image_key, map_key, map_categorical, 'ReplayFeed', goals,
                                         image_categorical)
        T, B = replay.batch_length, replay.batch_size
        # `terminal` always has a column: an episode without the field contributes zeros (SequentialReplay._copy), so a
        # repository that mixes files with and without it still yields the flags of those that carry them
        self._small = {k: np.empty((T, B) + probe[k].shape[1:], probe[k].dtype)
                       for k in ('action', 'action_next', 'reward', 'vecobs') if k in probe}
        self._small['terminal'] = np.empty((T, B), probe['terminal'].dtype if 'terminal' in probe else np.float32)
        if map_key:
            for k in ('map_seen', 'map_vis', 'agent_pos', 'agent_dir'):      # sources of the mask and the coord: scratch
                if k in probe and k != map_key:
                    self._small[k] = np.empty((T, B) + probe[k].shape[1:], probe[k].dtype)
        self._goal_sources = [k for k in GOAL_SOURCES + ('goals_visage',) if k in probe] if goals else []
        for k in self._goal_sources:                                         # sources of the goal fields: scratch
            self._small[k] = np.empty((T, B) + probe[k].shape[1:], probe[k].dtype)

    def spec(self):
        """{field: (shape, dtype)} of a slot."""
        return dict(self._spec)

    def _actions(self, src, dst):
        if src.ndim == 2:                                     # integer actions -> one-hot rows
            dst[...] = 0.0
            np.put_along_axis(dst, src[..., None].astype(np.int64), 1.0, axis=2)
        else:
            dst[...] = src

    def fill(self, slot):
        raw = dict(self._small)
        if self.image_key:
            raw[self.image_key] = slot['image']
        raw['reset'] = slot['reset']
        if self.map_key:
            raw[self.map_key] = slot['map']
        self.replay.fill(raw)
        self._actions(raw['action'], slot['action'])
        self._actions(raw['action_next'], slot['action_next'])
        slot['terminal'][...] = raw['terminal']
        r = raw['reward'].astype(np.float32)
        if self.clip_rewards == 'tanh':
            r = np.tanh(r)
        elif self.clip_rewards == 'log1p':
            r = np.log1p(r)
        slot['reward'][...] = r
        if 'vecobs' in raw:
            slot['vecobs'][...] = raw['vecobs']
        if 'map_seen_mask' in slot:
            slot['map_seen_mask'][...] = _map_seen_mask(raw)
        if 'map_coord' in slot:
            slot['map_coord'][...] = _map_coord(raw, slot['map'].shape[-2])
        if self._goal_sources:
            for k, v in _goal_fields(raw).items():
                slot[k][...] = v
        return slot


class DeviceRing:
    """Pinned staging + asynchronous H2D into a ring of device-resident batches, WITHOUT a stream of its own.

    A producer thread pulls numpy batches from `source` (an iterator of preprocess_batch outputs) into one of `depth` pinned
    host slots - host work only.  The H2D copies are enqueued by the CONSUMER, on whatever stream is current, in one of two
    places: `prefetch()` stages the next batch (call it right after `training_step()` returned: the caller's stream has
    nothing left to do then while the backward passes run on their own streams, so the ~31 MB transfer is hidden), and
    `next()` returns the staged batch, staging it first if nobody prefetched (the copy then sits in front of the step).
    Ordering needs no events on the device side: a device slot is overwritten by a copy on the caller's stream `depth`
    batches after it was handed out, and everything that read it (the step's kernels, the side-stream backward passes that
    `loss.backward()` joins) is ordered before that on the same stream.  A pinned slot is rewritten by the producer only
    after a host-side wait for the event recorded behind its copy.

    Why no copy stream (rounds 1-2 had one): ROCm multiplexes HIP streams onto four hardware queues by default, and the
    step already uses the caller's stream, two backward streams and the library's weight-gradient side stream.  A copy
    stream is the fifth; when it lands on the queue of a stream that is parked behind an event for most of a step (the
    actor-critic backward stream is), the transfer for step n+2 completes a step late - measured as a bimodal H2D-included
    step, 37.3 or 44-47 ms depending on the process."""

    def __init__(self, source, device, depth=4):
        # source: an iterator of {key: numpy array} batches (copied into the pinned slot), or a feed with spec() / fill(slot)
        # (ReplayFeed) that writes the batch INTO the pinned slot
        self.feed = source if hasattr(source, 'fill') and hasattr(source, 'spec') else None
        self.source = None if self.feed is not None else iter(source)
        self.device, self.depth = torch.device(device), max(3, depth)
        self.free = queue.Queue()               # pinned slots the producer may fill
        self.filled = queue.Queue()             # pinned slots holding a batch, in source order (None: exhausted / failed)
        self.host = None                        # per pinned slot: {key: pinned tensor}
        self.copied = [None] * self.depth       # per pinned slot: event behind its last H2D copy
        self.dev = None                         # per device slot: {key: device tensor}
        self.next_dev = 0
        self.staged = None
        self.error = None
        self.done = False
        for i in range(self.depth):
            self.free.put(i)
        self.thread = threading.Thread(target=self._produce, daemon=True, name='dm-replay')
        self.thread.start()

    def _produce_feed(self):
        spec = self.feed.spec()
        self.host = [None] * self.depth
        while True:
            i = self.free.get()
            if i is None:
                return
            if self.host[i] is None:
                with torch.cuda.device(self.device):        # (a new thread's current device is 0)
                    self.host[i] = {k: torch.empty(shape, dtype=torch.from_numpy(np.empty(0, dt)).dtype).pin_memory()
                                    for k, (shape, dt) in spec.items()}
            elif self.copied[i] is not None:                 # the pinned buffer is the source of an asynchronous copy until this fires
                self.copied[i].synchronize()
            self.feed.fill({k: t.numpy() for k, t in self.host[i].items()})
            self.filled.put(i)

    def _produce(self):
        try:
            if self.feed is not None:
                return self._produce_feed()
            for batch in self.source:
                i = self.free.get()
                if i is None:
                    return
                if self.host is None:
                    self.host = [None] * self.depth
                if self.host[i] is None:
                    # a new thread's current device is 0: pin under THIS ring's device, or every rank creates a context on GPU 0
                    with torch.cuda.device(self.device):
                        self.host[i] = {k: torch.from_numpy(np.ascontiguousarray(v)).clone().pin_memory() for k, v in batch.items()}
                else:
                    ev = self.copied[i]
                    if ev is not None:          # the pinned buffer is still the source of an asynchronous copy until this fires
                        ev.synchronize()
                    for k, v in batch.items():
                        self.host[i][k].copy_(torch.from_numpy(np.ascontiguousarray(v)))
                self.filled.put(i)
            self.filled.put(None)               # source exhausted: next() raises StopIteration after the last batch
        except Exception as e:                  # surfaced by next()
            self.error = e
            self.filled.put(None)

    def __iter__(self):
        return self

    __next__ = lambda self: self.next()

    def prefetch(self):
        """Stage the next batch: enqueue its H2D copies on the current stream (no-op if one is staged already)."""
        if self.staged is not None or self.done:
            return
        i = self.filled.get()
        if i is None:
            self.done = True
            return
        host = self.host[i]
        with torch.cuda.device(self.device):
            if self.dev is None:
                self.dev = [{k: torch.empty_like(h, device=self.device) for k, h in host.items()} for _ in range(self.depth)]
            d = self.dev[self.next_dev]
            self.next_dev = (self.next_dev + 1) % self.depth
            for k in host:
                d[k].copy_(host[k], non_blocking=True)
            ev = self.copied[i] or torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self.copied[i] = ev
        self.free.put(i)                        # the producer waits for `ev` before touching the pinned buffers again
        self.staged = d

    def next(self):
        self.prefetch()
        if self.staged is None:
            if self.error is not None:
                raise RuntimeError('replay producer failed') from self.error
            raise StopIteration
        d, self.staged = self.staged, None
        return d

    def close(self):
        self.free.put(None)


# ---------------------------------------------------------------------------------------------------------------------------
# Device-resident replay: the episodes live in HBM, a batch is one gather launch (csrc/replay_gather.hip)

_RESIDENT_ALIGN = 256        # every field of an episode starts on a multiple of this inside the episode's flat buffer


class _Resident:
    """A cached episode file: prepared ONCE on the host with the element-wise rules of ReplayFeed.fill / preprocess_batch into
    one flat byte buffer (field k: `rows` rows of row_bytes[k] at offsets[k]), uploaded once.  After the upload the host keeps
    only what later plans need: `reset` (the reset scatter reads it) and the row count."""
    __slots__ = ('path', 'rows', 'reset', 'nbytes', 'offsets', 'host', 'dev')

    def __init__(self, path, rows, reset, nbytes, offsets, host):
        self.path, self.rows, self.reset, self.nbytes, self.offsets, self.host, self.dev = path, rows, reset, nbytes, offsets, host, None


class _ResidentEpisode:
    """One VISIT of a cached episode - what the planner holds where SequentialReplay holds an _Episode: its own `marks` (the
    reset scatter is drawn per visit) over the shared entry."""
    __slots__ = ('entry', 'fields', 'rows', 'marks')

    def __init__(self, entry):
        self.entry, self.fields, self.rows, self.marks = entry, {'reset': entry.reset}, entry.rows, None


class ReplayPlan:
    """One planned batch, host side.  pieces (B, 2, 3) int32: per column at most two pieces (start row, length, mark), lengths
    adding up to T, mark = the piece's first row gets an artificial reset; offsets (B, 2, F) int64: byte offset of each field
    inside the flat buffer of the piece's episode (an unused second piece repeats the first); episodes[b][p]: that episode's
    cache entry (None for an unused second piece)."""
    __slots__ = ('pieces', 'offsets', 'episodes')

    def __init__(self, pieces, offsets, episodes):
        self.pieces, self.offsets, self.episodes = pieces, offsets, episodes

    def entries(self):
        seen = {}
        for row in self.episodes:
            for e in row:
                if e is not None:
                    seen[id(e)] = e
        return list(seen.values())


class DeviceReplay:
    """The second feed: episodes RESIDENT on the device, every (T, B, ...) batch assembled by ONE gather launch
    (dm_replay_gather) - a step's frames cross PCIe once per episode file instead of once per visit.  Hands training_step()
    bit for bit what DeviceRing(ReplayFeed(replay, ...)) hands it for the same files, arguments and seed: the windows come from
    the same planner (`replay`, a SequentialReplay nothing has been drawn from yet - its draws are untouched: file choice,
    random start, reset scatter, tails, buffer_size / reload_interval), only what a chosen file turns into is replaced
    (SequentialReplay.load_episode): a visit is a fresh _ResidentEpisode over a cache entry instead of a freshly read _Episode.

    Episode cache, keyed by file path.  On first use a file is read and prepared once on the host with exactly the element-wise
    rules of ReplayFeed.fill: float32 one-hot action / action_next, float32 reward with reward[0] = 0 and clip_rewards applied
    by numpy (tanh / log1p are the host's bits), float32 terminal (zeros when the file lacks it), bool reset with reset[0] =
    True, float32 vecobs, uint8 frames (n, H, W, C) (`image_t` files transposed), and with map_key / map_categorical the stored
    integer class map plus preprocess_batch's map_seen_mask and map_coord, and with goals=True preprocess_batch's float32
    goals_direction, goal_direction and goals_visage - three more resident fields the same gather copies.  A file whose rows do not have the layout of the
    first file is passed over like an unreadable one.  Eviction is least-recently-VISITED first once the cached bytes pass
    `capacity_bytes` (0: no limit), and only drops the cache's reference: an episode a column cursor, a carried tail or a
    planned batch still holds stays alive until they let go, so device residency can exceed the budget by up to those - at
    most 2 B episodes per batch in flight plus the B cursors'.  A file evicted and chosen again is read and uploaded again.

    Threads and streams, as in DeviceRing: one background thread does host work only (np.load, preparation into pinned
    memory, planning `depth` batches ahead); ALL device work is enqueued by the consumer on the caller's current stream, from
    prefetch() (call it right after training_step() returned) or next(): the uploads of episodes the batch is the first to
    use (non_blocking, from pinned memory), the copy of the two small tables, and the gather into one of `depth` >= 3 device
    batch slots.  No stream of its own (DeviceRing's docstring records what a fifth stream cost).  A pinned source - an
    episode's staging buffer, a table - is released or rewritten only after an event recorded behind its copy has fired.
    Errors of the producer surface from next().

    Without `device` nothing touches the GPU: plan() alone is usable, the prepared episodes stay in ordinary host memory.
    image_key=None: no frames are cached, uploaded or gathered (one field fewer; the files must hold `vecobs`, as for ReplayFeed).
    image_categorical = C: the files hold an integer class image (n,H,W), resident and gathered as stored - (T,B,H,W) in the stored
    dtype, ReplayFeed's field; a 7 x 7 uint8 image is a 49-byte row, which the gather copies through its byte lanes.  Preparation
    checks once per file that every class lies in [0, C); a file that fails is passed over like a file of another layout."""

    def __init__(self, replay, action_dim, device=None, depth=3, capacity_bytes=0, clip_rewards=None, image_key='image',
                 map_key=None, map_categorical=None, goals=False, image_categorical=None):
        if clip_rewards not in (None, '', False, 'tanh', 'log1p'):
            raise ValueError(clip_rewards)
        if any(c.episode is not None or c.tail is not None for c in replay.columns):
            raise ValueError('DeviceReplay needs a SequentialReplay nothing has been drawn from yet')
        self.replay, self.action_dim, self.clip_rewards, self.image_key = replay, int(action_dim), clip_rewards, image_key
        self.map_key, self.map_categorical = map_key, map_categorical
        self.image_categorical = int(image_categorical) if image_categorical else None
        self.device = None if device is None else torch.device(device)
        self.depth, self.capacity_bytes = max(3, int(depth)), int(capacity_bytes or 0)
        self.goals = bool(goals)
        _, self._spec = _feed_layout(replay, self.action_dim, image_key, map_key, map_categorical, 'DeviceReplay', goals,
                                     self.image_categorical)
        self.names = list(self._spec)
        self._rows = {k: (tuple(shape[2:]), np.dtype(dt)) for k, (shape, dt) in self._spec.items()}
        self.row_bytes = {k: int(np.prod(shape, dtype=np.int64)) * dt.itemsize for k, (shape, dt) in self._rows.items()}
        self._cache, self.cached_bytes = {}, 0                 # path -> _Resident, least recently visited first
        replay.load_episode = self._visit
        # consumer / producer state (device given)
        self.free, self.planned = queue.Queue(), queue.Queue()
        self.thread = None
        self.dev = None                         # per device slot: {key: device tensor}
        self._fields = None                     # per device slot: the host descriptor array of dm_replay_gather
        self._tab_host = self._tab_dev = None   # per device slot: pinned / device tables (source pointers, then the pieces)
        self._tab_copied = [None] * self.depth  # per device slot: event behind its last table copy
        self._held = [None] * self.depth        # per device slot: the plan it was gathered from (keeps its episodes alive)
        self._uploading = []                    # (event, entries): pinned episode buffers still the source of a copy
        self.next_dev, self.staged, self.error, self.done = 0, None, None, False

    def spec(self):
        """{field: (shape, dtype)} of a batch: ReplayFeed.spec() of the same arguments."""
        return dict(self._spec)

    # ---- the cache (producer side; host only)
    def _onehot(self, src):
        if src.ndim == 1:                                     # integer actions -> one-hot rows (ReplayFeed._actions)
            out = np.zeros((src.shape[0], self.action_dim), np.float32)
            np.put_along_axis(out, src[:, None].astype(np.int64), 1.0, axis=1)
            return out
        return src.astype(np.float32)

    def _prepare(self, info):
        f = _Episode(info.load_data()).fields
        n = f['reward'].shape[0]
        if self.image_key and self.image_categorical:
            img = f[self.image_key]
            if not np.issubdtype(img.dtype, np.integer) or (img.size and (img.min() < 0 or img.max() >= self.image_categorical)):
                raise ValueError(f'{self.image_key!r} holds classes outside [0, {self.image_categorical}) (or is not an integer array)')
        r = f['reward'].astype(np.float32)
        if self.clip_rewards == 'tanh':
            r = np.tanh(r)
        elif self.clip_rewards == 'log1p':
            r = np.log1p(r)
        vals = {'image': f[self.image_key] if self.image_key else None, 'action': self._onehot(f['action']), 'action_next': self._onehot(f['action_next']),
                'terminal': f['terminal'].astype(np.float32) if 'terminal' in f else np.zeros(n, np.float32),
                'reward': r, 'reset': f['reset'].astype(bool)}
        if 'vecobs' in self._rows:
            vals['vecobs'] = f['vecobs'].astype(np.float32)
        if self.map_key:
            vals['map'] = f[self.map_key]
            if 'map_seen_mask' in self._rows:
                vals['map_seen_mask'] = _map_seen_mask(f)
            if 'map_coord' in self._rows:
                vals['map_coord'] = _map_coord(f, f[self.map_key].shape[-2])
        if self.goals:
            _require_goal_sources(f, f'the episode file {info.path}')
            vals.update(_goal_fields(f))
        offsets, nbytes = {}, 0
        for k in self.names:                                  # the gather trusts row_bytes: every file must have the first one's layout
            shape, dt = self._rows[k]
            if vals.get(k) is None or vals[k].shape != (n,) + shape or vals[k].dtype != dt:
                got = None if vals.get(k) is None else (vals[k].dtype, vals[k].shape)
                raise ValueError(f'field {k!r} is {got}, the batches are laid out for {dt} {(n,) + shape}')
            offsets[k] = nbytes
            nbytes += -(-n * self.row_bytes[k] // _RESIDENT_ALIGN) * _RESIDENT_ALIGN
        if self.device is not None:
            with torch.cuda.device(self.device):              # (a new thread's current device is 0)
                host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            flat = host.numpy()
        else:
            host = flat = np.empty(nbytes, np.uint8)
        entry = _Resident(info.path, n, vals['reset'].copy(), nbytes, offsets, host)
        for k in self.names:                                  # the frames: one copy from the file's array (also for image_t)
            flat[offsets[k]:offsets[k] + n * self.row_bytes[k]].view(self._rows[k][1]).reshape((n,) + self._rows[k][0])[...] = vals[k]
        return entry

    def _visit(self, info):
        """SequentialReplay.load_episode: the cached entry of the file (read and prepared now if it is not cached) as a fresh visit."""
        entry = self._cache.pop(info.path, None)
        if entry is None:
            entry = self._prepare(info)
            self.cached_bytes += entry.nbytes
        self._cache[info.path] = entry                         # most recently visited last
        while self.capacity_bytes and self.cached_bytes > self.capacity_bytes and len(self._cache) > 1:
            old = self._cache.pop(next(iter(self._cache)))     # only the cache's reference: cursors, tails and plans keep theirs
            self.cached_bytes -= old.nbytes
        return _ResidentEpisode(entry)

    def plan(self):
        """Plan the next batch on the host: the planner's windows as the tables the gather reads (ReplayPlan).  Needs no GPU."""
        T, B, F = self.replay.batch_length, self.replay.batch_size, len(self.names)
        pieces, offsets, episodes = np.zeros((B, 2, 3), np.int32), np.zeros((B, 2, F), np.int64), []
        for b, ps in enumerate(self.replay.plan_batch()):
            assert 1 <= len(ps) <= 2
            row = [None, None]
            for p, (ep, a, z) in enumerate(ps):
                mark = ep.marks is not None and bool(ep.marks[a:z].any())      # SequentialReplay._copy
                if mark and ep.fields['reset'][a:z].any():
                    raise ValueError('an artificial reset fell into a window that holds a real one')
                assert 0 <= a < z <= ep.entry.rows, (a, z, ep.entry.rows)
                pieces[b, p] = (a, z - a, mark)
                offsets[b, p] = [ep.entry.offsets[k] for k in self.names]
                row[p] = ep.entry
            if len(ps) == 1:
                offsets[b, 1] = offsets[b, 0]
            assert int(pieces[b, :, 1].sum()) == T
            episodes.append(row)
        return ReplayPlan(pieces, offsets, episodes)

    # ---- producer thread: host work only
    def _produce(self):
        try:
            while self.free.get() is not None:
                self.planned.put(self.plan())
        except Exception as e:                  # surfaced by next()
            self.error = e
            self.planned.put(None)

    # ---- consumer: all device work, on the caller's current stream
    def _start(self):
        if self.device is None:
            raise ValueError('DeviceReplay was built without a device: only plan() is available')
        for _ in range(self.depth):
            self.free.put(True)
        self.thread = threading.Thread(target=self._produce, daemon=True, name='dm-device-replay')
        self.thread.start()

    def _alloc(self):
        from . import hip as H
        B, F = self.replay.batch_size, len(self.names)
        tdt = lambda dt: torch.from_numpy(np.empty(0, dt)).dtype
        self.dev = [{k: torch.empty(shape, dtype=tdt(dt), device=self.device) for k, (shape, dt) in self._spec.items()}
                    for _ in range(self.depth)]
        self._fields = []
        for d in self.dev:
            arr = (H.dm_replay_field * F)()
            for i, k in enumerate(self.names):
                assert d[k].data_ptr() % 16 == 0
                arr[i].dst, arr[i].row_bytes, arr[i].is_reset = d[k].data_ptr(), self.row_bytes[k], int(k == 'reset')
            self._fields.append(arr)
        words = B * 2 * F + B * 3                # int64 source pointers, then the int32 pieces
        self._tab_host = [torch.empty(words, dtype=torch.int64, pin_memory=True) for _ in range(self.depth)]
        self._tab_dev = [torch.empty(words, dtype=torch.int64, device=self.device) for _ in range(self.depth)]

    def _stage(self, plan):
        B, F = self.replay.batch_size, len(self.names)
        stream = torch.cuda.current_stream(self.device)
        if self.dev is None:
            self._alloc()
        # pinned episode buffers whose copy has completed are let go
        still = []
        for ev, entries in self._uploading:
            if ev.query():
                for e in entries:
                    e.host = None
            else:
                still.append((ev, entries))
        self._uploading = still
        fresh = [e for e in plan.entries() if e.dev is None]
        for e in fresh:
            e.dev = torch.empty(e.nbytes, dtype=torch.uint8, device=self.device)
            assert e.dev.data_ptr() % 16 == 0 and all(o % 16 == 0 for o in e.offsets.values())
            e.dev.copy_(e.host, non_blocking=True)
        if fresh:
            ev = torch.cuda.Event()
            ev.record(stream)
            self._uploading.append((ev, fresh))
        i = self.next_dev
        self.next_dev = (i + 1) % self.depth
        if self._tab_copied[i] is not None:                   # the pinned table is the source of a copy until this fires
            self._tab_copied[i].synchronize()
        tab = self._tab_host[i].numpy()
        base = np.array([[e.dev.data_ptr() for e in (row[0], row[1] or row[0])] for row in plan.episodes], np.int64)
        tab[:B * 2 * F] = (base[:, :, None] + plan.offsets).ravel()
        tab[B * 2 * F:].view(np.int32)[:] = plan.pieces.ravel()
        self._tab_dev[i].copy_(self._tab_host[i], non_blocking=True)
        ev = self._tab_copied[i] or torch.cuda.Event()
        ev.record(stream)
        self._tab_copied[i] = ev
        self._held[i] = plan
        self._launch(i, stream)
        return self.dev[i]

    def _launch(self, i, stream):
        """The gather of device slot i from the tables last copied for it (scripts/replay_feed_bench.py times this alone)."""
        from . import hip as H
        T, B, F = self.replay.batch_length, self.replay.batch_size, len(self.names)
        src = self._tab_dev[i].data_ptr()
        H.call('dm_replay_gather', T, B, F, self._fields[i], ctypes.c_void_p(src + 8 * B * 2 * F), ctypes.c_void_p(src),
               ctypes.c_void_p(stream.cuda_stream))

    def __iter__(self):
        return self

    __next__ = lambda self: self.next()

    def prefetch(self):
        """Stage the next batch: enqueue the uploads it needs, its tables and its gather on the current stream (no-op if one is
        staged already)."""
        if self.staged is not None or self.done:
            return
        if self.thread is None:
            self._start()
        plan = self.planned.get()
        if plan is None:
            self.done = True
            return
        with torch.cuda.device(self.device):
            self.staged = self._stage(plan)
        self.free.put(True)

    def next(self):
        self.prefetch()
        if self.staged is None:
            if self.error is not None:
                raise RuntimeError('replay producer failed') from self.error
            raise StopIteration
        d, self.staged = self.staged, None
        return d

    def close(self):
        self.free.put(None)
