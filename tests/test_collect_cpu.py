"""The collection loop without a GPU: EpisodeRecorder, collect and RandomPolicy over scripted numpy environments and a
scripted policy - file names, fields and dtypes, the NaN positions of the three policy columns, image_t, an integer class image,
episode numbering (continued, and in a fixed order when two environments finish on one step), flush(), the files read back through
SequentialReplay + preprocess_batch - and the host-side refusals of dm_policy_draw_mode and of Dreamer.act's new arguments."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import dreamer_oracle as O
from pydreamer_amd import replay as R
from pydreamer_amd.collect import EpisodeRecorder, collect, stack_obs
from pydreamer_amd.policy import METRIC_KEYS, RandomPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DM_E_SHAPE, DM_E_WORKSPACE, DM_E_NULL = -1, -2, -5
A = 4


class ScriptEnv:
    """The reference's wrapped-environment protocol (wrappers.py:43-72) on a script: episode e of environment `idx` lasts
    lengths[e % len(lengths)] steps; every field is a fixed function of (idx, episode, step).  Even episodes end by a time limit
    (terminal stays False), odd ones terminate.  `episodes`: every row emitted, per episode; `starts`: the environment's step
    count when each episode began."""

    def __init__(self, idx, lengths, image='u8'):
        self.idx, self.lengths, self.image = idx, lengths, image
        self.episodes, self.starts, self.steps, self.t = [], [], 0, 0

    def _obs(self, action, reward, terminal, reset):
        e, rs = len(self.episodes) - 1, np.random.RandomState(1000 * self.idx + 37 * len(self.episodes) + self.t)
        obs = dict(vecobs=rs.randn(5).astype(np.float32), action=action, reward=np.array(reward), terminal=np.array(terminal),
                   reset=np.array(reset), tag=np.array([self.idx, e, self.t], np.int16))
        if self.image == 'u8':
            obs['image'] = rs.randint(0, 256, (6, 5, 3)).astype(np.uint8)
        elif self.image == 'classes':
            obs['image'] = rs.randint(0, 7, (6, 5)).astype(np.int64)
        self.episodes[-1].append(obs)
        return dict(obs)

    def reset(self):
        self.episodes.append([])
        self.starts.append(self.steps)
        self.t = 0
        return self._obs(np.zeros(A), 0.0, False, True)

    def step(self, action):
        assert isinstance(action, np.ndarray) and action.shape == (A,)
        e = len(self.episodes) - 1
        self.t += 1
        self.steps += 1
        done = self.t >= self.lengths[e % len(self.lengths)]
        reward = float(self.idx + 1) + 0.25 * self.t
        return self._obs(action.astype(np.float64), reward, bool(done and e % 2 == 1), False), reward, done, {}


def _metric(j, call, b):
    return np.float32(0.5 * j + 0.01 * call + 0.001 * b)


class ScriptPolicy:
    """Call n gives environment b the one-hot action (n + b) % A and the per-environment metrics _metric(j, n, b)."""

    def __init__(self, B, metrics=True):
        self.B, self.metrics, self.calls, self.seen = B, metrics, 0, []

    def __call__(self, obs):
        n, B = self.calls, self.B
        self.calls += 1
        self.seen.append({k: v.copy() for k, v in obs.items()})
        act = np.eye(A, dtype=np.float32)[(n + np.arange(B)) % A]
        if not self.metrics:
            return act, {}
        return act, {k: np.array([_metric(j, n, b) for b in range(B)], np.float32) for j, k in enumerate(METRIC_KEYS)}


def _closed_in_order(envs):
    """(environment, episode number within it) of every finished episode, in the recorder's order: by the step it closed on, the
    lower environment index first."""
    out = []
    for env in envs:
        for e, rows in enumerate(env.episodes):
            L = env.lengths[e % len(env.lengths)]
            if len(rows) == L + 1:
                out.append((env.starts[e] + L, env.idx, e))
    return [(i, e) for _, i, e in sorted(out)]


def _episode_fields(env, e):
    rows = env.episodes[e]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def _load(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def test_files_fields_and_policy_columns(tmp_path):
    # environments 0 and 1 both finish on step 3; 2 finishes later
    envs = [ScriptEnv(0, [3, 2, 4]), ScriptEnv(1, [3, 5]), ScriptEnv(2, [4, 3])]
    repo = R.LocalEpisodeRepository(str(tmp_path))
    rec = EpisodeRecorder(repo, 3, steps_per_npz=1)          # every step that closes an episode writes a file
    policy = ScriptPolicy(3)
    out = collect(envs, policy, rec, 12)
    assert out['steps'] == 36 and policy.calls == 12 and all(env.steps == 12 for env in envs)
    order = _closed_in_order(envs)
    assert order[:2] == [(0, 0), (1, 0)] and len(order) == out['episodes'] == rec.episodes
    assert [os.path.basename(p) for p in out['files']] == sorted(os.listdir(tmp_path)) and out['files'] == rec.files
    number = 0
    for path in out['files']:
        data = _load(path)
        n_eps = int(data['reset'].sum())
        want = [(_episode_fields(envs[i], e), envs[i], e) for i, e in order[number:number + n_eps]]
        cat = {k: np.concatenate([w[0][k] for w in want]) for k in want[0][0]}
        steps = len(cat['reset']) - n_eps
        assert os.path.basename(path) == repo.build_episode_name(number, number + n_eps - 1, float(cat['reward'].sum()), steps)
        assert R.parse_episode_name(path) == (number, number + n_eps - 1, steps)
        assert sorted(data) == sorted([k for k in cat if k != 'image'] + ['image_t'] + list(METRIC_KEYS))
        for k, w in cat.items():
            g = data['image_t'].transpose(3, 0, 1, 2) if k == 'image' else data[k]
            assert g.dtype == w.dtype and np.array_equal(g, w), (path, k)
        assert data['image_t'].shape == (6, 5, 3, len(cat['reset'])) and data['image_t'].dtype == np.uint8
        assert data['action'].dtype == np.float64 and data['reset'].dtype == bool and data['tag'].dtype == np.int16
        # the policy columns: value / entropy of the call on row t, a NaN on the last row; prob of the action row t carries
        pos = 0
        for fields, env, e in want:
            L, c0 = len(fields['reset']) - 1, env.starts[e]
            for j, k in enumerate(METRIC_KEYS):
                col = data[k][pos:pos + L + 1]
                calls = np.array([_metric(j, c0 + t, env.idx) for t in range(L)], np.float64)
                assert col.dtype == np.float64
                if k == 'action_prob':
                    assert np.isnan(col[0]) and np.array_equal(col[1:], calls), (k, col, calls)
                else:
                    assert np.isnan(col[-1]) and np.array_equal(col[:-1], calls), (k, col, calls)
            # the action on row t + 1 is the one the policy chose on row t
            assert np.array_equal(fields['action'][1:].argmax(-1), (c0 + np.arange(L) + env.idx) % A)
            pos += L + 1
        number += n_eps
    assert number == rec.episodes
    # two environments closed on the same step: one file, the lower index first
    first = _load(out['files'][0])
    assert first['tag'][0].tolist() == [0, 0, 0] and first['tag'][4].tolist() == [1, 0, 0] and int(first['reset'].sum()) == 2


def test_without_metrics_the_policy_columns_are_nan_and_a_class_image_is_stored_untouched(tmp_path):
    envs = [ScriptEnv(0, [2, 3], image='classes'), ScriptEnv(1, [4], image='classes')]
    repo = R.LocalEpisodeRepository(str(tmp_path))
    rec = EpisodeRecorder(repo, 2, steps_per_npz=10 ** 6)
    out = collect(envs, ScriptPolicy(2, metrics=False), rec, 9)
    assert len(out['files']) == 1 and rec.queue == [] and rec.steps_saved == sum(R.parse_episode_name(p)[2] for p in out['files'])
    data = _load(out['files'][0])
    assert 'image_t' not in data and data['image'].dtype == np.int64 and data['image'].shape == (len(data['reset']), 6, 5)
    order = _closed_in_order(envs)
    assert np.array_equal(data['image'], np.concatenate([_episode_fields(envs[i], e)['image'] for i, e in order]))
    for k in METRIC_KEYS:
        assert data[k].shape == data['reward'].shape and data[k].dtype == np.float64 and np.isnan(data[k]).all()


def test_numbering_continues_and_flush_writes_the_queue(tmp_path):
    repo = R.LocalEpisodeRepository(str(tmp_path))
    old = dict(action=np.zeros((5, A)), reward=np.ones(5), terminal=np.zeros(5, bool), reset=np.arange(5) == 0)
    repo.save_data(old, 3, 6)                                # a repository that already holds episodes up to number 6
    assert repo.count_steps() == (1, 4, 7)
    rec = EpisodeRecorder(repo, 2, steps_per_npz=1000)
    assert rec.episodes == 7
    envs = [ScriptEnv(0, [2], image=None), ScriptEnv(1, [3], image=None)]
    cur = [env.reset() for env in envs]
    rec.add(stack_obs(cur), [False, False])
    policy = ScriptPolicy(2)
    for step in range(1, 4):
        act, mets = policy(stack_obs(cur))
        done = []
        for b, env in enumerate(envs):
            if step == 3 and b == 0:
                done.append(False)
                continue
            cur[b], _, d, _ = env.step(act[b])
            done.append(d)
        if step == 3:                                        # environment 0 sits this step out: rows of environment 1 only
            rec.add(stack_obs(cur[1:]), done[1:], {k: v[1:] for k, v in mets.items()}, envs=[1])
        else:
            rec.add(stack_obs(cur), done, mets)
    assert len(rec.queue) == 2 and rec.queued_steps == 5 and rec.episodes == 9 and len(os.listdir(tmp_path)) == 1
    path = rec.flush()
    assert os.path.basename(path) == repo.build_episode_name(7, 8, float(sum(r['reward'] for e in envs for r in e.episodes[0])), 5)
    assert rec.flush() is None and rec.queue == [] and repo.count_steps() == (2, 9, 9)
    data = _load(path)
    assert data['tag'][:, 0].tolist() == [0, 0, 0, 1, 1, 1, 1]
    with pytest.raises(ValueError, match='without an open episode'):
        rec.add(stack_obs(cur), [False, False])              # both episodes are closed: a step row has nothing to join
    with pytest.raises(ValueError, match='done has shape'):
        rec.add(stack_obs(cur), [False])
    with pytest.raises(KeyError, match='terminal'):
        rec.add({k: v for k, v in stack_obs(cur).items() if k != 'terminal'}, [False, False])


def test_collect_stops_at_num_steps_and_resets_done_environments(tmp_path):
    envs = [ScriptEnv(0, [3]), ScriptEnv(1, [5])]
    rec = EpisodeRecorder(R.LocalEpisodeRepository(str(tmp_path)), 2)
    policy = ScriptPolicy(2)
    out = collect(envs, policy, rec, 7)
    assert policy.calls == 7 and [env.steps for env in envs] == [7, 7] and out['steps'] == 14
    assert out['episodes'] == 3 and len(out['files']) == 1 and rec.queue == []      # flushed below steps_per_npz
    for n, seen in enumerate(policy.seen):                   # the row after a done one is a fresh reset row of that environment alone
        assert seen['reset'].tolist() == [n % 3 == 0, n % 5 == 0], n
        assert seen['tag'][:, 2].tolist() == [n % 3, n % 5]
        assert seen['action'].shape == (2, A) and seen['image'].shape == (2, 6, 5, 3)
    data = _load(out['files'][0])                            # the open episodes (1 and 2 steps in) are not written
    assert len(data['reset']) == 4 + 6 + 4 and data['reset'].sum() == 3
    with pytest.raises(ValueError, match='environments'):
        collect(envs[:1], policy, rec, 1)


@pytest.mark.parametrize('image', ['u8', 'classes', None])
def test_written_files_read_back_through_the_replay_reader(tmp_path, image):
    envs = [ScriptEnv(0, [3, 6], image=image), ScriptEnv(1, [4], image=image), ScriptEnv(2, [5, 2], image=image)]
    repo = R.LocalEpisodeRepository(str(tmp_path))
    collect(envs, ScriptPolicy(3), EpisodeRecorder(repo, 3, steps_per_npz=10 ** 6), 13)
    order = _closed_in_order(envs)
    want = {k: np.concatenate([_episode_fields(envs[i], e)[k] for i, e in order]) for k in envs[0].episodes[0][0]}
    T = len(want['reset'])
    assert repo.count_steps() == (1, T - len(order), len(order))
    batch = R.SequentialReplay(repo, batch_length=T, batch_size=1, skip_first=False).fill()      # one window: every whole episode
    kw = dict(image_key='image' if image else None, image_categorical=7 if image == 'classes' else None)
    got = R.preprocess_batch(batch, A, clip_rewards='tanh', **kw)
    assert np.array_equal(got['action'][:, 0], want['action'].astype(np.float32)) and got['action'].dtype == np.float32
    assert np.array_equal(got['reward'][:, 0], np.tanh(want['reward'].astype(np.float32)))
    assert np.array_equal(got['terminal'][:, 0], want['terminal'].astype(np.float32)) and want['terminal'].sum() >= 1
    assert np.array_equal(got['reset'][:, 0], want['reset']) and got['reset'].sum() == len(order)
    assert np.array_equal(got['vecobs'][:, 0], want['vecobs'])
    assert np.array_equal(batch['action_next'][:-1, 0], want['action'][1:])
    if image == 'u8':
        assert got['image'].dtype == np.uint8 and np.array_equal(got['image'][:, 0], want['image'])
    elif image == 'classes':
        assert np.array_equal(got['image'][:, 0].argmax(1), want['image']) and got['image'].shape == (T, 1, 7, 6, 5)
    else:
        assert 'image' not in got


def test_random_policy():
    for B in (1, 3):
        p, q, other = RandomPolicy(A, B, seed=5), RandomPolicy(A, B, seed=5), RandomPolicy(A, B, seed=6)
        acts = [p(None) for _ in range(20)]
        assert all(m == {} for _, m in acts)
        a = np.stack([x for x, _ in acts])
        assert a.shape == ((20, A) if B == 1 else (20, B, A)) and a.dtype == np.float32
        assert np.array_equal(a.sum(-1), np.ones(a.shape[:-1])) and np.array_equal(a.max(-1), np.ones(a.shape[:-1]))
        assert len(np.unique(a.reshape(-1, A).argmax(-1))) > 1
        assert np.array_equal(a, np.stack([q(None)[0] for _ in range(20)]))
        assert not np.array_equal(a, np.stack([other(None)[0] for _ in range(20)]))
        c = np.stack([RandomPolicy(A, B, seed=5, continuous=True)(None)[0] for _ in range(20)])
        assert c.shape == a.shape and c.dtype == np.float32 and c.min() >= -1.0 and c.max() <= 1.0 and c.min() < 0 < c.max()
        assert np.array_equal(c[0], RandomPolicy(A, B, seed=5, continuous=True)(None)[0])
    envs = [ScriptEnv(0, [3], image=None), ScriptEnv(1, [2], image=None)]
    assert RandomPolicy(A, 2, seed=1)(stack_obs([e.reset() for e in envs]))[0].shape == (2, A)


# ------------------------------------------------------------------------------------------------ NetworkPolicy(per_env=True) over a stub
class _StubModel:
    def __init__(self):
        self.kwargs = []

    def init_state(self, batch_size):
        return (torch.zeros(batch_size, 2),)

    def act(self, obs, in_state, noise=None, return_rows=False, mode='sample', action_noise=0.0):
        self.kwargs.append(dict(return_rows=return_rows, mode=mode, action_noise=action_noise))
        B = obs['action'].shape[1]
        action = torch.eye(A)[torch.arange(B) % A].view(1, B, A)
        stats = torch.tensor([1.0, 2.0, 3.0, 0.0])
        m = dict(policy_value=stats[0], action_prob=stats[1], policy_entropy=stats[2])
        if return_rows:
            m.update(log_prob=-torch.arange(1.0, B + 1), entropy=0.5 * torch.arange(1.0, B + 1), value=10.0 + torch.arange(B))
        return action, (in_state[0] + 1,), m


def test_network_policy_per_env_and_modes_over_a_stub():
    from pydreamer_amd import NetworkPolicy
    B = 3
    obs = dict(action=np.zeros((1, B, A), np.float32), reward=np.zeros((1, B), np.float32), reset=np.zeros((1, B), bool))
    model = _StubModel()
    policy = NetworkPolicy(model, lambda o: o, batch_size=B, device='cpu', mode='mode', per_env=True)
    action, mets = policy(obs)
    assert model.kwargs == [dict(return_rows=True, mode='mode', action_noise=0.0)]
    assert action.shape == (B, A) and set(mets) == set(METRIC_KEYS)
    assert all(v.shape == (B,) and v.dtype == np.float32 for v in mets.values())
    assert np.array_equal(mets['policy_value'], 10.0 + np.arange(B)) and np.array_equal(mets['policy_entropy'], 0.5 * np.arange(1, B + 1))
    assert np.array_equal(mets['action_prob'], torch.exp(-torch.arange(1.0, B + 1)).numpy())
    NetworkPolicy(model, lambda o: o, batch_size=B, device='cpu', action_noise=0.25)(obs)
    assert model.kwargs[-1] == dict(return_rows=False, mode='sample', action_noise=0.25)
    for kw in (dict(mode='greedy'), dict(action_noise=-0.1), dict(mode='mode', action_noise=0.1), dict(action_noise=float('nan'))):
        with pytest.raises(ValueError):
            NetworkPolicy(model, lambda o: o, batch_size=B, device='cpu', **kw)


# ------------------------------------------------------------------------------------------------ the library's and act's refusals
def test_draw_mode_symbol_and_host_side_argument_checks(hip):
    assert 'dm_policy_draw_mode' in hip.exported_symbols()
    hdr = open(os.path.join(ROOT, 'include', 'dreamer_hip.h')).read()
    assert 'dm_policy_draw_mode' in set(re.findall(r'\b(dm_[a-z0-9_]+)\s*\(', hdr))
    lib = hip.lib()
    assert lib.dm_version() == hip.DM_ABI_VERSION == 17
    rows = 5
    wsb = 4 * lib.dm_policy_draw_ws_floats(rows)
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every call below fails its host-side checks

    def draw(kind=0, mode=0, amount=0.0, A_=6, ldp=None, noise=fake, noise2=fake, params=fake, action=fake, stats=fake, ws=fake,
             wsb=wsb, lda=None):
        width = A_ if kind == 0 else 2 * A_
        return lib.dm_policy_draw_mode(kind, mode, amount, rows, A_, params, width if ldp is None else ldp, noise, noise2, fake, action,
                                       A_ if lda is None else lda, None, None, None, stats, ws, wsb, None)

    for kind in (0, 1, 2):
        for kw in (dict(mode=3), dict(mode=-1), dict(mode=2, amount=-0.5), dict(mode=0, amount=-1e-9), dict(mode=1, amount=float('nan')),
                   dict(mode=2, amount=float('nan')), dict(mode=1, ldp=0), dict(mode=2, amount=0.5, lda=5), dict(kind=3, mode=1)):
            assert draw(**{'kind': kind, **kw}) == DM_E_SHAPE, (kind, kw)
            assert lib.dm_last_error()
        for kw in (dict(mode=0, noise=None), dict(mode=2, noise=None), dict(mode=2, amount=0.5, noise=None),
                   dict(mode=2, amount=0.5, noise2=None), dict(mode=1, params=None), dict(mode=1, action=None), dict(mode=2, stats=None),
                   dict(mode=1, noise=None, noise2=None, ws=None)):
            assert draw(**{'kind': kind, **kw}) == DM_E_NULL, (kind, kw)
            assert b'null' in lib.dm_last_error()
        # what is NOT refused for its pointers gets as far as the workspace check: mode 1 without noise, mode 2 / amount 0 without noise2
        for kw in (dict(mode=1, noise=None, noise2=None), dict(mode=2, amount=0.0, noise2=None), dict(mode=0, noise2=None),
                   dict(mode=2, amount=0.5)):
            assert draw(**{'kind': kind, 'wsb': wsb - 4, **kw}) == DM_E_WORKSPACE, (kind, kw)
            assert b'workspace' in lib.dm_last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f'Dreamer.act reached the library ({name}) before refusing its arguments')


@pytest.mark.parametrize('actor_dist', ['onehot', 'tanh_normal'])
def test_act_refuses_its_new_arguments_before_any_device_use(monkeypatch, actor_dist):
    from pydreamer_amd import config, hip as H
    from pydreamer_amd.models import Dreamer
    oconf = O.tiny_conf()
    conf = config.load_config('defaults', 'atari', **{**vars(oconf), 'actor_dist': actor_dist})
    with torch.device('meta'):
        model = Dreamer(conf)
    monkeypatch.setattr(H, '_lib', _NoLibrary())
    monkeypatch.setattr(H, 'call', lambda *a, **k: (_ for _ in ()).throw(AssertionError('library call')))
    B, Ad = 3, conf.action_dim
    state = model.init_state(B)
    obs = dict(action=torch.zeros(1, B, Ad, device='meta'))
    with pytest.raises(ValueError, match="'sample' or 'mode'"):
        model.act(obs, state, mode='greedy')
    with pytest.raises(ValueError, match='action_noise'):
        model.act(obs, state, mode='mode', action_noise=0.3)
    for bad in (-0.1, float('nan')):
        with pytest.raises(ValueError, match='action_noise'):
            model.act(obs, state, action_noise=bad)
    good = (B, 2) if actor_dist == 'onehot' else (B, Ad)
    for shape in ((B,), (B + 1,) + good[1:], (1,) + good, (B, good[1] + 1)):
        with pytest.raises(ValueError, match='exploration noise'):
            model.act(obs, state, action_noise=0.3, noise=dict(u_expl=torch.zeros(shape)))
