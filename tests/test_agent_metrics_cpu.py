"""The feedback half of the loop without a GPU: collect.EpisodeStats against a restatement of generator.py:167-216
written here from the episode files read back through LocalEpisodeRepository, the recorder's on_episode hook and train / test split,
Collector.run_episodes and the environment wrappers of envs.py.  Scripted environments and policies only; no gym."""
import os
import time

import numpy as np
import pytest

from pydreamer_amd import config, replay as R
from pydreamer_amd.collect import Collector, EpisodeRecorder, EpisodeStats, collect
from pydreamer_amd.envs import wrap_env, wrap_envs
from pydreamer_amd.policy import METRIC_KEYS, RandomPolicy
from tests.test_collect_cpu import A, ScriptEnv, ScriptPolicy

GAMMA = 0.99
RTOL = 1e-6      # sums and means of <= 20 terms, both sides on the host
# env 0 and env 1 both close on step 1; env 1's episode 1 is ONE step long and terminates (odd episodes terminate, even ones end by
# a time limit); lengths 1, 2 and about 10
LENGTHS = [[1, 2, 10], [1, 1, 9, 2], [10, 3]]


def _envs(lengths=LENGTHS, cls=ScriptEnv):
    return [cls(i, l, image=None) for i, l in enumerate(lengths)]


def _episodes(repo):
    """Every episode of the repository's files, by episode number."""
    out = {}
    for info in repo.list_files():
        data = info.load_data()
        starts = np.flatnonzero(data['reset']).tolist() + [len(data['reset'])]
        assert len(starts) - 1 == info.episode_to - info.episode_from + 1, info.path
        for n, (a, z) in enumerate(zip(starts, starts[1:])):
            assert info.episode_from + n not in out
            out[info.episode_from + n] = {k: v[a:z] for k, v in data.items()}
    return out


def _restate(ep, gamma=GAMMA):
    """generator.py:167-202 for one episode, written from the formulas: plain Python sums, the discounted return as the explicit
    double sum."""
    r = [float(v) for v in ep['reward']]
    T = len(r)
    terminated = bool(ep['terminal'][-1])
    x = list(r)
    if not terminated:
        x[-1] += (sum(r) / T) / (1.0 - gamma)
    disc = [sum(gamma ** (k - t) * x[k] for k in range(t, T)) for t in range(T)]
    want = {'episode_length': T - 1, 'return': sum(r), 'return_discounted': sum(disc) / T}
    for k in METRIC_KEYS:
        vals = [float(v) for v in ep[k] if not np.isnan(v)]
        if vals:
            want[k] = sum(vals) / len(vals)
    if terminated and not np.isnan(ep['policy_value'][T - 2]):
        want['policy_value_terminal'] = float(ep['policy_value'][T - 2]) - r[-1]
    if 'goals_visage' in ep:
        g = np.asarray(ep['goals_visage'], np.float64)
        seen = g < 1e5
        want['goals_seen_avg'] = sum(int(row.sum()) for row in seen) / T
        want['goals_seen_last'] = int(seen[-1].sum())
        want['goals_seenage'] = float(g[seen].sum()) / int(seen.sum())
    return want


def _close(a, b):
    return abs(float(a) - float(b)) <= RTOL * abs(float(b))


def _closing_steps(envs):
    """{(environment, episode): the collector step on which it closed}, in closing order (the lower environment first)."""
    out = []
    for env in envs:
        for e, rows in enumerate(env.episodes):
            L = env.lengths[e % len(env.lengths)]
            if len(rows) == L + 1:
                out.append((env.starts[e] + L, env.idx, e))
    return sorted(out)


def _record(tmp_path, envs, policy, num_steps, prefix='agent', action_repeat=1):
    """Collects with steps_per_npz = 1 and an EpisodeStats popped after every episode: the per-episode values."""
    repo = R.LocalEpisodeRepository(str(tmp_path))
    stats, per_episode = EpisodeStats(prefix, gamma=GAMMA, log_every=1, action_repeat=action_repeat), []

    def hook(data):
        assert not stats.ready()
        stats.add_episode(data, col.steps, rec.steps_saved, rec.episodes + 1, col.seconds())
        assert stats.ready()
        per_episode.append(stats.pop())

    rec = EpisodeRecorder(repo, len(envs), steps_per_npz=1, on_episode=hook)
    col = Collector(envs, policy, rec)
    col.run(num_steps)
    col.close()
    return repo, rec, per_episode


def test_every_agent_value_equals_the_restatement_from_the_files(tmp_path):
    envs = _envs()
    B = len(envs)
    repo, rec, got = _record(tmp_path, envs, ScriptPolicy(B), 23, action_repeat=4)
    eps = _episodes(repo)
    closed = _closing_steps(envs)
    assert len(got) == len(eps) == len(closed) == rec.episodes >= 9
    assert closed[0][0] == closed[1][0] == 1                                   # two environments close on the same step
    lengths = sorted({len(e['reward']) - 1 for e in eps.values()})
    assert lengths[:2] == [1, 2] and lengths[-1] in (9, 10)
    returns, seen = [], {'boot': 0, 'term': 0, 'term1': 0}
    for n, (step, idx, e) in enumerate(closed):
        ep, m = eps[n], got[n]
        want = _restate(ep)
        terminated = bool(ep['terminal'][-1])
        assert terminated == (e % 2 == 1)
        returns.append(want['return'])
        want['return_cum'] = sum(returns[-100:]) / len(returns[-100:])
        want['return_max'] = want['return']
        keys = {f'agent/{k}' for k in want} | {'agent/steps', 'agent/env_steps', 'agent/steps_saved', 'agent/episodes'}
        assert set(m) - {'agent/fps'} == keys, (n, set(m) ^ keys)
        assert '_timestamp' not in m and m.get('agent/fps', 1.0) > 0
        for k, v in want.items():
            print(f'episode {n} (env {idx}, {len(ep["reward"]) - 1} steps, terminated {terminated}) {k}: {m["agent/" + k]:.9g} want {v:.9g}')
            assert _close(m[f'agent/{k}'], v), (n, k, m[f'agent/{k}'], v)
        # counts: exact
        assert m['agent/episode_length'] == len(ep['reward']) - 1 == envs[idx].lengths[e % len(envs[idx].lengths)]
        assert m['agent/steps'] == step * B and m['agent/env_steps'] == 4 * step * B
        assert m['agent/episodes'] == n + 1
        # steps_per_npz = 1: every step that closes an episode writes its file when the step's rows are in, so an episode sees the
        # steps of the episodes closed on EARLIER steps
        assert m['agent/steps_saved'] == sum(len(eps[j]['reward']) - 1 for j, c in enumerate(closed) if c[0] < step)
        assert ('agent/policy_value_terminal' in m) == terminated
        seen['term' if terminated else 'boot'] += 1
        if terminated and len(ep['reward']) == 2:
            seen['term1'] += 1
            assert _close(m['agent/policy_value_terminal'], float(ep['policy_value'][0]) - float(ep['reward'][1]))
    assert min(seen.values()) >= 1, seen
    # with and without the bootstrap term: the same rewards give different values
    ep = next(e for e in eps.values() if not e['terminal'][-1] and len(e['reward']) > 3)
    assert not _close(_restate(ep)['return_discounted'], _restate({**ep, 'terminal': np.ones_like(ep['terminal'])})['return_discounted'])


def test_return_discounted_with_and_without_the_bootstrap_term():
    reward = np.array([0.0, 1.0, -2.0, 0.5], np.float32)
    base = dict(reward=reward, policy_value=np.array([0.3, 0.2, 0.1, np.nan]), policy_entropy=np.full(4, np.nan),
                action_prob=np.full(4, np.nan))
    for terminated in (True, False):
        s = EpisodeStats('p', gamma=0.9, log_every=1)
        s.add_episode(dict(base, terminal=np.array([False, False, False, terminated])), 3, 0, 1, 0.5)
        m = s.pop()
        x = [0.0, 1.0, -2.0, 0.5 + (0.0 if terminated else (-0.5 / 4) / (1 - 0.9))]
        y3 = x[3]
        y2 = x[2] + 0.9 * y3
        y1 = x[1] + 0.9 * y2
        y0 = x[0] + 0.9 * y1
        assert _close(m['p/return_discounted'], (y0 + y1 + y2 + y3) / 4), (terminated, m)
        assert ('p/policy_value_terminal' in m) == terminated
        if terminated:
            assert _close(m['p/policy_value_terminal'], 0.1 - 0.5)
        assert m['p/fps'] == 3 / 0.5 and 'p/action_prob' not in m and _close(m['p/policy_value'], 0.2)


def test_random_policy_records_no_policy_keys(tmp_path):
    envs = _envs()
    repo, rec, got = _record(tmp_path, envs, RandomPolicy(A, len(envs), seed=3), 12)
    assert len(got) >= 6 and any(e['terminal'][-1] for e in _episodes(repo).values())
    for m in got:
        assert not {f'agent/{k}' for k in METRIC_KEYS + ('policy_value_terminal',)} & set(m), sorted(m)
        assert {'agent/return', 'agent/return_discounted', 'agent/episode_length'} <= set(m)


class GoalsEnv(ScriptEnv):
    """ScriptEnv with a (3,) goals_visage row: goal g was last seen (t + g) steps ago, or never (1e5) on some rows."""

    def _obs(self, action, reward, terminal, reset):
        obs = super()._obs(action, reward, terminal, reset)
        obs['goals_visage'] = np.array([1e5 if (self.t + g + self.idx) % 3 == 0 else float(self.t + g) for g in range(3)])
        return obs


def test_goals_metrics_on_an_episode_with_goals_visage(tmp_path):
    envs = _envs([[4, 3], [5]], cls=GoalsEnv)
    repo, rec, got = _record(tmp_path, envs, ScriptPolicy(2), 10)
    eps = _episodes(repo)
    assert len(got) == len(eps) >= 3
    for n, m in enumerate(got):
        want = _restate(eps[n])
        assert 0 < want['goals_seen_avg'] < 3
        for k in ('goals_seen_avg', 'goals_seen_last', 'goals_seenage'):
            assert _close(m[f'agent/{k}'], want[k]), (n, k, m[f'agent/{k}'], want[k])
    os.makedirs(tmp_path / 'plain')
    _, _, plain = _record(tmp_path / 'plain', _envs([[4]]), ScriptPolicy(1), 4)
    assert len(plain) == 1 and not any(k.startswith('agent/goals') for k in plain[0])


def _synthetic(i, terminated, with_policy=True, length=1):
    """A closed episode dict of `length` steps with return i."""
    n = length + 1
    col = np.full(n, np.nan)
    data = dict(reward=np.array([0.0] * length + [float(i)]), terminal=np.array([False] * length + [terminated]),
                reset=np.arange(n) == 0, policy_value=col.copy(), policy_entropy=col.copy(), action_prob=col.copy())
    if with_policy:
        data['policy_value'][:-1] = 0.25 * i
        data['policy_entropy'][:-1] = 0.5
        data['action_prob'][1:] = 0.125
    return data


def test_aggregation_log_every_4_over_9_episodes():
    stats = EpisodeStats('agent', gamma=GAMMA, log_every=4)
    pops, held = [], []
    for i in range(9):
        # odd episodes terminate (policy_value_terminal is NaN-free only there); episodes 2 and 6 carry no policy columns
        stats.add_episode(_synthetic(i, i % 2 == 1, with_policy=i not in (2, 6), length=1 + i % 3), 10 * (i + 1), 7 * i, i + 1, 0.5 * (i + 1))
        if stats.ready():
            pops.append(stats.pop())
            assert not stats.ready()
    assert len(pops) == 2 and len(stats.agg['agent/return']) == 1      # two pops, one pending episode
    for j, m in enumerate(pops):
        idx = list(range(4 * j, 4 * j + 4))
        assert _close(m['agent/return'], sum(idx) / 4) and m['agent/return_max'] == max(idx)
        assert _close(m['agent/episode_length'], sum(1 + i % 3 for i in idx) / 4)
        assert m['agent/steps'] == sum(10 * (i + 1) for i in idx) / 4 and m['agent/episodes'] == sum(i + 1 for i in idx) / 4
        assert m['agent/steps_saved'] == sum(7 * i for i in idx) / 4
        # keys that are NaN for some episodes are averaged over the others
        odd, pol = [i for i in idx if i % 2 == 1], [i for i in idx if i not in (2, 6)]
        assert len(pol) == 3 and len(odd) == 2
        assert _close(m['agent/policy_value'], sum(0.25 * i for i in pol) / 3)
        assert _close(m['agent/policy_entropy'], 0.5) and _close(m['agent/action_prob'], 0.125)
        assert _close(m['agent/policy_value_terminal'], sum(0.25 * i - i for i in odd) / 2)
        cums = [sum(range(i + 1)) / (i + 1) for i in idx]
        assert _close(m['agent/return_cum'], sum(cums) / 4)
        # 40 transitions in 2 seconds of collecting between two pops
        assert m['agent/fps'] == 20.0 and '_timestamp' not in m
    assert EpisodeStats('agent').pop() == {} and not EpisodeStats('agent', log_every=0).ready()


def test_return_cum_uses_the_last_100_returns_and_survives_pop():
    stats, last = EpisodeStats('agent', log_every=1), None
    for i in range(103):
        stats.add_episode(_synthetic(i, True), i + 1, i, i + 1, float(i + 1))
        last = stats.pop()
    assert len(stats.returns) == 100
    assert _close(last['agent/return_cum'], sum(range(3, 103)) / 100) and last['agent/return'] == 102.0


# ------------------------------------------------------------------------------------------------ the split
def test_split_follows_the_seeded_draws(tmp_path):
    da, db = str(tmp_path / 'train'), str(tmp_path / 'test')
    os.makedirs(da), os.makedirs(db)
    repo, repo2 = R.LocalEpisodeRepository(da), R.LocalEpisodeRepository(db)
    closed = []
    rec = EpisodeRecorder(repo, 3, steps_per_npz=1, on_episode=lambda d: closed.append(rec.steps_saved), repository2=repo2,
                          split_fraction=0.5, rng=np.random.RandomState(7))
    out = collect(_envs(), ScriptPolicy(3), rec, 30)
    assert len(rec.files) == len(out['files']) >= 8
    replay = np.random.RandomState(7)      # one draw per written queue, in writing order
    want = [da if replay.rand() > 0.5 else db for _ in rec.files]
    assert [os.path.dirname(p) for p in rec.files] == want and {da, db} == set(want)
    assert sorted(os.listdir(da)) == sorted(os.path.basename(p) for p, d in zip(rec.files, want) if d == da)
    assert sorted(os.listdir(db)) == sorted(os.path.basename(p) for p, d in zip(rec.files, want) if d == db)
    # one episode counter for both destinations
    spans = sorted(R.parse_episode_name(p)[:2] for p in rec.files)
    numbers = [n for a, z in spans for n in range(a, z + 1)]
    assert numbers == list(range(rec.episodes)) and rec.episodes == out['episodes']
    assert set(_episodes(repo)) | set(_episodes(repo2)) == set(numbers) and not set(_episodes(repo)) & set(_episodes(repo2))
    # steps_saved: the first repository's steps only - at the end, and whenever the hook looked
    assert rec.steps_saved == repo.count_steps()[1] < repo.count_steps()[1] + repo2.count_steps()[1]
    assert closed == sorted(closed) and closed[-1] <= rec.steps_saved
    with pytest.raises(ValueError, match='repository2'):
        EpisodeRecorder(repo, 3, split_fraction=0.5)
    # the default rng is RandomState(0)
    dc, dd = str(tmp_path / 'c'), str(tmp_path / 'd')
    os.makedirs(dc), os.makedirs(dd)
    rec0 = EpisodeRecorder(R.LocalEpisodeRepository(dc), 3, steps_per_npz=1, repository2=R.LocalEpisodeRepository(dd), split_fraction=0.5)
    collect(_envs(), ScriptPolicy(3), rec0, 30)
    replay = np.random.RandomState(0)
    assert [os.path.dirname(p) for p in rec0.files] == [dc if replay.rand() > 0.5 else dd for _ in rec0.files]


def test_split_fraction_zero_writes_the_same_bytes_and_draws_nothing(tmp_path, monkeypatch):
    # an npz is a zip file and stamps its members with the local time: hold the clock still, so that equal bytes mean equal content
    frozen = time.localtime(1_700_000_000)
    monkeypatch.setattr(time, 'localtime', lambda *a: frozen)
    da, db, dc = (str(tmp_path / n) for n in 'abc')
    os.makedirs(da), os.makedirs(db), os.makedirs(dc)
    collect(_envs(), ScriptPolicy(3), EpisodeRecorder(R.LocalEpisodeRepository(da), 3, steps_per_npz=5), 25)
    rng = np.random.RandomState(11)
    before = rng.get_state()[1].copy()
    rec = EpisodeRecorder(R.LocalEpisodeRepository(db), 3, steps_per_npz=5, on_episode=None, repository2=R.LocalEpisodeRepository(dc),
                          split_fraction=0.0, rng=rng)
    collect(_envs(), ScriptPolicy(3), rec, 25)
    assert np.array_equal(rng.get_state()[1], before) and os.listdir(dc) == []
    names = sorted(os.listdir(da))
    assert names == sorted(os.listdir(db)) and len(names) >= 3
    for n in names:
        assert open(os.path.join(da, n), 'rb').read() == open(os.path.join(db, n), 'rb').read(), n
    assert rec.steps_saved == R.LocalEpisodeRepository(db).count_steps()[1]


# ------------------------------------------------------------------------------------------------ run_episodes
def test_run_episodes_records_both_environments_that_close_together(tmp_path):
    envs = _envs([[3], [3], [7]])
    rec = EpisodeRecorder(R.LocalEpisodeRepository(str(tmp_path)), 3, steps_per_npz=10 ** 6)
    col = Collector(envs, ScriptPolicy(3), rec)
    out = col.run_episodes(2)
    assert out['episodes'] == 2 and out['steps'] == 9 == col.steps and out['files'] == [] and sorted(out) == ['episodes', 'files', 'steps']
    out = col.run_episodes(1)                                  # one asked for, two close on step 6
    assert out['episodes'] == 2 and out['steps'] == 9 and col.steps == 18 and rec.episodes == 4
    out = col.run_episodes(1)                                  # step 7: environment 2
    assert out['episodes'] == 1 and out['steps'] == 3
    assert col.run(2) == dict(steps=6, episodes=2, files=[]) and col.steps == 27      # run() goes on from there: step 9 closes two
    path = col.close()
    assert rec.files == [path] and rec.steps_saved == 3 * 6 + 7 and col.seconds() > 0
    eps = _episodes(R.LocalEpisodeRepository(str(tmp_path)))
    assert [int(e['tag'][0, 0]) for e in eps.values()] == [0, 1, 0, 1, 2, 0, 1]
    out = col.run_episodes(1)                                  # after close(): the environments are reset
    assert out['steps'] == 9 and out['episodes'] == 2 and rec.episodes == 9
    assert len(envs[2].episodes[-2]) == 3 and len(envs[2].episodes[-1]) == 4      # its open episode, two steps in, was dropped


# ------------------------------------------------------------------------------------------------ the wrappers
class RawEnv:
    """A raw environment: `kind` observation ('dict' / 'vector' / 'image'), a 4- or 5-tuple step result, reset() with or without
    info; done after `length` steps; records the actions it was given."""

    def __init__(self, kind, length, api=4, truncated_key=False):
        self.kind, self.length, self.api, self.truncated_key, self.t, self.actions = kind, length, api, truncated_key, 0, []

    def _obs(self):
        if self.kind == 'vector':
            return np.full(5, self.t, np.float32)
        if self.kind == 'image':
            return np.full((6, 5, 3), self.t, np.uint8)
        return dict(vecobs=np.full(5, self.t, np.float32), extra=np.array(self.t))

    def reset(self):
        self.t = 0
        return (self._obs(), {'note': 1}) if self.api == 5 else self._obs()

    def step(self, action):
        self.actions.append(action)
        self.t += 1
        done = self.t >= self.length
        if self.api == 5:      # even lengths terminate, odd ones are truncated
            return self._obs(), 0.5 * self.t, done and self.length % 2 == 0, done and self.length % 2 == 1, {}
        return self._obs(), 0.5 * self.t, done, ({'TimeLimit.truncated': True} if done and self.truncated_key else {})


def _onehot(i):
    return np.eye(A, dtype=np.float32)[i]


@pytest.mark.parametrize('kind,key', [('dict', 'vecobs'), ('vector', 'vecobs'), ('image', 'image')])
def test_wrapper_observations_and_fields(kind, key):
    raw = RawEnv(kind, 3)
    env = wrap_env(raw, A)
    obs = env.reset()
    assert set(obs) == {key, 'action', 'reward', 'terminal', 'reset'} | ({'extra'} if kind == 'dict' else set())
    assert obs['action'].shape == (A,) and not obs['action'].any() and obs['reward'] == 0.0 and obs['reward'].shape == ()
    assert obs['terminal'].dtype == bool and not obs['terminal'] and obs['reset'].dtype == bool and obs['reset']
    assert obs[key].shape == ((6, 5, 3) if kind == 'image' else (5,))
    for t in (1, 2, 3):
        obs, reward, done, info = env.step(_onehot(t))
        assert reward == 0.5 * t == obs['reward'] and done == (t == 3) and not obs['reset'] and bool(obs['terminal']) == (t == 3)
        assert np.array_equal(obs['action'], _onehot(t)) and (obs[key] == t).all()
    assert all(isinstance(a, np.ndarray) and a.shape == (A,) for a in raw.actions)      # one-hot actions are passed on as they are
    with pytest.raises(ValueError, match='shape'):
        env.step(np.zeros(A + 1))


def test_wrapper_discrete_actions_time_limit_no_terminal_and_truncation():
    raw = RawEnv('vector', 10)
    env = wrap_env(raw, A, time_limit=3, discrete=True)
    for episode in range(2):                                   # the limit counts from every reset
        env.reset()
        for t in (1, 2, 3):
            obs, _, done, info = env.step(_onehot(t % A))
            assert done == (t == 3) and bool(info.get('time_limit')) == (t == 3) and not obs['terminal']
            assert np.array_equal(obs['action'], _onehot(t % A))
    assert raw.actions == [1, 2, 3] * 2 and all(type(a) is int for a in raw.actions)
    # the environment ends first: terminal
    env = wrap_env(RawEnv('vector', 2), A, time_limit=3)
    env.reset()
    assert not env.step(_onehot(0))[0]['terminal']
    obs, _, done, info = env.step(_onehot(0))
    assert done and obs['terminal'] and 'time_limit' not in info
    # no_terminal
    env = wrap_env(RawEnv('vector', 1), A, no_terminal=True)
    env.reset()
    obs, _, done, _ = env.step(_onehot(0))
    assert done and not obs['terminal']
    # 'TimeLimit.truncated'
    env = wrap_env(RawEnv('vector', 1, truncated_key=True), A)
    env.reset()
    obs, _, done, info = env.step(_onehot(0))
    assert done and not obs['terminal'] and 'TimeLimit.truncated' in info


def test_wrapper_takes_five_tuple_steps_and_two_tuple_resets():
    for length, terminated in ((2, True), (3, False)):
        env = wrap_env(RawEnv('dict', length, api=5), A)
        obs = env.reset()
        assert isinstance(obs, dict) and obs['reset'] and 'note' not in obs
        for t in range(1, length + 1):
            out = env.step(_onehot(1))
            assert len(out) == 4
            obs, reward, done, info = out
            assert done == (t == length) and reward == 0.5 * t
        assert bool(obs['terminal']) == terminated and bool(info.get('time_limit')) == (not terminated)


def test_wrapped_raw_environments_through_collect_and_the_replay_reader(tmp_path):
    conf = config.load_config('defaults', 'vectorenv', action_dim=A, env_time_limit=4)
    assert config.load_config('defaults').env_time_limit == 0 and config.load_config('defaults').env_no_terminal is False
    raws = [RawEnv('vector', 3), RawEnv('vector', 9)]          # the second runs into the time limit
    envs = wrap_envs(raws, conf, discrete=True)
    assert [(e.action_dim, e.time_limit, e.no_terminal, e.discrete) for e in envs] == [(A, 4, False, True)] * 2
    repo = R.LocalEpisodeRepository(str(tmp_path))
    out = collect(envs, ScriptPolicy(2), EpisodeRecorder(repo, 2, steps_per_npz=10 ** 6), 12)
    assert out['episodes'] == 4 + 3 and len(out['files']) == 1
    eps = _episodes(repo)
    assert sorted(len(e['reward']) - 1 for e in eps.values()) == [3, 3, 3, 3, 4, 4, 4]
    for e in eps.values():
        assert bool(e['terminal'][-1]) == (len(e['reward']) == 4) and not e['terminal'][:-1].any()
    T = sum(len(e['reward']) for e in eps.values())
    batch = R.SequentialReplay(repo, batch_length=T, batch_size=1, skip_first=False).fill()
    got = R.preprocess_batch(batch, A, image_key=None)
    assert got['action'].shape == (T, 1, A) and got['vecobs'].shape == (T, 1, 5) and got['reset'].sum() == 7
    assert got['terminal'].sum() == 4 and np.array_equal(got['action'].sum(-1)[:, 0], 1.0 - got['reset'][:, 0])
    assert raws[0].actions[:3] == [0, 1, 2] and all(type(a) is int for a in raws[0].actions)


def test_run_refuses_eval_envs_without_a_repository_and_a_split_without_one(tmp_path):
    from pydreamer_amd.train import run
    repo = R.LocalEpisodeRepository(str(tmp_path))
    conf = config.load_config('defaults', 'vectorenv')
    with pytest.raises(ValueError, match='eval_repository'):
        run(conf, repo, envs=_envs([[4]]), eval_envs=_envs([[4]]), env_steps_per_grad_step=1, logdir=str(tmp_path / 'log'))
    with pytest.raises(ValueError, match='test_repository'):
        run(conf, repo, envs=_envs([[4]]), split_fraction=0.25, env_steps_per_grad_step=1, logdir=str(tmp_path / 'log'))
    assert not os.path.exists(str(tmp_path / 'log'))
