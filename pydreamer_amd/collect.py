"""The collection loop (generator.py:123-257 for B environments): a policy drives a list of environments as one batch,
and what happened becomes the episode files SequentialReplay / ReplayFeed / DeviceReplay read.

  * `EpisodeRecorder`  - the per-environment row lists of the reference's CollectWrapper (wrappers.py:75-93), the three policy
    columns of generator.py:140-149 and the npz writer of generator.py:218-253, for B environments at once;
  * `collect`          - reset, stack, one policy call per step, step, record, reset what is done;
  * `Collector`        - the same loop for a trainer that alternates collecting and training: the current observations and the
    recorder's open episodes live across run() calls; run_episodes(n) runs until n episodes have closed;
  * `EpisodeStats`     - the generator's per-episode metrics and their aggregation (generator.py:167-216), fed by the recorder's
    on_episode hook.

Host code only: the device work of a step is the policy's (policy.NetworkPolicy: one Dreamer.act call, one device-to-host copy).
Not here, and not needed by the readers: gym adapters (envs.py restates the wrappers as behaviour), mlflow logging, checkpoint
polling and rate limiting (generator.py:103-121; train.run turns it into a schedule)."""
import time

import numpy as np

from .policy import METRIC_KEYS


def stack_obs(obs_list):
    """B observation dicts -> one dict of arrays with a leading (B,) axis."""
    keys = list(obs_list[0])
    for o in obs_list[1:]:
        if list(o) != keys:
            raise ValueError(f'the environments emit different fields: {keys} and {list(o)}')
    return {k: np.stack([np.asarray(o[k]) for o in obs_list]) for k in keys}


class EpisodeRecorder:
    """Turns the steps of `num_envs` environments into episode files of `repository` (replay.LocalEpisodeRepository, or anything
    with its count_steps() and save_data(data, episode_from, episode_to)).

    add(obs, done, metrics=None, envs=None) takes one step of all environments.  `obs`: dict of arrays with a leading (B,) axis,
    the fields the reference's wrapped environment emits (wrappers.py:43-72) - action, reward, terminal, reset - plus the
    observation fields; row b is what environment b returned from reset() (reset = True: the row opens an episode, and an
    unfinished one of that environment is dropped) or from step().  `done`: (B,) bools, the row closes its episode.  `metrics`:
    the policy's per-environment dict (NetworkPolicy(per_env=True): policy_value, action_prob, policy_entropy, (B,) each) of the
    call that chose the action this row carries, or None; rows with reset = True carry no action and take none.  `envs`: the
    environments the leading axis holds, for a call that carries the rows of some of them only (the reset rows after a step);
    all of them, in order, by default.

    A closed episode is one dict, its fields stacked over time.  With metrics, policy_value and policy_entropy get a trailing
    NaN (no policy call on the last row) and action_prob a leading one (no action on the first); without, all three are NaN
    with the shape of `reward` - generator.py:140-149, so every file has the same keys; float64 as there.  Closed episodes queue
    up; when their steps (rows - 1 each, generator.py:222) reach steps_per_npz they are concatenated and written as ONE file: a
    (T,H,W,C) `image` as `image_t` (H,W,C,T), an integer class image as it is (generator.py:246-252).  Episode numbers go on from
    repository.count_steps(); episodes are numbered in the order they close, the lower environment index first within a step.
    flush() writes what is queued.  chunk=False (the default) always writes the queue whole, as ONE file.  chunk=True follows
    generator.py:237-240: a queue of 2 steps_per_npz steps or more is cut as chunk_episode_data (tools.py:269-278) cuts it - with
    n = rows - 1 into n // steps_per_npz pieces, piece i the rows up to n (i + 1) // pieces + 1 - and written as one file per
    piece, the piece's number in the file name; a shorter queue is written as with chunk=False.

    Keyword-only, off by default.  on_episode: called from _close with the closed episode dict (policy columns attached) before
    the dict is queued - EpisodeStats.add_episode behind a closure.  repository2, split_fraction, rng: the split of
    generator.py:244 - one draw per written queue, rng.rand() > split_fraction => repository, otherwise repository2; `rng` is a
    np.random.RandomState (RandomState(0) by default); one episode counter serves both, steps_saved counts the first
    repository's steps only (generator.py:255-257).  With split_fraction == 0 no draw is made."""

    def __init__(self, repository, num_envs, steps_per_npz=1000, chunk=False, *, on_episode=None, repository2=None,
                 split_fraction=0.0, rng=None):
        self.repository, self.num_envs, self.steps_per_npz = repository, int(num_envs), int(steps_per_npz)
        self.chunk = bool(chunk)
        if self.num_envs < 1:
            raise ValueError(f'num_envs={num_envs}')
        self.on_episode, self.repository2, self.split_fraction = on_episode, repository2, float(split_fraction)
        if not 0.0 <= self.split_fraction <= 1.0:
            raise ValueError(f'split_fraction={split_fraction}: expected 0 ... 1')
        if self.split_fraction > 0 and repository2 is None:
            raise ValueError(f'split_fraction={split_fraction} needs repository2')
        self.rng = rng if rng is not None else np.random.RandomState(0)
        self.episodes = int(repository.count_steps()[2])      # the number the next closed episode gets
        self.rows = [[] for _ in range(self.num_envs)]        # per environment: the open episode's row dicts
        self.mets = [[] for _ in range(self.num_envs)]        # per environment: (value, prob, entropy) per policy call, or None
        self.queue, self.queued_steps = [], 0
        self.steps_saved, self.files = 0, []

    def add(self, obs, done, metrics=None, envs=None):
        envs = range(self.num_envs) if envs is None else [int(e) for e in envs]
        n = len(envs)
        done = np.asarray(done, dtype=bool).reshape(-1)
        if done.shape != (n,):
            raise ValueError(f'done has shape {done.shape}, expected ({n},)')
        for k in ('action', 'reward', 'terminal', 'reset'):
            if k not in obs:
                raise KeyError(f'the observation lacks {k!r} (fields: {list(obs)})')
        obs = {k: np.asarray(v) for k, v in obs.items() if k not in METRIC_KEYS}
        for k, v in obs.items():
            if v.shape[:1] != (n,):
                raise ValueError(f'{k} has shape {v.shape}, expected a leading axis of {n}')
        if metrics is not None:
            metrics = [np.asarray(metrics[k], dtype=np.float64).reshape(-1) for k in METRIC_KEYS]
            if any(m.shape != (n,) for m in metrics):
                raise ValueError(f'per-environment metrics have shapes {[m.shape for m in metrics]}, expected ({n},) each')
        for i, b in enumerate(envs):
            if not 0 <= b < self.num_envs:
                raise ValueError(f'environment {b} of {self.num_envs}')
            first = bool(obs['reset'][i])
            if first:
                self.rows[b], self.mets[b] = [], []
            elif not self.rows[b]:
                raise ValueError(f'environment {b}: a step row without an open episode (the first row of an episode has reset = True)')
            self.rows[b].append({k: v[i].copy() for k, v in obs.items()})
            if not first:
                self.mets[b].append(None if metrics is None else tuple(m[i] for m in metrics))
            if done[i]:
                self._close(b)
        if self.queued_steps >= self.steps_per_npz:
            self.flush()

    def _close(self, b):
        rows, mets = self.rows[b], self.mets[b]
        self.rows[b], self.mets[b] = [], []
        data = {k: np.array([r[k] for r in rows]) for k in rows[0]}
        nan = np.full(data['reward'].shape, np.nan)
        if mets and all(m is not None for m in mets):
            value, prob, ent = (np.array([m[j] for m in mets], dtype=np.float64) for j in range(3))
            data['policy_value'] = np.concatenate([value, [np.nan]])       # no policy call on the last row
            data['policy_entropy'] = np.concatenate([ent, [np.nan]])
            data['action_prob'] = np.concatenate([[np.nan], prob])         # no action on the first row
        else:
            data['policy_value'], data['policy_entropy'], data['action_prob'] = nan, nan.copy(), nan.copy()
        if self.on_episode is not None:
            self.on_episode(data)
        self.queue.append(data)
        self.queued_steps += len(rows) - 1
        self.episodes += 1

    def flush(self):
        """Writes the queued episodes as one file - with chunk=True and 2 steps_per_npz steps or more queued, as several; returns the
        path of the (last) file written (None with an empty queue)."""
        if not self.queue:
            return None
        datas, steps = self.queue, self.queued_steps
        self.queue, self.queued_steps = [], 0
        data = {k: np.concatenate([d[k] for d in datas], axis=0) for k in datas[0]}
        if self.chunk and steps >= 2 * self.steps_per_npz:
            pieces = list(enumerate(chunk_episode_data(data, self.steps_per_npz)))
        else:
            pieces = [(None, data)]
        repo = self.repository
        if self.split_fraction > 0 and not self.rng.rand() > self.split_fraction:
            repo = self.repository2
        for seq, piece in pieces:
            if 'image' in piece and piece['image'].ndim == 4:      # THWC => HWCT for better compression; a class image stays
                piece['image_t'] = piece.pop('image').transpose(1, 2, 3, 0)
            path = repo.save_data(piece, self.episodes - len(datas), self.episodes - 1, seq)
            self.files.append(path)
        if repo is self.repository:      # only the training repository's steps: prefill and the step ratio go by them
            self.steps_saved += steps
        return path


def chunk_episode_data(data, min_length):
    """The cut rule of tools.py:269-278: with steps = rows - 1 (the first reset row is free: 2000 steps become 1001 + 1000 rows) the
    rows go into steps // min_length consecutive pieces of min_length ... 2 min_length - 1 steps each.  Returns dicts of views."""
    steps = len(data['reward']) - 1
    pieces = steps // min_length
    bounds = [0] + [steps * (i + 1) // pieces + 1 for i in range(pieces)]
    return [{k: v[a:z] for k, v in data.items()} for a, z in zip(bounds, bounds[1:])]


def collect(envs, policy, recorder, num_steps):
    """Drives the B = len(envs) environments for `num_steps` steps of all of them (num_steps policy calls, B num_steps transitions)
    and flushes the recorder.  Environment protocol - the reference's wrapped one (wrappers.py:43-72), no gym needed:
    reset() -> obs dict, step(action) -> (obs dict, reward, done, info), the dict carrying action / reward / terminal / reset.
    `policy`: (stacked obs dict) -> (actions (B, A) - (A,) for B = 1 -, metrics); NetworkPolicy(batch_size=B, per_env=True),
    RandomPolicy, or any callable of that shape (a metrics dict without the per-environment columns records NaNs).  Every
    environment is reset first.  A done environment is reset in place: the row the policy sees next for it carries reset = True,
    on which the world model zeroes that row's state, so the policy's carried state needs no other care.  Episodes still open
    when the loop stops are not written.  Returns dict(steps, episodes, files): transitions taken, episodes closed, files
    written by this call."""
    B = len(envs)
    if B != recorder.num_envs:
        raise ValueError(f'{B} environments, the recorder was built for {recorder.num_envs}')
    num_steps = int(num_steps)
    episodes0, files0 = recorder.episodes, len(recorder.files)
    cur = [env.reset() for env in envs]
    recorder.add(stack_obs(cur), np.zeros(B, bool))
    for _ in range(num_steps):
        action, metrics = policy(stack_obs(cur))
        action = np.asarray(action).reshape(B, -1)
        done = np.zeros(B, bool)
        for b, env in enumerate(envs):
            cur[b], _, d, _ = env.step(action[b])
            done[b] = bool(d)
        per_env = metrics if metrics and all(k in metrics and np.size(metrics[k]) == B for k in METRIC_KEYS) else None
        recorder.add(stack_obs(cur), done, per_env)
        again = np.flatnonzero(done)
        if len(again):
            for b in again:
                cur[b] = envs[b].reset()
            recorder.add(stack_obs([cur[b] for b in again]), np.zeros(len(again), bool), envs=again)
    recorder.flush()
    return dict(steps=B * num_steps, episodes=recorder.episodes - episodes0, files=recorder.files[files0:])


class Collector:
    """collect() for a loop that alternates collecting and training: run(num_steps) drives the environments for num_steps steps of
    all of them and can be called again - the current observations and the recorder's open episodes are kept, so an episode that
    spans two calls is written whole.  The environments are reset once, by the first run().  Files appear when the recorder's
    steps_per_npz is reached, on flush() (the closed episodes queued so far) and on close() (the same; episodes still open are
    not written).  Wherever no episode is open between two calls, run(k) twice records what collect() records in 2 k steps.
    run_episodes(n) is run() with another stop rule: until at least n episodes have closed in the call.
    `steps` counts the transitions taken so far, B per step, and is current while a step is being recorded (the on_episode hook
    reads it); seconds() is the time spent inside run() / run_episodes() so far."""

    def __init__(self, envs, policy, recorder):
        if len(envs) != recorder.num_envs:
            raise ValueError(f'{len(envs)} environments, the recorder was built for {recorder.num_envs}')
        self.envs, self.policy, self.recorder = list(envs), policy, recorder
        self.cur = None
        self.steps = 0
        self._seconds, self._since = 0.0, None

    def seconds(self):
        return self._seconds + (time.perf_counter() - self._since if self._since is not None else 0.0)

    def _step(self):
        envs, recorder, cur, B = self.envs, self.recorder, self.cur, len(self.envs)
        action, metrics = self.policy(stack_obs(cur))
        action = np.asarray(action).reshape(B, -1)
        done = np.zeros(B, bool)
        for b, env in enumerate(envs):
            cur[b], _, d, _ = env.step(action[b])
            done[b] = bool(d)
        self.steps += B
        per_env = metrics if metrics and all(k in metrics and np.size(metrics[k]) == B for k in METRIC_KEYS) else None
        recorder.add(stack_obs(cur), done, per_env)
        again = np.flatnonzero(done)
        if len(again):
            for b in again:
                cur[b] = envs[b].reset()
            recorder.add(stack_obs([cur[b] for b in again]), np.zeros(len(again), bool), envs=again)

    def _run(self, more):
        recorder, B = self.recorder, len(self.envs)
        steps0, episodes0, files0 = self.steps, recorder.episodes, len(recorder.files)
        self._since = time.perf_counter()
        try:
            if self.cur is None:
                self.cur = [env.reset() for env in self.envs]
                recorder.add(stack_obs(self.cur), np.zeros(B, bool))
            while more((self.steps - steps0) // B, recorder.episodes - episodes0):
                self._step()
        finally:
            self._seconds, self._since = self.seconds(), None
        return dict(steps=self.steps - steps0, episodes=recorder.episodes - episodes0, files=recorder.files[files0:])

    def run(self, num_steps):
        """Returns dict(steps, episodes, files) of this call: transitions taken, episodes closed, files written."""
        num_steps = int(num_steps)
        return self._run(lambda steps, episodes: steps < num_steps)

    def run_episodes(self, n):
        """Runs until at least `n` episodes have closed in this call - more when several environments close on the same step.
        Bookkeeping and return value as run()."""
        n = int(n)
        return self._run(lambda steps, episodes: episodes < n)

    def flush(self):
        return self.recorder.flush()

    def close(self):
        """Writes the queued episodes; the open ones are dropped, and the next run() resets the environments."""
        path = self.recorder.flush()
        self.recorder.rows = [[] for _ in range(self.recorder.num_envs)]
        self.recorder.mets = [[] for _ in range(self.recorder.num_envs)]
        self.cur = None
        return path


def discount(x, gamma):
    """y[t] = x[t] + gamma y[t+1], y[T] = 0 (tools.py:226-228) in float64."""
    x = np.asarray(x, dtype=np.float64)
    y = np.zeros_like(x)
    acc = np.zeros(x.shape[1:])
    for t in range(len(x) - 1, -1, -1):
        acc = x[t] + gamma * acc
        y[t] = acc
    return y


class EpisodeStats:
    """The generator's per-episode metrics and their aggregation (generator.py:167-216), keys `prefix/...`.

    add_episode(data, steps, steps_saved, episodes, seconds): `data` is one CLOSED episode - the dict EpisodeRecorder._close
    builds, policy columns attached; `steps`: the collector's transitions so far, all environments; `steps_saved`: the steps in
    the training repository; `episodes`: the episode count, this one included; `seconds`: the time the collector has spent
    collecting so far (Collector.seconds()).  Per episode: policy_value / policy_entropy / action_prob as the mean over the
    column's non-NaN entries (absent when the column is all NaN: a policy without per-environment metrics), episode_length =
    rows - 1, steps, env_steps = steps action_repeat, steps_saved, episodes, return, return_cum (the mean of the last 100
    returns), return_discounted (the mean of discount(reward), with mean(reward) / (1 - gamma) added to the last reward when the
    episode did not terminate), policy_value_terminal = policy_value[-2] - reward[-1] for a terminated episode, and the three
    goals_* keys for an episode with goals_visage.  A NaN value is not appended.  ready(): log_every returns are held.  pop():
    the mean per key, return_max, and fps - the transitions taken per second of collecting time since the previous pop (B
    environments advance in lock-step, so the reference's per-episode wall-clock rate has no meaning here) - and the lists are
    cleared; the window of 100 returns stays.  No _timestamp."""

    def __init__(self, prefix='agent', gamma=0.99, log_every=10, action_repeat=1):
        self.prefix, self.gamma, self.log_every, self.action_repeat = prefix, float(gamma), int(log_every), int(action_repeat)
        self.returns = []           # the last 100
        self.agg = {}               # key -> values since the last pop
        self._mark = self._last = (0, 0.0)      # (steps, seconds) at the previous pop / at the last episode

    def add_episode(self, data, steps, steps_saved, episodes, seconds):
        p = self.prefix
        reward, terminal = np.asarray(data['reward']), np.asarray(data['terminal'])
        m = {}
        for k in METRIC_KEYS:
            col = np.asarray(data[k], dtype=np.float64) if k in data else np.zeros(0)
            col = col[~np.isnan(col)]
            if len(col):
                m[f'{p}/{k}'] = col.mean()
        ret = reward.sum()
        self.returns = (self.returns + [ret])[-100:]
        m.update({f'{p}/episode_length': len(reward) - 1,
                  f'{p}/steps': steps,
                  f'{p}/steps_saved': steps_saved,
                  f'{p}/env_steps': steps * self.action_repeat,
                  f'{p}/episodes': episodes,
                  f'{p}/return': ret,
                  f'{p}/return_cum': np.array(self.returns).mean()})
        rewards_v = reward.astype(np.float64)
        if not terminal[-1]:
            rewards_v[-1] += rewards_v.mean() / (1.0 - self.gamma)
        m[f'{p}/return_discounted'] = discount(rewards_v, self.gamma).mean()
        if terminal[-1] and 'policy_value' in data and len(reward) >= 2:
            m[f'{p}/policy_value_terminal'] = data['policy_value'][-2] - reward[-1]      # zero for a critic that is right
        if 'goals_visage' in data:
            visage = np.asarray(data['goals_visage'])
            seen = visage < 1e5
            m[f'{p}/goals_seen_avg'] = seen.sum(axis=-1).mean()
            m[f'{p}/goals_seen_last'] = seen[-1].sum()
            m[f'{p}/goals_seenage'] = (visage * seen).sum() / seen.sum() if seen.any() else np.nan
        for k, v in m.items():
            if not np.isnan(v):
                self.agg.setdefault(k, []).append(float(v))
        self._last = (steps, seconds)

    def ready(self):
        return self.log_every > 0 and len(self.agg.get(f'{self.prefix}/return', ())) >= self.log_every

    def pop(self):
        """{key: mean}, plus return_max and fps; {} when no episode was added since the last pop."""
        if not self.agg:
            return {}
        p = self.prefix
        out = {k: float(np.array(v).mean()) for k, v in self.agg.items()}
        out[f'{p}/return_max'] = float(np.array(self.agg[f'{p}/return']).max())
        dsteps, dsec = self._last[0] - self._mark[0], self._last[1] - self._mark[1]
        if dsec > 0 and dsteps > 0:      # (two pops within one step have taken no transition between them)
            out[f'{p}/fps'] = dsteps / dsec
        self._mark = self._last
        self.agg = {}
        return out
