"""-m gpu: the collection loop closed over the device - toy environments driven by NetworkPolicy(per_env=True) through
collect() into episode files, the files read back by DeviceReplay, one gradient step on that batch.  One loop per configuration:
the tiny `vectorenv` model (no frames) and the tiny cnn model at 64 x 64 frames, built as the inference fixtures build them."""
import numpy as np
import pytest
import torch

from oracle import dreamer_oracle as O
from pydreamer_amd import replay as R
from pydreamer_amd.collect import EpisodeRecorder, collect
from pydreamer_amd.policy import METRIC_KEYS, NetworkPolicy, StepPreprocessor
from tests.test_collect_cpu import _closed_in_order, _episode_fields
from tests.test_gpu_act import _build, _fixture

pytestmark = pytest.mark.gpu
DEV = 'cuda'


class ToyEnv:
    """The wrapped-environment protocol on a toy: episodes of lengths[e % len] steps (4 to 7), the reward a function of the action
    taken, observations a fixed function of (idx, episode, step).  Odd episodes terminate, even ones run into a time limit."""

    def __init__(self, idx, lengths, A, vec_dim=0, frame=None):
        assert all(4 <= n <= 7 for n in lengths)
        self.idx, self.lengths, self.A, self.vec_dim, self.frame = idx, lengths, A, vec_dim, frame
        self.episodes, self.starts, self.steps, self.t = [], [], 0, 0

    def _obs(self, action, reward, terminal, reset):
        rs = np.random.RandomState(1000 * self.idx + 37 * len(self.episodes) + self.t)
        obs = dict(action=action, reward=np.array(reward, np.float32), terminal=np.array(terminal), reset=np.array(reset))
        if self.vec_dim:
            obs['vecobs'] = rs.randn(self.vec_dim).astype(np.float32)
        if self.frame:
            obs['image'] = rs.randint(0, 256, self.frame).astype(np.uint8)
        self.episodes[-1].append(obs)
        return dict(obs)

    def reset(self):
        self.episodes.append([])
        self.starts.append(self.steps)
        self.t = 0
        return self._obs(np.zeros(self.A, np.float32), 0.0, False, True)

    def step(self, action):
        assert action.shape == (self.A,) and action.dtype == np.float32 and action.sum() == 1.0 and action.max() == 1.0
        e = len(self.episodes) - 1
        self.t += 1
        self.steps += 1
        done = self.t >= self.lengths[e % len(self.lengths)]
        reward = 0.5 * int(action.argmax()) - 0.25 * self.t
        return self._obs(action, reward, bool(done and e % 2 == 1), False), reward, done, {}


def _models(which):
    from pydreamer_amd import config
    if which == 'vectorenv':
        g, model, obs = _fixture('tiny_vectorenv_inference')
        assert 'image' not in obs and not model.conf.image_key
        return model, dict(vec_dim=obs['vecobs'].shape[-1]), None
    oconf = O.tiny_conf()
    model = _build(config.load_config('defaults', 'atari', **vars(oconf)), params=O.make_params(oconf, seed=0))
    return model, dict(frame=(64, 64, oconf.image_channels)), 'image'


@pytest.mark.parametrize('which', ['vectorenv', 'cnn'])
def test_collect_replay_and_one_gradient_step(hip, tmp_path, which):
    model, env_kw, image_key = _models(which)
    conf = model.conf
    A, B, steps = conf.action_dim, 3, 40
    envs = [ToyEnv(b, lengths, A, **env_kw) for b, lengths in enumerate([[4, 6], [7, 5], [5, 4, 6]])]
    repo = R.LocalEpisodeRepository(str(tmp_path))
    policy = NetworkPolicy(model, StepPreprocessor(A, clip_rewards='tanh', image_key=image_key, batched=True), batch_size=B, per_env=True,
                           action_noise=0.2)
    torch.manual_seed(3)
    out = collect(envs, policy, EpisodeRecorder(repo, B, steps_per_npz=10 ** 6), steps)
    order = _closed_in_order(envs)
    assert out['steps'] == B * steps and out['episodes'] == len(order) >= 18 and len(out['files']) == 1
    want = {k: np.concatenate([_episode_fields(envs[i], e)[k] for i, e in order]) for k in envs[0].episodes[0][0]}
    rows = len(want['reset'])
    assert repo.count_steps() == (1, rows - len(order), len(order))
    with np.load(out['files'][0]) as f:
        for k in METRIC_KEYS:      # every policy call landed in its row: finite except the one NaN per episode
            col = f[k]
            assert col.shape == (rows,) and int(np.isnan(col).sum()) == len(order), k
            assert np.array_equal(np.isnan(col), want['reset'] if k == 'action_prob' else np.append(want['reset'][1:], True)), k
        assert (f['action_prob'][~want['reset']] > 0).all() and (f['action_prob'][~want['reset']] <= 1).all()
        assert (f['policy_entropy'][~np.isnan(f['policy_entropy'])] > 0).all()
    # the files through the device-resident feed: every column's first window is the file's first T rows
    T, Bt = conf.batch_length, conf.batch_size
    assert rows >= T
    dr = R.DeviceReplay(R.SequentialReplay(repo, T, Bt, skip_first=False, seed=0), A, DEV, clip_rewards='tanh', image_key=image_key)
    obs = dr.next()
    for b in range(Bt):
        assert np.array_equal(obs['reward'][:, b].cpu().numpy(), np.tanh(want['reward'][:T].astype(np.float32)))
        assert np.array_equal(obs['action'][:, b].cpu().numpy(), want['action'][:T])
        assert np.array_equal(obs['reset'][:, b].cpu().numpy(), want['reset'][:T])
        if image_key:
            assert np.array_equal(obs['image'][:, b].cpu().numpy(), want['image'][:T])
        else:
            assert 'image' not in obs and np.array_equal(obs['vecobs'][:, b].cpu().numpy(), want['vecobs'][:T])
    assert float(obs['action'][1:].sum()) == (T - 1) * Bt and float(obs['reward'].abs().max()) > 0
    # one gradient step on it
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    losses, state, metrics, tensors, _ = model.training_step(obs, model.init_state(Bt))
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    gm = model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
    torch.cuda.synchronize()
    dr.close()
    assert all(np.isfinite(float(x.detach())) for x in losses), [float(x.detach()) for x in losses]
    assert all(np.isfinite(float(v)) for v in gm.values()) and float(gm['grad_norm']) > 0, {k: float(v) for k, v in gm.items()}
