"""-m gpu: the trainer loop on the device.

  run()       the tiny `vectorenv` model on a scripted environment of this file (T 5, B 3, prefill 40 steps; n_steps 6, log_interval 3,
              save_interval 3, eval_interval 6): the logger is called at steps 3 and 6; every logged train/<name> EQUALS
              sum(vals) / len(vals) of the per-step packed_metrics_host() values an on_step hook gathered in the same run, under the
              reference's NaN / finite filters (train.py:204-210); the _max keys; the four data statistics against numpy on the
              batches at the dm_batch_stats bar.  Without the hook packed_metrics_host() is never called and read_and_reset() runs
              exactly twice.  latest.pt loads into a fresh model and optimizers, every tensor equal, epoch 6.  test/ and eval/ keys
              are logged.
  evaluate()  three hand-made batches - all columns reset, some, none - on the tiny cnn model (eval_samples 2) and the tiny minigrid
              map-probe model (eval_samples 1) against a loop written here that follows train.py:325-399 with .item() calls under the
              same torch.manual_seed: equal, or within the metric bar of DESIGN 4.13 (1e-4 relative / 5e-6 absolute)."""
import ast
import math
import os
import warnings
from argparse import Namespace
from collections import defaultdict

import numpy as np
import pytest
import torch

from oracle import dreamer_oracle as O
from pydreamer_amd import config, replay as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
GRAD_NORMS = ('grad_norm', 'grad_norm_probe', 'grad_norm_actor', 'grad_norm_critic')


class LoopEnv:
    """The wrapped-environment protocol on a script: episodes of lengths[e % len] steps - 10 to 13 here, two windows of T = 5 and
    more, so that the second evaluation batch continues its columns -, vector observations, the reward a function of the action
    taken; odd episodes terminate, even ones run into a time limit."""

    def __init__(self, idx, lengths, A, vec_dim):
        self.idx, self.lengths, self.A, self.vec_dim, self.episode, self.t = idx, lengths, A, vec_dim, -1, 0

    def _obs(self, action, reward, terminal, reset):
        rs = np.random.RandomState(1000 * self.idx + 37 * self.episode + self.t)
        return dict(action=action, reward=np.array(reward, np.float32), terminal=np.array(terminal), reset=np.array(reset),
                    vecobs=rs.randn(self.vec_dim).astype(np.float32))

    def reset(self):
        self.episode, self.t = self.episode + 1, 0
        return self._obs(np.zeros(self.A, np.float32), 0.0, False, True)

    def step(self, action):
        self.t += 1
        done = self.t >= self.lengths[self.episode % len(self.lengths)]
        reward = 0.5 * int(np.argmax(action)) - 0.25 * self.t
        return self._obs(np.asarray(action, np.float32), reward, bool(done and self.episode % 2 == 1), False), reward, done, {}


def _loop_conf():
    g = np.load(os.path.join(GOLD, 'tiny_vectorenv_inference.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    conf = config.load_config('defaults', 'vectorenv', **{**vars(oconf), **extra})
    assert (conf.batch_length, conf.batch_size) == (5, 3) and not conf.image_key
    return Namespace(**{**vars(conf), **dict(device='cuda:0', n_steps=6, log_interval=3, save_interval=3, eval_interval=6,
                                             generator_prefill_steps=40, test_batches=2, eval_batches=2, test_batch_size=3,
                                             eval_batch_size=3)})


def _run(tmp_path, on_step):
    from pydreamer_amd.train import run
    conf = _loop_conf()
    data_dir, logdir = str(tmp_path / 'episodes'), str(tmp_path / 'log')
    os.makedirs(data_dir)
    repo = R.LocalEpisodeRepository(data_dir)
    envs = [LoopEnv(b, lengths, conf.action_dim, conf.vecobs_size) for b, lengths in enumerate([[11, 12], [12, 10], [13, 11, 10]])]
    logged = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        steps = run(conf, repo, test_repository=repo, envs=envs, logdir=logdir, logger=lambda m, s: logged.append((s, dict(m))),
                    env_steps_per_grad_step=3, on_step=on_step, seed=1, steps_per_npz=10)
    failed = [str(w.message) for w in caught if 'Evaluation failed' in str(w.message)]
    assert not failed, failed
    assert steps == 6 and repo.count_steps()[1] >= 40 + 5 * 3
    return conf, logdir, logged


def test_logged_metrics_equal_the_per_step_values_and_the_checkpoint_loads(hip, tmp_path):
    from pydreamer_amd.models import Dreamer
    from pydreamer_amd.train import load_checkpoint
    per_step, batches, seen = [], [], {}

    def on_step(step, model, obs, tensors):
        per_step.append((step, model.packed_metrics_host()))
        batches.append({k: obs[k].cpu().numpy() for k in ('reward', 'reset', 'terminal')})
        seen['model'] = model

    conf, logdir, logged = _run(tmp_path, on_step)
    assert [s for s, _ in per_step] == [1, 2, 3, 4, 5, 6]
    train = [(s, m) for s, m in logged if 'train/steps' in m]
    assert [s for s, _ in train] == [3, 6], [s for s, _ in logged]
    names = list(per_step[0][1])
    assert {'loss_model', 'loss_kl', 'loss_actor', 'policy_entropy'} <= set(names) and set(GRAD_NORMS) <= set(names)
    for j, (s, m) in enumerate(train):
        assert m['train/steps'] == s and m['train/fps'] > 0
        rows = [v for _, v in per_step[3 * j:3 * j + 3]]
        for k in names:
            keep = (lambda v: math.isfinite(v)) if k in GRAD_NORMS else (lambda v: not math.isnan(v))
            vals = [r[k] for r in rows if keep(r[k])]
            if not vals:
                assert f'train/{k}' not in m, k
                continue
            assert m[f'train/{k}'] == sum(vals) / len(vals), (s, k, m[f'train/{k}'], vals)
            if k in GRAD_NORMS:
                assert m[f'train/{k}_max'] == max(vals), (s, k)
            else:
                assert f'train/{k}_max' not in m
        assert m['train/loss_model'] != 0 and m['train/grad_norm'] > 0
        # the data statistics: per step one fp32 rounding of the float64 mean, then the float64 mean over the three steps
        bs = batches[3 * j:3 * j + 3]
        for k in ('reward', 'terminal'):
            x = [b[k].astype(np.float64) for b in bs]
            ref = float(np.mean([v.mean() for v in x]))
            bar = float(np.mean([2.0 ** -23 * abs(v.mean()) + 1e-12 * np.abs(v).mean() for v in x]))
            print(f'step {s} data_{k}: logged {m["train/data_" + k]:.9g} float64 {ref:.9g} bar {bar:.3e}')
            assert abs(m[f'train/data_{k}'] - ref) <= bar, (s, k, m[f'train/data_{k}'], ref, bar)
        assert m['train/data_reset'] == sum(float(np.float32(b['reset'].sum()) / np.float32(b['reset'].size)) for b in bs) / 3
        assert m['train/data_reward_max'] == max(float(b['reward'].max()) for b in bs)
        assert any((b['reward'] != 0).any() for b in bs)
    assert any(b['reset'].any() for b in batches)
    # the checkpoint of step 6 in a fresh model and fresh optimizers
    path = os.path.join(logdir, 'checkpoints', 'latest.pt')
    assert os.path.exists(path)
    ck = torch.load(path, map_location='cpu')
    assert list(ck) == ['epoch', 'model_state_dict'] + [f'optimizer_{i}_state_dict' for i in range(4)] and ck['epoch'] == 6
    fresh = Dreamer(conf).to(DEV)
    fopts = fresh.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    assert load_checkpoint(path, fresh, fopts, map_location=DEV) == 6
    trained = seen['model'].state_dict()
    loaded = fresh.state_dict()
    assert list(trained) == list(loaded) == list(ck['model_state_dict'])
    for k in trained:
        assert torch.equal(trained[k], loaded[k]) and torch.equal(loaded[k].cpu(), ck['model_state_dict'][k]), k

    def tensors_of(x, pre=''):
        if torch.is_tensor(x):
            yield pre, x
        elif isinstance(x, dict):
            for k, v in x.items():
                yield from tensors_of(v, f'{pre}/{k}')
        elif isinstance(x, (list, tuple)):
            for i, v in enumerate(x):
                yield from tensors_of(v, f'{pre}/{i}')

    n = 0
    for i, opt in enumerate(fopts):
        got, want = dict(tensors_of(opt.state_dict())), dict(tensors_of(ck[f'optimizer_{i}_state_dict']))
        assert list(got) == list(want)
        for k in got:
            assert torch.equal(got[k].cpu(), want[k].cpu()), (i, k)
            n += 1
    assert n > 0


def test_no_per_step_host_read_and_evaluation_is_logged(hip, tmp_path, monkeypatch):
    from pydreamer_amd import train as TR
    from pydreamer_amd.models import Dreamer

    def boom(self):
        raise AssertionError('packed_metrics_host() was called by the loop')

    reads = []
    real = TR.MetricAccumulator.read_and_reset
    monkeypatch.setattr(Dreamer, 'packed_metrics_host', boom)
    monkeypatch.setattr(TR.MetricAccumulator, 'read_and_reset', lambda self: (reads.append(1), real(self))[1])
    conf, logdir, logged = _run(tmp_path, None)
    assert len(reads) == 2
    assert [s for s, m in logged if 'train/steps' in m] == [3, 6]
    keys = {k for _, m in logged for k in m}
    for prefix in ('test/', 'eval/'):
        got = sorted(k for k in keys if k.startswith(prefix))
        print(prefix, got)
        assert f'{prefix}loss_model' in got and any(k.endswith('_open') for k in got), got
    assert all(s == 6 for s, m in logged if any(k.startswith(('test/', 'eval/')) for k in m))
    assert os.path.exists(os.path.join(logdir, 'checkpoints', 'latest.pt'))
    assert os.path.exists(os.path.join(logdir, 'd2_wm_closed', '0000001.npz'))      # step 1 is a logged batch (steps % 1000 == 1)
    assert any(n.startswith('0000006_r') for n in os.listdir(os.path.join(logdir, 'd2_wm_closed_test')))


# ------------------------------------------------------------------------------------------------ evaluate()
def _reference_evaluate(prefix, model, batches, eval_samples, keep_state, save_size, conf):
    """train.py:325-399 with its .item() calls (and init_state where no state is carried yet)."""
    from pydreamer_amd.train import prepare_batch_npz
    metrics_eval = defaultdict(list)
    state, tensors, npz_datas, do_output_tensors = None, None, [], True
    n_finished = np.zeros(1)
    for i_batch, obs in enumerate(batches):
        with torch.no_grad():
            T, B = obs['action'].shape[:2]
            reset_episodes = obs['reset'].any(dim=0)
            n_reset, n_continued = reset_episodes.sum().item(), (~reset_episodes).sum().item()
            n_finished = np.zeros(B) if i_batch == 0 else n_finished + reset_episodes.cpu().numpy()
            if n_reset > 0 and tensors is not None and 'loss_map' in tensors:
                last = (tensors['loss_map'].mean(dim=0) * reset_episodes).sum() / reset_episodes.sum()
                metrics_eval['logprob_map_last'].append(last.item())
            if n_continued > 0:
                st = state if state is not None else model.init_state(B * eval_samples)
                _, _, _, tensors_im, _ = model.training_step(obs, st, iwae_samples=eval_samples, imag_horizon=conf.imag_horizon,
                                                             do_open_loop=True, do_image_pred=True)
                mask = (~reset_episodes).float()
                for key, logprobs in tensors_im.items():
                    if key.startswith('logprob_'):
                        lps = logprobs[:5] * mask / mask
                        ok = ~torch.isnan(lps)
                        lp = (torch.where(ok, lps, torch.zeros_like(lps)).sum() / ok.sum()).item()
                        if not np.isnan(lp):
                            metrics_eval[f'{key}_open'].append(lp)
            if state is None or not keep_state:
                state = model.init_state(B * eval_samples)
            _, state, loss_metrics, tensors, _ = model.training_step(obs, state, iwae_samples=eval_samples,
                                                                    imag_horizon=conf.imag_horizon, do_image_pred=True)
            for k, v in loss_metrics.items():
                if not np.isnan(v.item()):
                    metrics_eval[k].append(v.item())
            if do_output_tensors:
                npz_datas.append(prepare_batch_npz({**obs, **tensors}, take_b=save_size))
            if n_finished[0] > 0:
                do_output_tensors = False
    metrics = {f'{prefix}/{k}': np.array(v).mean() for k, v in metrics_eval.items()}
    return metrics, {k: np.concatenate([d[k] for d in npz_datas], 1) for k in npz_datas[0]}


def _three_batches(obs):
    """All columns reset, then some, then none."""
    T, B = obs['reset'].shape
    out = []
    for which in ('all', 'some', 'none'):
        reset = torch.zeros(T, B, dtype=torch.bool, device=DEV)
        if which == 'all':
            reset[0] = True
        elif which == 'some':
            reset[0, 0] = True
            reset[T // 2, B - 1] = True
        b = {k: v.clone() for k, v in obs.items()}
        b['reset'] = reset
        if which != 'all':      # other rows, so that the three batches differ in more than the resets
            for k in b:
                if k != 'reset':
                    b[k] = torch.roll(b[k], 1 if which == 'some' else 2, dims=0).contiguous()
        out.append(b)
    return out


@pytest.mark.parametrize('which', ['cnn', 'minigrid'])
def test_evaluate_matches_the_loop_with_item_calls(hip, which):
    from pydreamer_amd.train import evaluate
    if which == 'cnn':
        from tests.test_gpu_act import _build
        oconf = O.tiny_conf()
        model = _build(config.load_config('defaults', 'atari', **vars(oconf)), params=O.make_params(oconf, seed=0))
        obs = {k: v.to(DEV) for k, v in O.preprocess(O.synthetic_batch(oconf), oconf).items()}
        samples = 2
    else:
        from tests.test_gpu_minigrid import _model, _obs
        g = np.load(os.path.join(GOLD, 'tiny_minigrid.npz'))
        oconf, model = _model(g)
        assert model.conf.probe_model == 'map'
        obs, _ = _obs(g, 's0_', oconf, model)
        samples = 1
    conf = model.conf
    batches = _three_batches(obs)
    torch.manual_seed(11)
    ref, ref_npz = _reference_evaluate('eval', model, batches, samples, True, 2, conf)
    torch.manual_seed(11)
    got, npz = evaluate('eval', 0, model, iter([dict(b) for b in batches]), len(batches), samples, True, 2, conf)
    print(sorted(got))
    assert set(got) == set(ref), set(got) ^ set(ref)
    assert any(k.endswith('_open') for k in got) and 'eval/loss_model' in got
    if which == 'minigrid':
        assert 'eval/logprob_map_last' in got and 'eval/loss_map' in got
    exact = 0
    for k in sorted(ref):
        a, b = float(got[k]), float(ref[k])
        exact += a == b
        print(f'{which} {k}: evaluate {a:.9g} loop {b:.9g}' + ('' if a == b else f'  rel {abs(a - b) / max(abs(b), 1e-12):.2e}'))
        assert a == b or abs(a - b) <= 1e-4 * abs(b) or abs(a - b) < 5e-6, (k, a, b)
    print(f'{which}: {exact} of {len(ref)} keys equal')
    assert list(npz) == list(ref_npz)
    for k in npz:
        assert npz[k].shape == ref_npz[k].shape and npz[k].dtype == ref_npz[k].dtype, k
        assert npz[k].shape[0] == 2, (k, npz[k].shape)
    # logged until column 0 has finished an episode: batch 0 opens, batch 1 resets column 0, batch 2 is not logged
    assert npz['reward'].shape == (2, 2 * obs['reset'].shape[0])
