"""The trainer loop (train.py:24-465 in one process): replay -> training_step -> backward -> clip -> step, with the
logging on the device - every scalar of a step is folded into running accumulators by one small launch (csrc/logging.hip) and
the host reads them ONCE per log interval - plus evaluation, the batch export, checkpoints in the reference's layout and, with
environments, collection between gradient steps.

  * `MetricAccumulator`                    - running sum / max / count per slot on the device; add() never waits;
  * `prepare_batch_npz`                    - train.py:423-465; float images leave the device as uint8 in the npz layout;
  * `evaluate`                             - train.py:306-408 with one host read of the scalars at the end;
  * `save_checkpoint` / `load_checkpoint`  - tools.py:164-197 on a local file;
  * `run`                                  - the loop; `python -m pydreamer_amd.train` runs its offline form.
Not here: mlflow, generator subprocesses, DataLoader workers, GradScaler (amp is bf16 operands with fp32 storage: no loss scaling),
the profiler hook, the 10 % random dump of open-loop batches (train.py:361-363)."""
import ctypes
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

from . import hip as H
from .models import GOALS_METRIC_SLOTS, KL_FREE_METRIC_SLOTS, METRIC_BUF_FLOATS, METRIC_SLOTS, RETURN_METRIC_SLOTS

RULE_IGNORE, RULE_NOT_NAN, RULE_FINITE_MAX, RULE_ALWAYS, RULE_MAX_ONLY = 0, 1, 2, 3, 4
MAX_SLOTS = 256
GRAD_NORMS = ('grad_norm', 'grad_norm_probe', 'grad_norm_actor', 'grad_norm_critic')
# the four data statistics (train.py:211-214), in dm_batch_stats' order, behind the metric buffer's slots
STATS_BASE = METRIC_BUF_FLOATS
DATA_STATS = {'data_reward': [(STATS_BASE, RULE_ALWAYS), (STATS_BASE + 3, RULE_MAX_ONLY)],
              'data_reset': (STATS_BASE + 1, RULE_ALWAYS), 'data_terminal': (STATS_BASE + 2, RULE_ALWAYS)}


# ------------------------------------------------------------------------------------------------ kernel wrappers
def rules_tensor(rules, device):
    """The device bytes dm_metric_accum reads, from a host sequence of rules 0 ... 4.  The kernel cannot report a bad rule, so
    this is where one is refused."""
    rules = [int(r) for r in rules]
    bad = [r for r in rules if not 0 <= r <= 4]
    if bad:
        raise ValueError(f'metric rules {bad}: expected 0 (ignore), 1 (not NaN), 2 (finite, with max), 3 (always), 4 (max only)')
    if not 1 <= len(rules) <= MAX_SLOTS:
        raise ValueError(f'{len(rules)} metric slots (1 ... {MAX_SLOTS})')
    return torch.tensor(rules, dtype=torch.uint8).to(device)


def _at(t, offset):
    """Device pointer of element `offset` of a contiguous tensor."""
    return ctypes.c_void_p(t.data_ptr() + offset * t.element_size())


def _f32(t, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise H.DreamerHipError(f'{what}: expected a contiguous float32 device tensor, got '
                                f'{(t.dtype, t.device, t.is_contiguous()) if torch.is_tensor(t) else type(t)}')
    return t


def _bytes(t, what):
    """bool / uint8 device tensor as bytes (NULL for None)."""
    if t is None:
        return None
    if not (t.is_cuda and t.dtype in (torch.bool, torch.uint8) and t.is_contiguous()):
        raise H.DreamerHipError(f'{what}: expected a contiguous bool device tensor, got {t.dtype} on {t.device}')
    return t


def batch_stats(reward, reset, terminal=None, out=None):
    """dm_batch_stats on (T,B) device tensors: out (4 floats) = [mean reward, mean reset, mean terminal, max reward]."""
    reward = _f32(reward, 'reward')
    reset = _bytes(reset, 'reset')
    n = reward.numel()
    if reset.numel() != n or (terminal is not None and _f32(terminal, 'terminal').numel() != n):
        raise H.DreamerHipError(f'batch_stats: reward has {n} elements, reset {reset.numel()}, terminal '
                                f'{None if terminal is None else terminal.numel()}')
    if out is None:
        out = torch.empty(4, device=reward.device)
    H.call('dm_batch_stats', n, H.fptr(reward), H.ptr(reset), H.fptr(terminal), H.fptr(out), H.stream())
    return out


def masked_mean(x, take_rows, col_keep=None, skip_nan=True, out=None):
    """dm_masked_mean on a (T,B) float32 device tensor (a row-sliced view of a wider one is taken as it lies); col_keep: (B,)
    bool device tensor or None; returns the one-float device tensor `out`."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise H.DreamerHipError('masked_mean: expected a (T,B) float32 device tensor with unit column stride')
    T, B = x.shape
    ldx = x.stride(0) if T > 1 else max(x.stride(0), B)
    col_keep = _bytes(col_keep, 'col_keep')
    if col_keep is not None and col_keep.numel() != B:
        raise H.DreamerHipError(f'masked_mean: col_keep has {col_keep.numel()} elements for {B} columns')
    if out is None:
        out = torch.empty(1, device=x.device)
    H.call('dm_masked_mean', T, B, ctypes.c_void_p(x.data_ptr()), ldx, int(take_rows), H.ptr(col_keep), int(bool(skip_nan)),
           ctypes.c_void_p(out.data_ptr()), H.stream())
    return out


def export_image_u8(x, take_b=999):
    """dm_export_image_u8: (T,B,C,H,W) float32 device tensor -> (min(take_b,B),T,H,W,C) uint8 device tensor."""
    x = _f32(x, 'image')
    if x.dim() != 5:
        raise H.DreamerHipError(f'export_image_u8: expected (T,B,C,H,W), got {tuple(x.shape)}')
    T, B, C, Hh, W = x.shape
    out = torch.empty(min(max(int(take_b), 0), B), T, Hh, W, C, dtype=torch.uint8, device=x.device)
    H.call('dm_export_image_u8', T, B, int(take_b), C, Hh, W, H.fptr(x), H.ptr(out), H.stream())
    return out


# ------------------------------------------------------------------------------------------------ accumulators
def default_slots(model):
    """{name: (index, rule)} for a model's metric buffer (Dreamer or WorldModelProbe): packed_metrics()'s names under rule 1 (counted unless NaN,
    train.py:204-206), the gradient norms under rule 2 (counted when finite, with their max, train.py:207-210), and the four
    data statistics behind the buffer (train.py:211-214)."""
    table = dict(METRIC_SLOTS)      # packed_metrics()'s table, which a model has only once a step has run
    if 'goals' in getattr(model.conf, 'probe_model', 'none'):
        table.update(GOALS_METRIC_SLOTS)
    if getattr(model.conf, 'return_norm', 'none') == 'percentile':
        table.update(RETURN_METRIC_SLOTS)
    if getattr(model.conf, 'kl_free', 0.0) > 0:
        table.update(KL_FREE_METRIC_SLOTS)
    slots = {k: (i, RULE_FINITE_MAX if k in GRAD_NORMS else RULE_NOT_NAN) for k, i in table.items()}
    slots.update(DATA_STATS)
    return slots


class MetricAccumulator:
    """Running sum (fp64), max (fp64) and count (int64) per slot, on the device.  `slots`: {name: (index, rule)} - or a list of
    such pairs for a name that owns two slots, as data_reward does (its mean and its max); the rules are dm_metric_accum's.
    add() and add_batch_stats() enqueue one or two small launches on the current stream and never wait; read_and_reset() makes
    ONE device-to-host copy of all accumulators and refills them asynchronously."""

    def __init__(self, slots, device):
        self.device = torch.device(device)
        self.entries = []      # (name, index, rule)
        for name, v in slots.items():
            for index, rule in (v if isinstance(v, list) else [v]):
                self.entries.append((name, int(index), int(rule)))
        idx = [e[1] for e in self.entries]
        if not idx or min(idx) < 0 or len(set(idx)) != len(idx):
            raise ValueError(f'metric slots must be distinct indices >= 0, got {sorted(idx)}')
        self.n = n = max(idx) + 1
        rules = [RULE_IGNORE] * n
        for _, i, r in self.entries:
            rules[i] = r
        self.rules = rules_tensor(rules, self.device)      # refuses n > 256 and rules above 4
        fresh = torch.zeros(3 * n, dtype=torch.float64)     # sum | max | count (the bits of int64 0 are those of 0.0)
        fresh[n:2 * n] = -np.inf
        self._fresh = fresh.to(self.device)
        self.acc = self._fresh.clone()
        self._stats = torch.zeros(4, device=self.device)
        self.reads = 0

    def _fold(self, vals, offset):
        m, n = vals.numel(), self.n
        if offset < 0 or offset + m > n:
            raise ValueError(f'{m} values at slot {offset}: the accumulator has {n} slots')
        H.call('dm_metric_accum', m, H.fptr(vals), _at(self.rules, offset), _at(self.acc, offset), _at(self.acc, n + offset),
               _at(self.acc, 2 * n + offset), H.stream())

    def add(self, buffer, offset=0):
        """Folds buffer[i] into slot offset + i for every i the accumulator has a slot for.  The caller orders the stream behind
        whoever wrote the buffer (Dreamer.join_optimizers() for the pipelined gradient norms)."""
        buffer = _f32(buffer, 'metric buffer').view(-1)
        self._fold(buffer[:max(0, self.n - offset)], offset)

    def add_batch_stats(self, obs, base=STATS_BASE):
        """The batch's four data statistics (dm_batch_stats) into slots base ... base + 3."""
        batch_stats(obs['reward'], obs['reset'], obs.get('terminal'), out=self._stats)
        self._fold(self._stats, base)

    def read(self):
        """(sum, max, count) as numpy arrays: the ONE device-to-host copy."""
        host = self.acc.cpu()
        self.reads += 1
        n = self.n
        return host[:n].numpy(), host[n:2 * n].numpy(), host[2 * n:].view(torch.int64).numpy()

    def reset(self):
        self.acc.copy_(self._fresh)      # device to device, asynchronous

    def read_and_reset(self):
        """{name: sum / count} in float64 and {name + '_max': max} for the rules that track one; a name nothing was counted
        for is left out, as the reference's dict has a key only once something was appended."""
        s, m, c = self.read()
        self.reset()
        out = {}
        for name, i, rule in self.entries:
            if rule in (RULE_NOT_NAN, RULE_FINITE_MAX, RULE_ALWAYS) and c[i] > 0:
                out[name] = float(s[i]) / float(c[i])
        for name, i, rule in self.entries:
            if (rule == RULE_FINITE_MAX and c[i] > 0) or (rule == RULE_MAX_ONLY and m[i] != -np.inf):
                out[name + '_max'] = float(m[i])
        return out


# ------------------------------------------------------------------------------------------------ batch export
def _softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def prepare_batch_npz(data, take_b=999):
    """train.py:423-465: {key: (T,B,...) tensor} -> {key: (B',T,...) numpy array}, B' = min(take_b, B).  A float32 device tensor
    (T,B,C,W,W) with C in {1, 3} becomes uint8 (B',T,W,W,C) on the device (dm_export_image_u8) and crosses at one byte per
    pixel.  Everything else follows the reference's rule on the host, sliced to take_b BEFORE the copy: rank 2-4 as they are;
    rank 5 channels-last, then uint8 for 1 or 3 channels, argmax for a one-hot, softmax for categorical logits.  A uint8 rank-5
    tensor (the replay's own frames) is in its npz form already and is only transposed to (B',T,...)."""
    out = {}
    for key, val in data.items():
        if not torch.is_tensor(val):
            val = torch.as_tensor(np.asarray(val))
        val = val.detach()
        if val.dim() == 5 and val.dtype != torch.uint8:
            assert val.dtype in (torch.float16, torch.float32, torch.float64) and (key.startswith('image') or key.startswith('map')), \
                f'Unexpected 3D tensor: {key}: {tuple(val.shape)}, {val.dtype}'
        if (val.is_cuda and val.dim() == 5 and val.dtype == torch.float32 and val.shape[-1] == val.shape[-2]
                and val.shape[2] in (1, 3)):
            out[key] = export_image_u8(val.contiguous(), take_b).cpu().numpy()
            continue
        if take_b < val.shape[1]:
            val = val[:, :take_b]
        x = val.cpu().numpy()      # (T,B,*)
        if x.dtype in (np.float16, np.float64):
            x = x.astype(np.float32)
        if x.ndim == 5 and x.dtype != np.uint8:
            if x.shape[-1] == x.shape[-2]:      # (T,B,C,W,W) => (T,B,W,W,C)
                x = x.transpose(0, 1, 3, 4, 2)
            assert x.shape[-2] == x.shape[-3], 'Assuming rectangular images, otherwise need to improve logic'
            if x.shape[-1] in (1, 3):      # RGB or grayscale
                x = ((x + 0.5) * 255.0).clip(0, 255).astype('uint8')
            elif np.allclose(x.sum(axis=-1), 1.0) and np.allclose(x.max(axis=-1), 1.0):      # one-hot
                x = x.argmax(axis=-1)
            else:      # categorical logits
                assert key in ('map_rec', 'image_rec', 'image_pred'), f'Unexpected 3D categorical logits: {key}: {x.shape}'
                x = _softmax(x)
        out[key] = x.swapaxes(0, 1)      # (T,B,*) => (B,T,*)
    return out


def save_npz(data, path):
    """np.savez_compressed to a temporary name, then renamed into place."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f'{path}.tmp{os.getpid()}'
    with open(tmp, 'wb') as f:
        np.savez_compressed(f, **data)
    os.replace(tmp, path)
    return path


# ------------------------------------------------------------------------------------------------ checkpoints
def save_checkpoint(path, model, optimizers, steps, explore=None, explore_optimizers=()):
    """The dict of tools.py:164-175 - epoch, model_state_dict, optimizer_{i}_state_dict - written with torch.save to a temporary
    name and renamed into place.  explore (a Plan2Explore): explore_state_dict and explore_optimizer_{i}_state_dict beside them."""
    checkpoint = {'epoch': int(steps), 'model_state_dict': model.state_dict()}
    for i, opt in enumerate(optimizers):
        checkpoint[f'optimizer_{i}_state_dict'] = opt.state_dict()
    if explore is not None:
        checkpoint['explore_state_dict'] = explore.state_dict()
        for i, opt in enumerate(explore_optimizers):
            checkpoint[f'explore_optimizer_{i}_state_dict'] = opt.state_dict()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f'{path}.tmp{os.getpid()}'
    torch.save(checkpoint, tmp)
    os.replace(tmp, path)
    return path


def load_checkpoint(path, model, optimizers=(), map_location=None, explore=None, explore_optimizers=()):
    """tools.py:177-197: loads model and optimizers, returns the checkpoint's epoch; None when the file is absent.  explore (a
    Plan2Explore) and its optimizers are loaded from the explore_ keys when the file has them: a checkpoint written without
    Plan2Explore leaves them as they are."""
    if not os.path.exists(path):
        return None
    checkpoint = torch.load(path, map_location=map_location)
    model.load_state_dict(checkpoint['model_state_dict'])
    for i, opt in enumerate(optimizers):
        opt.load_state_dict(checkpoint[f'optimizer_{i}_state_dict'])
    if explore is not None and 'explore_state_dict' in checkpoint:
        explore.load_state_dict(checkpoint['explore_state_dict'])
        for i, opt in enumerate(explore_optimizers):
            opt.load_state_dict(checkpoint[f'explore_optimizer_{i}_state_dict'])
    return checkpoint['epoch']


# ------------------------------------------------------------------------------------------------ evaluation
# slots for the scalars of an evaluation batch: the step's metrics, then the *_open means.  A categorical reward decoder adds one
# logprob_reward{i} and one logprob_reward{i}_open per support value, up to 2 x 32 names on top of the ~35 of a Normal head
_EVAL_EXTRA = 160


def _to_device(batch, device):
    return {k: (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(device) for k, v in batch.items()}


def evaluate(prefix, steps, model, data_iterator, eval_batches, eval_samples, keep_state, save_size, conf):
    """train.py:306-408.  Returns (metrics, npz_data): {f'{prefix}/{key}': mean over the batches where the key was not NaN} and
    the concatenated npz batches of the first `save_size` columns (None without batches), kept until column 0 has finished an
    episode.  Per batch: logprob_map_last from the previous batch's loss_map over the columns that reset, the open-loop pass over
    the continued columns with logprob_*_open over the first five rows, the closed-loop pass with carried state.
    Different from the reference: every scalar goes through a MetricAccumulator and is read once at the end - the only host
    wait per batch is the (B,) copy of reset.any(0) that steers the control flow; a column that continues while no state is
    carried yet starts from init_state(B * eval_samples), where the reference would pass None and fail; the 10 % random dump of
    open-loop batches is not built."""
    device = next(model.parameters()).device
    slots = {'logprob_map_last': (0, RULE_ALWAYS)}
    slots.update({f'_{i}': (1 + i, RULE_NOT_NAN) for i in range(_EVAL_EXTRA)})
    acc = MetricAccumulator(slots, device)
    names = {}      # metric name -> slot 1 + i, in order of first appearance
    nan = torch.full((), float('nan'), device=device)
    one = torch.empty(1, device=device)
    state, tensors, npz_datas = None, None, []
    n_finished = np.zeros(1)
    do_output_tensors = True

    def slot(name):
        if name not in names:
            if len(names) >= _EVAL_EXTRA:
                raise ValueError(f'evaluate: more than {_EVAL_EXTRA} distinct metrics')
            names[name] = len(names)
        return names[name]

    for i_batch in range(eval_batches):
        with torch.no_grad():
            batch = next(data_iterator)
            obs = _to_device(batch, device)
            T, B = obs['action'].shape[:2]
            reset_episodes = obs['reset'].any(dim=0)      # (B,)
            reset_host = reset_episodes.cpu().numpy()     # the batch's one host wait: it steers what runs below
            n_reset, n_continued = int(reset_host.sum()), int((~reset_host).sum())
            n_finished = np.zeros(B) if i_batch == 0 else n_finished + reset_host
            scalars = {}      # slot -> 0-dim device tensor

            # _last predictions from the last batch of the previous episode
            if n_reset > 0 and tensors is not None and 'loss_map' in tensors:
                masked_mean(tensors['loss_map'].contiguous(), T, reset_episodes, skip_nan=False, out=one)
                acc.add(one, 0)

            # open loop & unseen logprob
            if n_continued > 0:
                st = state if state is not None else model.init_state(B * eval_samples)
                _, _, _, tensors_im, _ = model.training_step(obs, st, iwae_samples=eval_samples, imag_horizon=conf.imag_horizon,
                                                             do_open_loop=True, do_image_pred=True)
                keep = ~reset_episodes
                for key, logprobs in tensors_im.items():
                    if key.startswith('logprob_'):      # many are NaN - the mean of those that exist, over the first five rows
                        lp = logprobs.float().contiguous()
                        scalars[slot(f'{key}_open')] = masked_mean(lp.view(lp.shape[0], -1), 5, keep, skip_nan=True).view(())

            # closed loop & loss
            if state is None or not keep_state:
                state = model.init_state(B * eval_samples)
            _, state, loss_metrics, tensors, _ = model.training_step(obs, state, iwae_samples=eval_samples,
                                                                    imag_horizon=conf.imag_horizon, do_image_pred=True)
            for k, v in loss_metrics.items():
                scalars[slot(k)] = torch.as_tensor(v, device=device).detach().float().reshape(())
            acc.add(torch.stack([scalars.get(i, nan) for i in range(len(names))]), 1)

            # one episode batch
            if do_output_tensors:
                npz_datas.append(prepare_batch_npz({**batch, **tensors}, take_b=save_size))
            if n_finished[0] > 0:      # predictions are logged until the first episode has finished
                do_output_tensors = False

    s, _, c = acc.read()
    if hasattr(model, 'check_device_status'):
        model.check_device_status()
    metrics = {}
    if c[0] > 0:
        metrics[f'{prefix}/logprob_map_last'] = float(s[0]) / float(c[0])
    for name, i in names.items():
        if c[1 + i] > 0:
            metrics[f'{prefix}/{name}'] = float(s[1 + i]) / float(c[1 + i])
    npz_data = {k: np.concatenate([d[k] for d in npz_datas], 1) for k in npz_datas[0]} if npz_datas else None
    return metrics, npz_data


# ------------------------------------------------------------------------------------------------ the loop
class JsonlLogger:
    """The default logger: one JSON line per call in logdir/metrics.jsonl."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        self.path = os.path.join(logdir, 'metrics.jsonl')

    def __call__(self, metrics, step):
        with open(self.path, 'a') as f:
            f.write(json.dumps({'_step': int(step), **{k: float(v) for k, v in metrics.items()}}) + '\n')


def _build_model(conf):
    model = getattr(conf, 'model', 'dreamer')
    if model == 'dreamer':
        from .models import Dreamer
        return Dreamer(conf)
    if model == 'gru_probe':
        from .baselines import WorldModelProbe
        return WorldModelProbe(conf)
    raise ValueError(f'model={model!r}: the trainer loop builds dreamer and gru_probe')


def _feed(conf, repository, batch_size, device, has_goals, **replay_kw):
    from .replay import DeviceReplay, SequentialReplay
    probe = getattr(conf, 'probe_model', 'none')
    return DeviceReplay(SequentialReplay(repository, conf.batch_length, batch_size, **replay_kw), conf.action_dim, device,
                        clip_rewards=conf.clip_rewards, image_key=conf.image_key,
                        map_key=conf.map_key if 'map' in probe else None,
                        map_categorical=conf.map_channels if ('map' in probe and conf.map_categorical) else None,
                        goals=has_goals, image_categorical=conf.image_channels if conf.image_categorical else None)


def run(conf, train_repository, eval_repository=None, test_repository=None, envs=None, policy_kwargs=None, logdir=None, logger=None,
        env_steps_per_grad_step=None, on_step=None, seed=0, steps_per_npz=1000, agent_log_every=10, eval_envs=None,
        eval_episodes=None, eval_policy_kwargs=None, split_fraction=0.0):
    """train.py:24-303 in one process.  Data: DeviceReplay(SequentialReplay(train_repository, ...)) with the reference's reader
    arguments; model: Dreamer, or WorldModelProbe for conf.model = 'gru_probe'; logdir/checkpoints/latest.pt is resumed if
    present.  Per step: training_step, prefetch of the next batch, zero_grad, backward, grad_clip, step, then two accumulate
    calls; every log_interval steps ONE host read of the accumulators (the loop's only host wait), check_device_status(),
    train/steps and train/fps, and logger(metrics, step) - by default JSON lines in logdir/metrics.jsonl.  Logged batches go to
    logdir/d2_wm_closed and d2_wm_dream, checkpoints are written every save_interval, evaluate('test') and evaluate('eval')
    run every eval_interval (on test_repository / eval_repository; each defaults to the other, and without either nothing is
    evaluated).  Stops at n_steps, or when the listed steps reach n_env_steps.
    Online (envs given): prefill with RandomPolicy until generator_prefill_steps steps are listed; after each gradient step
    collect with NetworkPolicy(model, ..., per_env=True, **policy_kwargs) until the environment steps recorded since the prefill
    reach grad steps x ratio - env_steps_per_grad_step, or conf.limit_step_ratio when > 0: the reference's rate limit
    (generator.py:118) as a schedule; the recorder writes a file once steps_per_npz steps of closed episodes are queued, and after
    every collection round.
    Agent metrics (online, agent_log_every > 0): the training recorder feeds a collect.EpisodeStats('agent') through its
    on_episode hook; after every collection round, prefill included, logger(stats.pop(), steps) once agent_log_every returns are
    held - a logger call of its own, every key agent/..., host numbers only: no device read, no accumulator call.
    Evaluation episodes (eval_envs; needs eval_repository): at every eval_interval step, before the two evaluate() calls, a second
    Collector with its own NetworkPolicy(model, ..., batch_size=len(eval_envs), per_env=True, **eval_policy_kwargs) runs
    run_episodes(eval_episodes or len(eval_envs)) into eval_repository and is closed (open episodes are dropped, the next round
    resets the environments); one agent_eval/... entry over the round's episodes is logged, and evaluate('eval') reads what was
    just written.  The default policy samples, as the reference's evaluation generators do; dict(mode='mode') is greedy.  This
    draws from the device's random stream, which is why it is opt-in.
    split_fraction > 0: the training recorder writes that fraction of its files to test_repository (generator.py:244).
    on_step(step, model, obs, tensors): a hook behind the optimizer step (tests); None costs nothing.  Returns the step count.
    conf.expl_behavior = 'plan2explore' ('greedy' runs none of this): an explore.Plan2Explore beside the model - its
    training_step behind the model's, its backward, clip and AdamW behind the model's optimizer step; its scalars go through a
    second MetricAccumulator and are logged as train/expl_*; the checkpoint holds explore_state_dict and
    explore_optimizer_{i}_state_dict.  Online, the training collector's NetworkPolicy acts with the exploration actor-critic while
    conf.expl_until == 0 or the collector has taken fewer than expl_until environment steps (prefill included), then with the task
    one, on the same carried state.  Evaluation always uses the task policy.  on_step may take a fifth argument, the Plan2Explore.
    conf.eval_behavior = 'plan' ('actor' is the text above): the evaluation Collector acts with planner.PlannerPolicy -
    CEM in latent space at the conf.plan_* sizes, eval_policy_kwargs going to CEMPlanner - and logs the same agent_eval/* keys."""
    from .collect import Collector, EpisodeRecorder, EpisodeStats
    from .policy import NetworkPolicy, RandomPolicy, StepPreprocessor
    model_name = getattr(conf, 'model', 'dreamer')
    if model_name not in ('dreamer', 'gru_probe'):
        raise ValueError(f'model={model_name!r}: the trainer loop builds dreamer and gru_probe')
    online = envs is not None
    ratio = None
    if online:
        ratio = env_steps_per_grad_step if env_steps_per_grad_step else (conf.limit_step_ratio if conf.limit_step_ratio > 0 else None)
        if not ratio:
            raise ValueError('online training needs env_steps_per_grad_step, or conf.limit_step_ratio > 0')
    if eval_envs is not None and eval_repository is None:
        raise ValueError('eval_envs needs an eval_repository to write the evaluation episodes to')
    if split_fraction > 0 and test_repository is None:
        raise ValueError(f'split_fraction={split_fraction} needs a test_repository')
    if split_fraction > 0 and not online:
        raise ValueError(f'split_fraction={split_fraction} without envs: nothing is recorded offline')
    expl_behavior = getattr(conf, 'expl_behavior', 'greedy')
    if expl_behavior not in ('greedy', 'plan2explore'):
        raise ValueError(f'expl_behavior={expl_behavior!r}: the trainer loop builds greedy and plan2explore')
    explore = expl_behavior == 'plan2explore'
    if explore and model_name != 'dreamer':
        raise ValueError(f"expl_behavior='plan2explore' needs model='dreamer', got {model_name!r}")
    eval_behavior = getattr(conf, 'eval_behavior', 'actor')
    if eval_behavior not in ('actor', 'plan'):
        raise ValueError(f'eval_behavior={eval_behavior!r}: the evaluation episodes act with the actor or by planning (plan)')
    if eval_behavior == 'plan' and model_name != 'dreamer':
        raise ValueError(f"eval_behavior='plan' needs model='dreamer', got {model_name!r}")
    if logdir is None:
        raise ValueError('run() needs a logdir: checkpoints, logged batches and the default logger write there')
    if eval_behavior == 'plan':      # (the default never imports the module)
        from .planner import PlannerPolicy
    if explore:      # (a greedy run never imports the module)
        from .explore import EXPLORE_GRAD_NORMS, EXPLORE_METRIC_SLOTS, Plan2Explore, log_name
    device = torch.device(conf.device)
    torch.manual_seed(seed)
    logger = logger or JsonlLogger(logdir)
    ckpt = os.path.join(logdir, 'checkpoints', 'latest.pt')

    model = _build_model(conf).to(device)
    optimizers = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    p2e, p2e_optimizers, ckpt_kw = None, (), {}
    if explore:
        p2e = Plan2Explore(conf, model).to(device)
        p2e_optimizers = p2e.init_optimizers()
        ckpt_kw = dict(explore=p2e, explore_optimizers=p2e_optimizers)
    steps = load_checkpoint(ckpt, model, optimizers, map_location=device, **ckpt_kw) or 0
    has_goals = 'goals' in getattr(conf, 'probe_model', 'none')
    image_cat = conf.image_channels if conf.image_categorical else None

    def attach_stats(prefix, log_every, col):
        """An EpisodeStats fed by the on_episode hook of the collector's recorder, with the counters of both."""
        stats, rec = EpisodeStats(prefix, action_repeat=conf.env_action_repeat, log_every=log_every), col.recorder
        rec.on_episode = lambda data: stats.add_episode(data, col.steps, rec.steps_saved, rec.episodes + 1, col.seconds())
        return stats

    def log_agent():
        if stats is not None and stats.ready():
            logger(stats.pop(), steps)

    prep = StepPreprocessor(conf.action_dim, clip_rewards=conf.clip_rewards, image_key=conf.image_key,
                            image_categorical=image_cat, batched=True)
    eval_collector = None
    if eval_envs is not None:
        # eval_behavior='plan' (DESIGN 4.19): the same episodes, columns and agent_eval/* keys with the CEM planner acting; the
        # sizes are conf.plan_*, eval_policy_kwargs are then CEMPlanner's
        eval_policy = PlannerPolicy if eval_behavior == 'plan' else NetworkPolicy
        eval_collector = Collector(eval_envs, eval_policy(model, prep, batch_size=len(eval_envs), device=device, per_env=True,
                                                          **(eval_policy_kwargs or {})),
                                   EpisodeRecorder(eval_repository, len(eval_envs), steps_per_npz=steps_per_npz))
        eval_stats = attach_stats('agent_eval', 0, eval_collector)

    # prefill
    collector, stats = None, None
    if online:
        B_env = len(envs)
        split = {}
        if split_fraction > 0:
            split = dict(repository2=test_repository, split_fraction=split_fraction, rng=np.random.RandomState(seed))
        recorder = EpisodeRecorder(train_repository, B_env, steps_per_npz=steps_per_npz, **split)
        collector = Collector(envs, RandomPolicy(conf.action_dim, B_env, seed=seed, continuous=conf.actor_dist != 'onehot'), recorder)
        if agent_log_every:
            stats = attach_stats('agent', agent_log_every, collector)
        while train_repository.count_steps()[1] < conf.generator_prefill_steps:
            collector.run(max(1, -(-(conf.generator_prefill_steps - train_repository.count_steps()[1]) // B_env)))
            collector.flush()
            log_agent()
        collector.policy = NetworkPolicy(model, prep, batch_size=B_env, device=device, per_env=True, **(policy_kwargs or {}))
        if p2e is not None:
            collector.policy.ac = p2e.ac
        recorded0 = recorder.steps_saved + recorder.queued_steps
        if train_repository.count_steps()[1] * conf.env_action_repeat >= conf.n_env_steps:
            return steps      # a prefill-only job, or a finished one resumed

    data = _feed(conf, train_repository, conf.batch_size, device, has_goals, skip_first=True, reload_interval=120 if online else 0,
                 buffer_size=conf.buffer_size if online else conf.buffer_size_offline, reset_interval=conf.reset_interval,
                 allow_mid_reset=conf.allow_mid_reset, seed=seed)
    acc = MetricAccumulator(default_slots(model), device)
    acc_expl = None
    if p2e is not None:      # the exploration step's own buffer, its own accumulator: default_slots(model) is what it always was
        acc_expl = MetricAccumulator({log_name(k): (i, RULE_FINITE_MAX if k in EXPLORE_GRAD_NORMS else RULE_NOT_NAN)
                                      for k, i in EXPLORE_METRIC_SLOTS.items()}, device)
    join = getattr(model, 'join_optimizers', None)
    state = None
    grad_steps, last_time, last_steps = 0, time.time(), steps
    try:
        while True:
            steps += 1
            grad_steps += 1
            will_log_batch = steps % conf.logbatch_interval == 1
            will_image_pred = will_log_batch or steps % conf.log_interval >= int(conf.log_interval * 0.9)      # 10 % of batches
            obs = data.next()
            if state is None:
                state = model.init_state(conf.batch_size * conf.iwae_samples)
            losses, new_state, _, tensors, dream_tensors = model.training_step(obs, state, do_image_pred=will_image_pred,
                                                                               do_dream_tensors=will_log_batch)
            data.prefetch()
            state = new_state if conf.keep_state else None
            if p2e is not None:      # on the weights and features the model's own step has just used
                expl_losses, _ = p2e.training_step()
            for opt in optimizers:
                opt.zero_grad()
            for loss in losses:
                loss.backward()
            model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
            for opt in optimizers:
                opt.step()
            if p2e is not None:
                for opt in p2e_optimizers:
                    opt.zero_grad()
                for loss in expl_losses:
                    loss.backward()
                p2e.grad_clip(conf.grad_clip, conf.grad_clip_ac)
                for opt in p2e_optimizers:
                    opt.step()
            if on_step is not None:
                on_step(steps, model, obs, tensors, *(() if p2e is None else (p2e,)))
            # the step's scalars: folded on the device behind a stream-side wait for the pipelined gradient norms
            if join is not None:
                join()
            acc.add(model.metric_buffer)
            acc.add_batch_stats(obs)
            if acc_expl is not None:
                acc_expl.add(p2e.metric_buffer)

            if will_log_batch:
                save_npz(prepare_batch_npz({**obs, **tensors}), os.path.join(logdir, 'd2_wm_closed', f'{steps:07}.npz'))
            if dream_tensors:
                save_npz(prepare_batch_npz({**obs, **dream_tensors}), os.path.join(logdir, 'd2_wm_dream', f'{steps:07}.npz'))

            if online and steps % conf.logbatch_interval == 0:
                listed = train_repository.count_steps()[1]
                if listed * conf.env_action_repeat >= conf.n_env_steps:
                    break

            if steps % conf.log_interval == 0:
                metrics = {f'train/{k}': v for k, v in acc.read_and_reset().items()}      # the loop's only host wait
                if acc_expl is not None:
                    metrics.update({f'train/{k}': v for k, v in acc_expl.read_and_reset().items()})
                if hasattr(model, 'check_device_status'):
                    model.check_device_status()
                t = time.time()
                metrics['train/steps'] = steps
                metrics['train/fps'] = (steps - last_steps) / max(t - last_time, 1e-9)
                last_time, last_steps = t, steps
                logger(metrics, steps)

            if steps % conf.save_interval == 0:
                save_checkpoint(ckpt, model, optimizers, steps, **ckpt_kw)

            # (the reference returns at n_steps before it evaluates; here a run whose last step is an evaluation step evaluates)
            if conf.eval_interval and steps % conf.eval_interval == 0:
                if eval_collector is not None:
                    eval_collector.run_episodes(eval_episodes or len(eval_envs))
                    eval_collector.close()
                    agent_eval = eval_stats.pop()
                    if agent_eval:
                        logger(agent_eval, steps)
                _evaluate_both(conf, model, steps, test_repository, eval_repository, device, has_goals, logdir, logger, seed)
            if steps >= conf.n_steps:
                break

            if online:
                while (collector.recorder.steps_saved + collector.recorder.queued_steps - recorded0) < grad_steps * ratio:
                    if p2e is not None and conf.expl_until > 0 and collector.steps >= conf.expl_until:
                        collector.policy.ac = None      # from here on the task policy collects, on the same carried state
                    collector.run(1)
                collector.flush()
                log_agent()
    finally:
        data.close()
        if collector is not None:
            collector.close()
    return steps


def _evaluate_both(conf, model, steps, test_repository, eval_repository, device, has_goals, logdir, logger, seed):
    """train.py:275-289: test = the training settings, eval = no state reset and multisampling; a failure only warns (there may
    be no evaluation data yet)."""
    test_repository, eval_repository = test_repository or eval_repository, eval_repository or test_repository
    if test_repository is None:
        return
    try:
        for prefix, repo, bsz, kw, args in (
                ('test', test_repository, conf.test_batch_size, dict(skip_first=False, reset_interval=conf.reset_interval),
                 (conf.test_batches, conf.iwae_samples, conf.keep_state, conf.test_save_size)),
                ('eval', eval_repository, conf.eval_batch_size, dict(skip_first=False),
                 (conf.eval_batches, conf.eval_samples, True, conf.eval_save_size))):
            feed = _feed(conf, repo, bsz, device, has_goals, seed=seed, **kw)
            try:
                metrics, npz_data = evaluate(prefix, steps, model, feed, *args, conf)
            finally:
                feed.close()
            logger(metrics, steps)
            if npz_data is not None:
                r = float(npz_data['reward'][0].sum())
                save_npz(npz_data, os.path.join(logdir, f'd2_wm_closed_{prefix}', f'{steps:07}_r{r:.0f}.npz'))
    except Exception as e:
        warnings.warn(f'Evaluation failed: {e!r}')


def main(argv=None):
    """python -m pydreamer_amd.train --configs defaults atari --offline_data_dir DIR --logdir DIR [key=value ...]"""
    import argparse
    import ast
    from . import config
    from .replay import LocalEpisodeRepository
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument('--configs', nargs='+', default=['defaults'])
    ap.add_argument('--offline_data_dir', required=True, nargs='+')
    ap.add_argument('--offline_test_dir', nargs='+')
    ap.add_argument('--offline_eval_dir', nargs='+')
    ap.add_argument('--logdir', required=True)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('overrides', nargs='*', help='key=value')
    args = ap.parse_args(argv)
    over = {}
    for item in args.overrides:
        k, _, v = item.partition('=')
        try:
            over[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            over[k] = v
    conf = config.load_config(*args.configs, **over)
    repo = lambda d: LocalEpisodeRepository(d) if d else None
    steps = run(conf, repo(args.offline_data_dir), eval_repository=repo(args.offline_eval_dir),
                test_repository=repo(args.offline_test_dir), logdir=args.logdir, seed=args.seed)
    print(f'finished at step {steps}')


if __name__ == '__main__':
    main(sys.argv[1:])
