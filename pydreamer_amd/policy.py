"""The acting process's policy object (generator.py:311-331) on Dreamer.act: preprocess -> one device call -> ONE device-to-host
copy per environment step.  batch_size = 1 is the reference's generator; batch_size = N drives N environments as one batch."""
import numpy as np
import torch

from .replay import preprocess_batch

METRIC_KEYS = ('policy_value', 'action_prob', 'policy_entropy')
_LOGGED_BY_ACTOR = METRIC_KEYS      # preprocessing.py:100: what an earlier policy call logged is not an observation


class StepPreprocessor:
    """Preprocessor.apply(obs, expandTB=True) (preprocessing.py:91-180) for one environment step, over replay.preprocess_batch:
    the environment's observation dict -> numpy (1, B, ...) fields.  batched=False: `obs` holds one environment's fields, (*) =>
    (1, 1, *); batched=True: every field carries a leading environment axis, (B, *) => (1, B, *).  The other arguments are
    preprocess_batch's."""

    def __init__(self, action_dim, clip_rewards=None, image_key='image', image_categorical=None, batched=False):
        self.action_dim, self.clip_rewards, self.image_key = action_dim, clip_rewards, image_key
        self.image_categorical, self.batched = image_categorical, batched

    def __call__(self, obs):
        lead = (np.newaxis,) if self.batched else (np.newaxis, np.newaxis)
        batch = {k: np.asarray(v)[lead] for k, v in obs.items() if k not in _LOGGED_BY_ACTOR}
        return preprocess_batch(batch, self.action_dim, clip_rewards=self.clip_rewards, image_key=self.image_key,
                                image_categorical=self.image_categorical)


class CarriedStatePolicy:
    """What every policy that acts through the world model shares: the recurrent state carried on the device between calls
    (reset_state), the step's preprocessing and upload (_ingest) and its ONE device-to-host copy (_emit).  NetworkPolicy acts with
    an actor, planner.PlannerPolicy with the planner."""

    def __init__(self, model, preprocess, batch_size=1, device=None, per_env=False):
        self.model, self.preprocess, self.batch_size, self.per_env = model, preprocess, int(batch_size), bool(per_env)
        if device is None:
            device = next(model.parameters()).device
        self.device = torch.device(device)
        self.state = self._to_device(model.init_state(self.batch_size))

    def _to_device(self, state):
        if isinstance(state, (tuple, list)):
            return tuple(self._to_device(s) for s in state)
        return state.to(self.device)

    def reset_state(self, mask=None):
        """Zero the carried state of the environments where `mask` ((B,) bools) is set - all of them without a mask - for callers
        whose preprocessing does not emit `reset`."""
        fresh = self._to_device(self.model.init_state(self.batch_size))
        if mask is None:
            self.state = fresh
            return
        m = torch.as_tensor(np.asarray(mask, dtype=bool)).to(self.device)
        if tuple(m.shape) != (self.batch_size,):
            raise ValueError(f'reset mask has shape {tuple(m.shape)}, expected ({self.batch_size},)')

        def pick(old, new):      # states are (..., B, width): the mask runs over the batch axis
            if isinstance(old, (tuple, list)):
                return tuple(pick(o, n) for o, n in zip(old, new))
            return torch.where(m.view((1,) * (old.dim() - 2) + (-1, 1)), new, old)

        self.state = pick(self.state, fresh)

    def _ingest(self, obs):
        """The environment's observation dict -> (the model's (1, B, ...) device tensors, B)."""
        batch = self.preprocess.apply(obs, expandTB=True) if hasattr(self.preprocess, 'apply') else self.preprocess(obs)
        obs_model = {k: torch.from_numpy(np.ascontiguousarray(v)).to(self.device, non_blocking=True) for k, v in batch.items()}
        B = obs_model['action'].shape[1]
        if B != self.batch_size:
            raise ValueError(f'the preprocessed observation holds {B} environments, this policy was built for {self.batch_size}')
        return obs_model, B

    def _emit(self, action, tail, B):
        """The step's single device-to-host wait: the action and `tail` - the three scalars in METRIC_KEYS order, per_env: three
        (B,) rows - in one buffer."""
        host = torch.cat([action.reshape(-1)] + tail).cpu().numpy()
        A = action.shape[-1]
        act = host[:B * A].reshape(B, A)
        if B == 1:
            act = act[0]      # (1,1,A) => A
        if self.per_env:
            return act.copy(), {k: host[B * A + i * B:B * A + (i + 1) * B].copy() for i, k in enumerate(METRIC_KEYS)}
        return act.copy(), {k: float(host[B * A + i]) for i, k in enumerate(METRIC_KEYS)}


class NetworkPolicy(CarriedStatePolicy):
    """generator.py:311-331.  `preprocess`: any callable from the environment's observation dict to numpy (1, B, ...) fields
    (StepPreprocessor above; an object with the reference's `.apply(obs, expandTB=True)` is taken too).  __call__ returns
    (action ndarray, {policy_value, action_prob, policy_entropy} as Python floats); the action is (A,) for batch_size == 1 as in
    the reference, (B, A) otherwise.  The recurrent state is carried on the device between calls.
    mode, action_noise: Dreamer.act's ('mode' for evaluation; action_noise > 0 for DreamerV2's exploration noise).  per_env=True:
    the three metrics are (B,) float32 arrays, one number per environment - the critic's value, exp(log_prob) and the entropy of
    act(..., return_rows=True) - in the same single copy as the action; what an EpisodeRecorder (collect.py) stores per step.
    ac: the actor-critic handed to Dreamer.act (the exploration policy of explore.Plan2Explore); None: the model's own."""

    def __init__(self, model, preprocess, batch_size=1, device=None, mode='sample', action_noise=0.0, per_env=False, ac=None):
        self.ac = ac      # the actor-critic that acts (Dreamer.act's `ac`: explore.Plan2Explore's); None: the model's own
        if mode not in ('sample', 'mode'):
            raise ValueError(f"mode is {mode!r}, expected 'sample' or 'mode'")
        if not float(action_noise) >= 0.0 or (float(action_noise) > 0.0 and mode == 'mode'):
            raise ValueError(f'action_noise is {action_noise} with mode {mode!r}: expected >= 0, and 0 with mode=\'mode\'')
        self.mode, self.action_noise = mode, float(action_noise)
        super().__init__(model, preprocess, batch_size, device, per_env)

    def __call__(self, obs):
        obs_model, B = self._ingest(obs)
        kw = {}
        if self.mode != 'sample' or self.action_noise > 0.0:      # the defaults are the call as it always was
            kw.update(mode=self.mode, action_noise=self.action_noise)
        if self.per_env:
            kw.update(return_rows=True)
        if self.ac is not None:
            kw.update(ac=self.ac)
        action, self.state, metrics = self.model.act(obs_model, self.state, **kw)
        if self.per_env:
            tail = [metrics['value'].reshape(B), metrics['log_prob'].reshape(B).exp(), metrics['entropy'].reshape(B)]
        else:
            tail = [metrics[k].reshape(1) for k in METRIC_KEYS]
        return self._emit(action, tail, B)


class RandomPolicy:
    """generator.py:303-308, the prefill policy, for batch_size environments: uniform one-hot actions, or with continuous=True
    uniform actions in [-1, 1); no metrics.  The action is (A,) for batch_size == 1, (B, A) otherwise, float32; the same seed gives
    the same actions."""

    def __init__(self, action_dim, batch_size=1, seed=None, continuous=False):
        self.action_dim, self.batch_size, self.continuous = int(action_dim), int(batch_size), bool(continuous)
        if self.action_dim < 1 or self.batch_size < 1:
            raise ValueError(f'action_dim={action_dim} batch_size={batch_size}')
        self.rng = np.random.RandomState(seed)

    def __call__(self, obs):
        B, A = self.batch_size, self.action_dim
        if self.continuous:
            act = self.rng.uniform(-1.0, 1.0, (B, A)).astype(np.float32)
        else:
            act = np.zeros((B, A), np.float32)
            act[np.arange(B), self.rng.randint(0, A, B)] = 1.0
        return (act[0] if B == 1 else act), {}
