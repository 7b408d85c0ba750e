"""The wrapped-environment protocol collect() documents, over a raw environment (wrappers.py:10-72, 96-111 as behaviour; DESIGN
4.16): reset() -> obs dict, step(action) -> (obs dict, reward, done, info), the dict carrying action / reward / terminal / reset.
No gym: a raw environment is any object with reset() -> obs (or (obs, info)) and step(action) -> (obs, reward, done, info) (or
(obs, reward, terminated, truncated, info)).  Not here: the restart-on-exception wrapper and the per-suite adapters."""
import numpy as np


class WrappedEnv:
    """wrap_env()'s object.  In the reference's order: the dict observation (wrappers.py:10-21), the time limit (24-40), the
    one-hot action in front of a discrete environment (96-111), then action / reward / terminal / reset (43-72)."""

    def __init__(self, env, action_dim, time_limit=0, no_terminal=False, discrete=False):
        self.env, self.action_dim, self.time_limit = env, int(action_dim), int(time_limit)
        self.no_terminal, self.discrete = bool(no_terminal), bool(discrete)
        if self.action_dim < 1 or self.time_limit < 0:
            raise ValueError(f'action_dim={action_dim} time_limit={time_limit}')
        self.step_ = 0

    @staticmethod
    def _dict(obs):
        if isinstance(obs, dict):
            return dict(obs)
        obs = np.asarray(obs)
        return {'vecobs': obs} if obs.ndim == 1 else {'image': obs}

    def reset(self):
        out = self.env.reset()
        if isinstance(out, tuple) and len(out) == 2 and isinstance(out[1], dict):      # (obs, info)
            out = out[0]
        self.step_ = 0
        obs = self._dict(out)
        obs['action'] = np.zeros(self.action_dim)
        obs['reward'] = np.array(0.0)
        obs['terminal'] = np.array(False)
        obs['reset'] = np.array(True)
        return obs

    def step(self, action):
        action_vec = np.asarray(action)
        if action_vec.shape != (self.action_dim,):
            raise ValueError(f'the action has shape {action_vec.shape}, expected ({self.action_dim},)')
        out = self.env.step(int(action_vec.argmax()) if self.discrete else action)
        if len(out) == 5:
            obs, reward, terminated, truncated, info = out
            done, info = bool(terminated) or bool(truncated), dict(info)
            if truncated:
                info['time_limit'] = True
        else:
            obs, reward, done, info = out
            done, info = bool(done), dict(info)
        self.step_ += 1
        if self.time_limit and self.step_ >= self.time_limit:
            done = True
            info['time_limit'] = True
        obs = self._dict(obs)
        obs['action'] = action_vec
        obs['reward'] = np.array(reward)
        obs['terminal'] = np.array(False if self.no_terminal or 'TimeLimit.truncated' in info or info.get('time_limit') else done)
        obs['reset'] = np.array(False)
        return obs, reward, done, info


def wrap_env(env, action_dim, time_limit=0, no_terminal=False, discrete=False):
    """A raw environment behind the protocol collect() drives.  A non-dict observation becomes {'vecobs': x} (1-D) or {'image': x};
    the action arrives one-hot (A,) and is passed on as int(argmax) when `discrete`, otherwise as it is, and obs['action'] is
    always the (A,) vector; reset() adds a zero action, reward 0.0, terminal False, reset True; step() adds reward, reset False
    and terminal = done, except False with no_terminal, 'TimeLimit.truncated' in info or info.get('time_limit').  time_limit > 0:
    the time_limit-th step of an episode returns done = True and info['time_limit'] = True.  A 5-tuple step result is taken too
    (done = terminated or truncated; truncated sets info['time_limit']), and a 2-tuple reset result (obs, info)."""
    return WrappedEnv(env, action_dim, time_limit=time_limit, no_terminal=no_terminal, discrete=discrete)


def wrap_envs(envs, conf, discrete=False):
    """wrap_env over a list, with conf.action_dim, conf.env_time_limit and conf.env_no_terminal."""
    return [wrap_env(env, conf.action_dim, time_limit=conf.env_time_limit, no_terminal=conf.env_no_terminal, discrete=discrete)
            for env in envs]
