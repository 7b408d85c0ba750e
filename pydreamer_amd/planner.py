"""Latent-space planning: what the world model itself says is the best action, by the cross-entropy method (PlaNet's
planner) over open-loop rollouts of the RSSM.  CEMPlanner.plan is the search from a batch of model states, CEMPlanner.act puts the
world model's posterior step in front of it like Dreamer.act, and PlannerPolicy is NetworkPolicy's call protocol on top - what
collect(), Collector and EpisodeRecorder take unchanged.  The candidate draw and the per-environment update are csrc/cem.hip; the
rollout is dm_rssm_sequence_fwd under the open-loop parameter substitution (models.open_loop_struct), the heads are the decoder's
dream forward and the critic."""
import ctypes

import torch

from . import hip as H
from .models import _grow_ws, open_loop_struct
from .policy import METRIC_KEYS, CarriedStatePolicy

MAX_CANDIDATES, MAX_HORIZON = 1024, 64      # csrc/cem.hip's bounds on J and Hp


class CEMPlanner:
    """CEM over action sequences in the model's latent space.  horizon Hp, candidates J, elites K, iters, alpha (the share of the
    previous proposal kept by the refit), floor (the uniform-mix share of a one-hot proposal; the minimum std of a continuous
    one), use_value (the critic on the last imagined state closes the return): None takes model.conf's plan_* key.  ac: the
    actor-critic whose critic, discount and action kind are used; None: the model's own.  The actor is never evaluated."""

    def __init__(self, model, horizon=None, candidates=None, elites=None, iters=None, alpha=None, floor=None, use_value=None, ac=None):
        c = model.conf
        pick = lambda v, key: getattr(c, key) if v is None else v
        self.model, self.ac = model, (model.ac if ac is None else ac)
        self.horizon, self.candidates = int(pick(horizon, 'plan_horizon')), int(pick(candidates, 'plan_candidates'))
        self.elites, self.iters = int(pick(elites, 'plan_elites')), int(pick(iters, 'plan_iters'))
        self.alpha, self.floor = float(pick(alpha, 'plan_alpha')), float(pick(floor, 'plan_floor'))
        self.use_value = bool(pick(use_value, 'plan_value'))
        if not 1 <= self.candidates <= MAX_CANDIDATES:
            raise ValueError(f'candidates={self.candidates}: 1 .. {MAX_CANDIDATES}')
        if not 1 <= self.elites <= self.candidates:
            raise ValueError(f'elites={self.elites}: 1 .. candidates={self.candidates}')
        if not 1 <= self.horizon <= MAX_HORIZON:
            raise ValueError(f'horizon={self.horizon}: 1 .. {MAX_HORIZON}')
        if self.iters < 1:
            raise ValueError(f'iters={self.iters}: at least 1')
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError(f'alpha={self.alpha}: 0 .. 1')
        if not self.floor >= 0.0 or (self.ac.dist_kind == 0 and self.floor > 1.0):
            raise ValueError(f'floor={self.floor}: >= 0, and a share <= 1 for one-hot actions')
        if c.action_dim > 64:
            raise ValueError(f'action_dim={c.action_dim}: the planning kernels take up to 64')
        self._ws = None

    # ---- sizes
    def _shape(self, M):
        """The chain's geometry for M candidate rows; no image stage runs here, so none is sized."""
        shp = self.model.wm.shape(self.horizon, M, 1)
        shp.cnn_depth = shp.img = shp.img_ch = 0
        return shp

    def _ws_bytes(self, M):
        """Scratch for the chain and the heads on Hp M rows."""
        rows, lib = self.horizon * M, H.lib()
        heads = [h.model for _, h, _ in self.model.wm.decoder.heads()[:2]] + [self.ac.critic]
        return max([H.workspace_bytes(self._shape(M))] +
                   [4 * int(lib.dm_mlp_ws_floats(rows, m.hidden_dim, m.hidden_layers)) for m in heads])

    # ---- the search
    def plan(self, feat, noise=None, keep_iterations=False, keep_rollout=False):
        """feat: (B, F) rows [h|z] as WorldModel.forward returns them.  noise: dict with u_cand (iters, Hp, M) uniforms for one-hot
        actions or (iters, Hp, M, A) standard normals for continuous ones, and / or u_prior (iters, Hp, M, S) - uniforms for
        categorical latents, standard normals for Gaussian ones; M = B J, row m = b J + j.  What is missing is drawn on the device.
        Returns dict(action (B,A), stats (B,4), prop, ret (M,), elite (B,K)) of the last iteration; keep_iterations: also
        `iterations`, a list of (stats, ret) clones per iteration; keep_rollout: also `rollout`, the last iteration's imagined
        features (Hp, M, F), actions (Hp, M, A), reward and terminal means (Hp, M) and values (M,) or None (a test's view).
        No gradient, the caller's stream, no host synchronisation.  The environments are planned one after the other (below): the
        result for an environment is, bit for bit, what plan() gives for it alone."""
        wm, ac, c = self.model.wm, self.ac, self.model.conf
        B, F_ = feat.shape
        if F_ != wm.features_dim:
            raise ValueError(f'feature rows are {F_} wide, the model has {wm.features_dim}')
        Hp, J, K, A, S = self.horizon, self.candidates, self.elites, c.action_dim, c.stoch_dim
        kind, dev, M, D_ = ac.dist_kind, feat.device, B * J, c.deter_dim
        noise = noise or {}
        uc_shape = (self.iters, Hp, M) if kind == 0 else (self.iters, Hp, M, A)
        u_cand, u_prior = noise.get('u_cand'), noise.get('u_prior')
        if u_cand is not None and tuple(u_cand.shape) != uc_shape:
            raise ValueError(f'candidate noise has shape {tuple(u_cand.shape)}, expected {uc_shape}')
        if u_prior is not None and tuple(u_prior.shape) != (self.iters, Hp, M, S):
            raise ValueError(f'prior noise has shape {tuple(u_prior.shape)}, expected {(self.iters, Hp, M, S)}')
        with torch.no_grad():
            feat = feat.float().contiguous()
            if kind == 0:
                prop = torch.full((B, Hp, A), 1.0 / A, device=dev)
            else:
                prop = torch.cat((torch.zeros(B, Hp, A, device=dev), torch.ones(B, Hp, A, device=dev)), -1)
            out = dict(action=torch.empty(B, A, device=dev), stats=torch.empty(B, 4, device=dev), prop=prop,
                       ret=torch.empty(M, device=dev), elite=torch.empty(B, K, dtype=torch.int32, device=dev))
            its = [(torch.empty(B, 4, device=dev), torch.empty(M, device=dev)) for _ in range(self.iters)] if keep_iterations else None
            roll = None
            if keep_rollout:
                roll = dict(features=torch.empty(Hp, M, F_, device=dev), actions=torch.empty(Hp, M, A, device=dev),
                            reward=torch.empty(Hp, M, device=dev), terminal=torch.empty(Hp, M, device=dev),
                            value=torch.empty(M, device=dev) if self.use_value else None)
            # One environment per launch, always: the library's products pick their schedule by row count, so the last bits of a row
            # depend on how many rows travel with it (measured: M = 24 against M = 8 moved the returns' last bits).  Launched alone,
            # an environment's plan is a function of its own state and noise - it does not depend on B or on its neighbours - and
            # the transient memory is that of Hp J rows whatever B is.
            for b in range(B):
                self._plan_envs(feat, b, b + 1, u_cand, u_prior, out, its, roll)
        if its is not None:
            out['iterations'] = its
        if roll is not None:
            out['rollout'] = roll
        return out

    def _plan_envs(self, feat, b0, b1, u_cand, u_prior, out, its, roll):
        """All iterations for the environments [b0, b1) as ONE batch of launches, into their rows of `out` (plan() hands over one
        environment at a time)."""
        wm, ac, c = self.model.wm, self.ac, self.model.conf
        Hp, J, K, A, S = self.horizon, self.candidates, self.elites, c.action_dim, c.stoch_dim
        kind, dev, D_, F_ = ac.dist_kind, feat.device, c.deter_dim, wm.features_dim
        Bc = b1 - b0
        Mc, m0, m1 = Bc * J, b0 * J, b1 * J
        N = Hp * Mc
        gauss = not c.stoch_discrete
        ZP = S * (c.stoch_discrete or 2)
        shp, lib = self._shape(Mc), H.lib()
        ws = self._ws = _grow_ws(self._ws, self._ws_bytes(Mc), dev)
        # the start states, each environment's row J times (row m = b J + j)
        start = feat[b0:b1].repeat_interleave(J, dim=0)
        h0, z0 = start[:, :D_].contiguous(), start[:, D_:].contiguous()
        embed = torch.zeros(N, wm.encoder.out_dim, device=dev)
        reset = torch.zeros(Hp, Mc, dtype=torch.uint8, device=dev)
        rssm_p = open_loop_struct(wm.core.cell)
        rssm_acts = torch.empty(int(lib.dm_rssm_acts_floats(ctypes.byref(shp))), device=dev)
        feats = torch.empty(N, F_, device=dev)
        post, prior = torch.empty(N, ZP, device=dev), torch.empty(N, ZP, device=dev)
        idx = torch.empty(N, S, dtype=torch.int32, device=dev)
        actions = torch.empty(Hp, Mc, A, device=dev)
        act_idx = torch.empty(Hp, Mc, dtype=torch.int32, device=dev) if kind == 0 else None
        dec = wm.decoder
        outs = dec.dream_buffers(N, dev)
        prop, ret, elite = out['prop'][b0:b1], out['ret'][m0:m1], out['elite'][b0:b1]
        action, stats = out['action'][b0:b1], out['stats'][b0:b1]
        uc_shape = (Hp, Mc) if kind == 0 else (Hp, Mc, A)
        for it in range(self.iters):
            if u_cand is not None:
                uc = u_cand[it][:, m0:m1].float().contiguous()
            else:
                uc = torch.rand(uc_shape, device=dev) if kind == 0 else torch.randn(uc_shape, device=dev)
            if u_prior is not None:
                up = u_prior[it][:, m0:m1].float().contiguous()
            else:
                up = (torch.randn if gauss else torch.rand)(Hp, Mc, S, device=dev)
            H.call('dm_cem_draw', kind, Bc, J, Hp, A, H.fptr(prop), H.fptr(uc), H.fptr(actions), H.ptr(act_idx), H.stream())
            H.call('dm_rssm_sequence_fwd', ctypes.byref(shp), H.fptr(embed), H.fptr(actions), H.ptr(reset), H.fptr(h0), H.fptr(z0),
                   H.fptr(up), None, ctypes.byref(rssm_p), H.fptr(rssm_acts), H.fptr(feats), H.fptr(post), H.fptr(prior), H.ptr(idx),
                   H.ptr(ws), ws.numel(), H.stream())
            dec.dream_fwd(feats, 0, N, ws, outs)
            term, mu = dec.dream_means(outs)
            value = None
            if self.use_value:
                value, _ = ac.value(feats[(Hp - 1) * Mc:], F_, Mc, ws)
            H.call('dm_cem_update', kind, Bc, J, K, Hp, A, float(ac.gamma), H.fptr(mu), H.fptr(term), H.fptr(value), H.fptr(actions),
                   H.ptr(act_idx), H.fptr(prop), self.alpha, self.floor, H.fptr(prop), H.fptr(ret), H.ptr(elite), H.fptr(action),
                   H.fptr(stats), H.stream())
            if its is not None:
                its[it][0][b0:b1].copy_(stats)
                its[it][1][m0:m1].copy_(ret)
        if roll is not None:
            roll['features'][:, m0:m1].copy_(feats.view(Hp, Mc, F_))
            roll['actions'][:, m0:m1].copy_(actions)
            roll['reward'][:, m0:m1].copy_(mu.view(Hp, Mc))
            roll['terminal'][:, m0:m1].copy_(term.view(Hp, Mc))
            if value is not None:
                roll['value'][m0:m1].copy_(value.view(Mc))

    # ---- acting (Dreamer.act's shape)
    def act(self, obs, in_state, noise=None, return_rows=False):
        """The world model's posterior step on `obs`, then plan() from its features.  Returns (action (1,B,A), out_state, metrics):
        metrics = {policy_value: the mean best return, action_prob: the mean of the final proposal's probability of the executed
        action (0 for continuous actions), policy_entropy: the mean of the final proposal's first-step entropy (continuous: sum of
        log std)} as 0-dim device tensors.  return_rows=True adds value, log_prob (the log of the probability; 0 for continuous
        actions), entropy and prob (the probability itself) as (B,) rows.  noise: u_post (1,B,S) for the posterior draw, u_cand /
        u_prior for plan()."""
        assert 'action' in obs, 'Observation should contain previous action'
        act_shape = obs['action'].shape
        assert len(act_shape) == 3 and act_shape[0] == 1, f'Expected shape (1,B,A), got {act_shape}'
        B = act_shape[1]
        noise = noise or {}
        with torch.no_grad():
            self.model.join_optimizers()
            features, out_state = self.model.wm.forward(obs, in_state, noise.get('u_post'))
            res = self.plan(features.reshape(B, -1), noise)
            stats = res['stats']
            means = stats.mean(0)
            metrics = dict(policy_value=means[0], action_prob=means[3], policy_entropy=means[2])
            if return_rows:
                lp = stats[:, 3].log() if self.ac.dist_kind == 0 else torch.zeros(B, device=stats.device)
                metrics.update(value=stats[:, 0], log_prob=lp, entropy=stats[:, 2], prob=stats[:, 3])
        return res['action'].view(1, B, -1), out_state, metrics


class PlannerPolicy(CarriedStatePolicy):
    """NetworkPolicy's call protocol with CEMPlanner.act in place of Dreamer.act: __call__(obs) -> (action ndarray, {policy_value,
    action_prob, policy_entropy}), (A,) for batch_size == 1 and (B, A) otherwise, one device-to-host copy per environment step,
    the recurrent state carried on the device, reset_state.  per_env=True: the three metrics are (B,) rows - each environment's
    best return, the final proposal's probability of the executed action and its first-step entropy.  planner_kwargs: CEMPlanner's
    (horizon, candidates, elites, iters, alpha, floor, use_value, ac)."""

    def __init__(self, model, preprocess, batch_size=1, device=None, per_env=False, **planner_kwargs):
        self.planner = CEMPlanner(model, **planner_kwargs)
        super().__init__(model, preprocess, batch_size, device, per_env)

    def __call__(self, obs):
        obs_model, B = self._ingest(obs)
        action, self.state, metrics = self.planner.act(obs_model, self.state, return_rows=self.per_env)
        keys = ('value', 'prob', 'entropy') if self.per_env else METRIC_KEYS
        return self._emit(action, [metrics[k].reshape(-1) for k in keys], B)
