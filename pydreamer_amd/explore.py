"""Plan2Explore (Sekar et al. 2020, as in DreamerV2's expl.py; the reference has no counterpart - its README lists it as the one
feature DreamerV2 has and pydreamer lacks): exploration by the disagreement of an ensemble.

  * `ensemble`: K one-step predictors, MLPs from [feature_t | action taken in state t] to the stochastic part of feature_{t+1},
    trained on the replayed window with a Normal(mean, 1) loss (dm_ensemble_mse).
  * the intrinsic reward of an imagined transition is the ensemble's disagreement on it: the standard deviation over the K
    predicted means, averaged over the target's columns (dm_disag_reward).
  * `ac`: a second ActorCritic, trained in imagination on that reward and used to collect data (Dreamer.act(ac=...)).

Plan2Explore holds the Dreamer by an UNREGISTERED reference: the two state_dicts stay separate and the Dreamer's keys stay the
reference's.  Everything here runs on the caller's stream, behind the Dreamer's training_step(); the Dreamer's own losses, metric
buffer and gradients are not touched.  The MLPs run through MLP.fwd / bwd_into, one head after the other.
"""
import ctypes

import torch
import torch.nn as nn

from . import hip as H
from .models import (METRIC_BUF_FLOATS, MLP, MLP_HIDDEN, ActorCritic, _grow_ws, _multi_sum, _Params, _ProbeLoss, _require_cuda,
                     init_weights_tf2)
from .optim import FusedAdamW

DISAG_MAX_MODELS = 16      # dm_disag_reward keeps the K values of a column in registers
# The exploration step's own metric buffer (METRIC_BUF_FLOATS floats, the Dreamer's layout where the ActorCritic writes: slots
# 8-14 are ActorCritic.training_step's): names -> slots, what a MetricAccumulator over this buffer reads.
EXPLORE_METRIC_SLOTS = dict(loss_disag=0, expl_reward=1, expl_reward_std=2, expl_loss_critic=8, expl_loss_actor=9,
                            expl_policy_entropy=10, expl_policy_value=11, expl_policy_value_im=12, expl_policy_reward=13,
                            expl_policy_reward_std=14, grad_norm_disag=16, grad_norm_expl_actor=20, grad_norm_expl_critic=22)
EXPLORE_GRAD_NORMS = ('grad_norm_disag', 'grad_norm_expl_actor', 'grad_norm_expl_critic')
_CHUNK_FLOATS = 1 << 26      # the K heads' outputs over the imagined rows are made and reduced in row chunks of this many floats


def log_name(name):
    """The trainer's key of an exploration scalar: every one under expl_ (train/expl_loss_disag, train/expl_grad_norm_actor)."""
    return 'expl_' + name.replace('expl_', '')


class _Ensemble(_Params):
    """The K heads; `_fused` (set by init_optimizers) is their one optimizer, whose gradient buffer _ProbeLoss claims once."""

    def __init__(self, K, in_dim, out_dim, layer_norm):
        super().__init__()
        self.heads = nn.ModuleList([MLP(in_dim, out_dim, MLP_HIDDEN, 4, layer_norm) for _ in range(K)])


class Plan2Explore(nn.Module):
    def __init__(self, conf, dreamer):
        super().__init__()
        if int(getattr(conf, 'iwae_samples', 1)) > 1:
            raise NotImplementedError('Plan2Explore with iwae_samples > 1 is not built: the ensemble is trained on one posterior '
                                      'sample per step')
        K = int(conf.disag_models)
        if not 2 <= K <= DISAG_MAX_MODELS:
            raise ValueError(f'disag_models={K}: the disagreement kernels take 2 .. {DISAG_MAX_MODELS} heads')
        self.__dict__['_dreamer'] = dreamer      # not a submodule: separate state_dicts, the Dreamer's keys stay the reference's
        self.conf = conf
        self.K = K
        self.action_cond = bool(conf.disag_action_cond)
        self.intr_scale, self.extr_scale = float(conf.expl_intr_scale), float(conf.expl_extr_scale)
        F_ = conf.deter_dim + conf.stoch_dim * (conf.stoch_discrete or 1)
        self.features_dim, self.deter_dim = F_, conf.deter_dim
        self.target_dim = conf.stoch_dim * (conf.stoch_discrete or 1)
        self.in_dim = F_ + (conf.action_dim if self.action_cond else 0)
        self.ensemble = _Ensemble(K, self.in_dim, self.target_dim, conf.layer_norm)
        for m in self.ensemble.modules():      # DreamerV2's heads are Keras layers: Glorot-uniform weights, zero biases
            init_weights_tf2(m)
        self.ac = ActorCritic(in_dim=F_, out_actions=conf.action_dim, layer_norm=conf.layer_norm, gamma=conf.gamma,
                              lambda_gae=conf.lambda_gae, entropy_weight=conf.entropy, target_interval=conf.target_interval,
                              actor_grad=conf.actor_grad, actor_dist=conf.actor_dist)
        self.ac.sparse_cols = conf.stoch_dim * conf.stoch_discrete
        for m in self.modules():
            if isinstance(m, MLP):
                m.precision = int(bool(getattr(conf, 'amp', False)))
        self._opt = None
        self._ws = None
        self.metric_buffer = None
        self.last_extras = {}

    @property
    def dreamer(self):
        return self._dreamer

    @property
    def heads(self):
        return list(self.ensemble.heads)

    # ---- optimizers
    def init_optimizers(self, lr=None, lr_actor=None, lr_critic=None, eps=None):
        """Three FusedAdamW: the ensemble (one group, conf.adam_lr_expl), the exploration actor and critic (the task ones'
        rates)."""
        c = self.conf
        eps = c.adam_eps if eps is None else eps
        self._opt = dict(disag=FusedAdamW(list(self.ensemble.parameters()), lr=lr or c.adam_lr_expl, eps=eps),
                         actor=FusedAdamW(list(self.ac.actor.parameters()), lr=lr_actor or c.adam_lr_actor, eps=eps),
                         critic=FusedAdamW(list(self.ac.critic.parameters()), lr=lr_critic or c.adam_lr_critic, eps=eps))
        self.ensemble._fused, self.ac.actor._fused, self.ac.critic._fused = self._opt['disag'], self._opt['actor'], self._opt['critic']
        return self._opt['disag'], self._opt['actor'], self._opt['critic']

    def grad_clip(self, grad_clip, grad_clip_ac=None):
        if self._opt is None:
            raise RuntimeError('call init_optimizers() before grad_clip(): clipping runs on the optimizers\' flat buffers')
        o, mb = self._opt, self.metric_buffer
        if mb is not None and mb.device != o['disag'].flat_grad.device:
            mb = None
        out = lambda name: None if mb is None else mb[EXPLORE_METRIC_SLOTS[name]:EXPLORE_METRIC_SLOTS[name] + 2]
        return dict(grad_norm_disag=o['disag'].clip_grad_norm(grad_clip, out('grad_norm_disag')),
                    grad_norm_expl_actor=o['actor'].clip_grad_norm(grad_clip_ac or grad_clip, out('grad_norm_expl_actor')),
                    grad_norm_expl_critic=o['critic'].clip_grad_norm(grad_clip_ac or grad_clip, out('grad_norm_expl_critic')))

    # ---- the Dreamer's last step
    def step_features(self):
        """The detached (T*B, F) feature matrix [h | z] of the Dreamer's last training_step(), row t*B + b."""
        pk = getattr(self._dreamer.wm, '_last_pack', None)
        if not isinstance(pk, dict) or pk.get('feat') is None:
            raise RuntimeError('Plan2Explore.training_step() reads the feature matrix of Dreamer.training_step(): call that first')
        return pk['feat']

    def _workspace(self, rows, device):
        need = 4 * int(H.lib().dm_mlp_ws_floats(rows, MLP_HIDDEN, 4))
        self._ws = _grow_ws(self._ws, need, device)
        return self._ws

    def _rows(self, feat2d, ldx, extra, rows, out=None):
        """[feature | action] rows (dm_cat_concat_rows, I = 1); the bare feature rows without disag_action_cond."""
        if not self.action_cond:
            return feat2d, ldx
        if out is None:
            out = torch.empty(rows, self.in_dim, device=feat2d.device)
        A = self.in_dim - self.features_dim
        H.call('dm_cat_concat_rows', rows, 1, self.features_dim, A, H.fptr(feat2d), ldx, H.fptr(extra), H.fptr(out), H.stream())
        return out, self.in_dim

    def predict(self, feat2d, act2d, means=None, xbuf=None):
        """The K heads' means for `rows` transitions: feat2d (rows, F), act2d (rows, A) (ignored without disag_action_cond) ->
        (K, rows, Dt); row r of head k lies at means[k, r].  means / xbuf: the caller's buffers, at least rows long."""
        rows, dev = feat2d.shape[0], feat2d.device
        if means is None:
            means = torch.empty(self.K, rows, self.target_dim, device=dev)
        x, ldx = self._rows(feat2d, feat2d.shape[1], act2d, rows, out=xbuf)
        ws = self._workspace(rows, dev)
        for k, head in enumerate(self.ensemble.heads):
            head.fwd(x, ldx, rows, ws, save_acts=False, window=(rows, 0), out=means[k, :rows])
        return means

    def intrinsic_reward(self, features, actions, out=None):
        """features (H+1, M, F), actions (H, M, A) of an imagined rollout -> (H+1, M): row 0 is zero, row i + 1 is
        expl_intr_scale x the ensemble's disagreement on the transition (features[i], actions[i]) - a2c.py's ordering, reward[i+1]
        pays for what was done in state i.  The heads' outputs are made and reduced in row chunks (a row's reward does not depend
        on the chunk it falls into)."""
        J, M, F_ = features.shape
        Hh, K, Dt, dev = J - 1, self.K, self.target_dim, features.device
        if out is None:
            out = torch.zeros(J, M, device=dev)
        rows = Hh * M
        f2 = features.contiguous().view(J * M, F_)
        a2 = actions.contiguous().view(rows, -1)
        flat = out.view(-1)
        chunk = max(1, min(rows, _CHUNK_FLOATS // (K * Dt)))
        means = torch.empty(K, chunk, Dt, device=dev)
        xbuf = torch.empty(chunk, self.in_dim, device=dev) if self.action_cond else None
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            self.predict(f2[r0:r0 + n], a2[r0:r0 + n], means=means, xbuf=xbuf)
            H.call('dm_disag_reward', K, n, Dt, H.fptr(means), chunk * Dt, Dt, self.intr_scale, H.fptr(flat[M + r0:M + r0 + n]),
                   H.stream())
        return out

    # ---- the step
    def training_step(self, noise=None):
        """Behind Dreamer.training_step(...) (before or after its backward()s): trains the ensemble on that step's window and the
        exploration actor-critic on the ensemble's disagreement over its own imagined rollout.  noise: dict(u_act (H,M) / eps_act
        (H,M,A), u_prior (H,M,S)) as Dreamer.training_step's.  Returns ((loss_disag, loss_expl_actor, loss_expl_critic), metrics);
        each loss supports its own backward().  Metrics are 0-dim views of this module's metric_buffer."""
        d = self._dreamer
        feat = self.step_features()
        _require_cuda(feat, 'features')
        pk = d.wm._last_pack
        action, reset = pk['action'], pk['reset']
        T, B = action.shape[:2]
        F_, Dt, K, dev = self.features_dim, self.target_dim, self.K, feat.device
        if feat.shape != (T * B, F_):
            raise NotImplementedError(f'the feature matrix is {tuple(feat.shape)}, expected {(T * B, F_)}: Plan2Explore is built '
                                      f'for iwae_samples = 1')
        if T < 2:
            raise ValueError('Plan2Explore needs a window of at least two steps: the ensemble predicts step t + 1 from step t')
        noise = noise or {}
        train = torch.is_grad_enabled()
        mbuf = torch.zeros(METRIC_BUF_FLOATS, device=dev)
        self.metric_buffer = mbuf
        N = (T - 1) * B
        with torch.no_grad():
            # ---- the ensemble on the replayed window: [feat_t | action_{t+1}] -> stoch part of feat_{t+1}, skipped where t+1 resets
            act_next = action.float().contiguous().view(T * B, -1)[B:]
            skip = reset.contiguous().view(T * B)[B:]
            skip = skip.view(torch.uint8) if skip.dtype == torch.bool else skip.to(torch.uint8)
            x, ldx = self._rows(feat, F_, act_next, N)
            ws = self._workspace(N, dev)
            means = torch.empty(K, N, Dt, device=dev)
            dmeans = torch.empty(K, N, Dt, device=dev) if train else None
            packs = []
            for k, head in enumerate(self.ensemble.heads):
                acts = torch.empty(head.acts_floats(N), device=dev) if train else None
                head.fwd(x, ldx, N, ws, acts=acts, save_acts=train, window=(N, 0), out=means[k])
                if train:
                    packs.append(dict(mlp=head, x=x, ldx=ldx, rows=N, acts=acts, dout=dmeans[k], ws=ws))
            loss_rows = torch.empty(K, N, device=dev)
            target = ctypes.c_void_p(feat.data_ptr() + 4 * (B * F_ + self.deter_dim))      # feat[B:, deter_dim:], in place
            H.call('dm_ensemble_mse', K, N, Dt, H.fptr(means), N * Dt, Dt, target, F_, H.ptr(skip), 1.0 / N, H.fptr(loss_rows),
                   H.fptr(dmeans), H.stream())
            _multi_sum([(loss_rows, 1.0 / N)], dev, out=mbuf[0:1])
            loss_disag_v = mbuf[0]

            # ---- the exploration behaviour: its own rollout from the same start rows, rewarded by the disagreement
            Hh = int(d.imag_horizon)
            self.ac.begin_step(log_only=not train)
            dpk = {}
            feats_d, actions_d, rewards_d, terminals_d = d._dream_from_features(
                feat, Hh, noise.get('u_act') if self.ac.dist_kind == 0 else noise.get('eps_act'), noise.get('u_prior'),
                _pack=dpk, ac=self.ac)
            M = feats_d.shape[1]
            rewards = self.intrinsic_reward(feats_d, actions_d)
            intr = rewards.view(-1)[M:]
            n_r = intr.numel()
            _multi_sum([(intr, 1.0 / n_r)], dev, out=mbuf[1:2])
            _multi_sum([(intr, 1.0 / max(n_r - 1, 1), mbuf[1:2], 2)], dev, out=mbuf[2:3])
            if self.extr_scale != 0.0:
                H.call('dm_axpby', rewards.numel(), self.extr_scale, H.fptr(rewards_d.mean.contiguous()), 1.0, H.fptr(rewards),
                       H.stream())
        (loss_actor, loss_critic), metrics_ac, tensors_ac = self.ac.training_step(
            feats_d, actions_d, rewards, terminals_d.mean, log_only=not train, act_idx=dpk['act_idx'], ws=dpk['ws'],
            actor_acts=dpk['actor_acts'], actor_logits=dpk['actor_logits'], mbuf=mbuf, values=dpk['values'], _begun=True)
        if train:
            loss_disag = _ProbeLoss.apply(self.ensemble, dict(loss=loss_disag_v, heads=packs), *self.ensemble.parameters())
        else:
            loss_disag = loss_disag_v
        metrics = dict(loss_disag=mbuf[0], expl_reward=mbuf[1], expl_reward_std=mbuf[2])
        metrics.update({f'expl_{k}': v for k, v in metrics_ac.items()})
        # diagnostics for tests / debugging, the step's own buffers
        self.last_extras = dict(dream_features=feats_d, actions=actions_d, act_idx=dpk['act_idx'], rewards=rewards,
                                reward_pred=rewards_d.mean, terminal_pred=terminals_d.mean, actor_logits=dpk['actor_logits'],
                                ac_tensors=tensors_ac, values=dpk['values'])
        return (loss_disag, loss_actor, loss_critic), metrics

    # ---- trainer plumbing
    def packed_metrics(self):
        """(names, buffer, idx) of the last step, as Dreamer.packed_metrics()."""
        names = list(EXPLORE_METRIC_SLOTS)
        return names, self.metric_buffer, [EXPLORE_METRIC_SLOTS[n] for n in names]
