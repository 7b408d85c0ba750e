"""Restatements of the two-hot symlog critic and the percentile return normalisation for the tests: the rule of
include/dreamer_hip.h (dm_twohot_decode / dm_twohot_loss / dm_return_norm) written with torch in whatever dtype it is handed - float64
is the reference, float32 the plain composition whose own error sizes the kernels' tolerance - and with numpy float32 scalars
where the header fixes every rounding (the percentile rule).  Pure CPU; nothing here touches the library."""
import numpy as np
import torch

from oracle import dreamer_oracle as O


def symlog(x):
    return torch.sign(x) * torch.log1p(x.abs())


def symexp(x):
    return torch.sign(x) * torch.expm1(x.abs())


def twohot_rows(target, bins):
    """(k, w_lo, w_hi) of every target: x = clamp(symlog(t), bins[0], bins[-1]), k = clamp(#{bins <= x} - 1, 0, K - 2)."""
    x = symlog(target).clamp(bins[0], bins[-1])
    k = ((bins[None, :] <= x[:, None]).sum(-1) - 1).clamp(0, bins.numel() - 2)
    w_hi = (x - bins[k]) / (bins[k + 1] - bins[k])
    return k, 1 - w_hi, w_hi


def twohot_compose(logits, bins, target, weight, scale):
    """loss (rows,), dlogits (rows, K), value (rows,) by log_softmax / gather / softmax . bins / expm1, in the dtype of `logits`."""
    lsm = torch.log_softmax(logits, -1)
    k, w_lo, w_hi = twohot_rows(target, bins)
    pick = lambda i: lsm.gather(-1, i[:, None])[:, 0]
    loss = -weight * (w_lo * pick(k) + w_hi * pick(k + 1))
    p = torch.softmax(logits, -1)
    y = torch.zeros_like(p).scatter_(-1, k[:, None], w_lo[:, None]).scatter_add_(-1, (k + 1)[:, None], w_hi[:, None])
    return loss, scale * weight[:, None] * (p - y), symexp((p * bins).sum(-1))


def twohot_decode(logits, bins):
    return symexp((torch.softmax(logits, -1) * bins).sum(-1))


def ulp32(x):
    """The fp32 unit in the last place at |x| (numpy array or scalar of any float dtype), at least that of the smallest normal."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


# ---------------------------------------------------------------------------------------------- the percentile rule, fp32 scalars
def sort_total(x):
    """x (float32 array) in the kernel's total order: ascending, -0 below +0."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    key = np.where(u >> 31, ~u, u | np.uint32(0x80000000))
    return np.asarray(x, np.float32)[np.argsort(key, kind='stable')]


def percentile_f32(s, q):
    """pos = fl(q fl(n - 1)); i = floor(pos); fr = fl(pos - i); fl(s_i + fl(fr fl(s_{i+1} - s_i))) on the sorted float32 array s."""
    f = np.float32
    n = len(s)
    pos = f(q) * f(n - 1)
    i = min(max(int(np.floor(pos)), 0), n - 1)
    fr = f(pos - f(i))
    s0, s1 = f(s[i]), f(s[min(i + 1, n - 1)])
    return f(s0 + f(fr * f(s1 - s0)))


def return_norm_f32(x, q_lo, q_hi, decay, limit, update, state, adv):
    """dm_return_norm restated: returns (out[5], state[2], adv) as float32 arrays; `state` and `adv` are not modified."""
    f = np.float32
    s = sort_total(x)
    p = [percentile_f32(s, q_lo), percentile_f32(s, q_hi)]
    lo, hi = f(state[0]), f(state[1])
    if update:
        om = f(f(1) - f(decay))
        lo = f(f(f(decay) * lo) + f(om * p[0]))
        hi = f(f(f(decay) * hi) + f(om * p[1]))
    scale = max(f(limit), f(hi - lo))
    return (np.array([p[0], p[1], lo, hi, scale], np.float32), np.array([lo, hi], np.float32),
            (np.asarray(adv, np.float32) / f(scale)).astype(np.float32))


# ---------------------------------------------------------------------------------------------- the actor-critic step
def ac_params(ac, dtype):
    """The actor-critic's parameters under the oracle's names ('ac.critic.model.0.weight', ...) as CPU leaves of `dtype`."""
    return {f'ac.{k}': v.detach().to('cpu', dtype).requires_grad_(not k.startswith('critic_target'))
            for k, v in ac.state_dict().items() if k != 'return_range'}


def ac_step(p, ac, features, act_idx, rewards, terminals, return_range=None, update=True):
    """a2c.py:61-149 for a one-hot actor with the switches of `ac` (an ActorCritic, read for its configuration only), in the dtype
    of the parameters p (ac_params): the two-hot critic replaces the squared error, the percentile scale divides the actor's
    advantages.  features (J, M, F), act_idx (H, M) long, rewards / terminals (J, M).  Returns ((loss_actor, loss_critic),
    tensors, new return_range or None)."""
    dt = features.dtype
    gamma, lam = ac.gamma, ac.lambda_
    twohot = ac.critic_dist == 'twohot'
    bins = ac.bins.detach().to('cpu', dt) if twohot else None
    J, M, _ = features.shape

    def values(prefix):
        out = O.mlp(p, prefix, features, 4)
        return (out, twohot_decode(out.reshape(J * M, -1), bins).reshape(J, M)) if twohot else (None, out)

    reward1, terminal0, terminal1 = rewards[1:], terminals[:-1], terminals[1:]
    with torch.no_grad():
        _, value_t = values('ac.critic_target.model')
    value0t, value1t = value_t[:-1], value_t[1:]
    advantage = -value0t + reward1 + gamma * (1.0 - terminal1) * value1t
    gae, agae = [], None
    for adv, term in zip(reversed(advantage.unbind()), reversed(terminal1.unbind())):
        agae = adv if agae is None else adv + lam * gamma * (1.0 - term) * agae
        gae.append(agae)
    gae.reverse()
    advantage_gae = torch.stack(gae)
    value_target = (advantage_gae + value0t).detach()
    weight = (1 - terminal0).log().cumsum(dim=0).exp()
    logits_c, value = values('ac.critic.model')
    if twohot:
        rows = (J - 1) * M
        lc, _, _ = twohot_compose(logits_c[:-1].reshape(rows, -1), bins, value_target.reshape(rows), weight.reshape(rows), 1.0)
        loss_critic = lc.mean()
    else:
        loss_critic = (0.5 * torch.square(value_target - value[:-1]) * weight).mean()
    scale, new_range = None, None
    if ac.return_norm == 'percentile':
        q = torch.quantile(value_target.flatten(), torch.tensor(ac.return_norm_q, dtype=dt), interpolation='linear')
        new_range = return_range.to(dt)
        if update:
            new_range = ac.return_norm_decay * new_range + (1 - ac.return_norm_decay) * q
        scale = torch.clamp(new_range[1] - new_range[0], min=ac.return_norm_limit)
    adv_actor = advantage_gae.detach() if scale is None else advantage_gae.detach() / scale
    lsm = torch.log_softmax(O.mlp(p, 'ac.actor.model', features[:-1], 4), -1)
    logp = lsm.gather(-1, act_idx[..., None])[..., 0]
    entropy = -(lsm.exp() * lsm).sum(-1)
    loss_actor = ((-logp * adv_actor - ac.entropy_weight * entropy) * weight).mean()
    tensors = dict(value=value.detach(), value_target=value_target, value_advantage=advantage.detach(),
                   value_advantage_gae=advantage_gae.detach(), value_weight=weight.detach(), scale=scale)
    return (loss_actor, loss_critic), tensors, new_range
