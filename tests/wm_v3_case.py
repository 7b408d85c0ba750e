"""Restatements of the world model's free bits and symlog two-hot reward head for the tests, written with torch in
whatever dtype they are handed - float64 is the reference - and built from the oracle's functions (conv_encoder, cell_forward with
forced_idx, prior_head, mlp, zdistr, conv_decoder) and the two-hot rule of tests/twohot_case.py.  Pure CPU; nothing here touches
the library."""
import numpy as np
import torch
import torch.distributions as D

from oracle import dreamer_oracle as O
from tests import twohot_case as TC


# ---------------------------------------------------------------------------------------------- free bits
def row_kl(post, prior, S, C):
    """KL(post || prior) per row, summed over the S groups: post / prior (rows, S C) logits, or (rows, 2 S) Gaussian parameters
    (mean | raw std) for C = 0, in their own dtype."""
    conf = O.make_conf(stoch_dim=S, stoch_discrete=C)
    if C:      # (zdistr casts categorical logits to fp32: the same distribution written out in the inputs' dtype)
        dist = lambda x: D.Independent(D.OneHotCategorical(logits=x.reshape(-1, S, C), validate_args=False), 1)
        return D.kl_divergence(dist(post), dist(prior))
    return D.kl_divergence(O.zdistr(conf, post), O.zdistr(conf, prior))


def mid_free(kl64):
    """(free, gap): the midpoint of the widest gap between neighbouring order statistics of the row KLs in the central third, and
    that gap.  Fewer than 3 rows: the central third is the whole list; one row: (kl / 2, kl)."""
    s = np.sort(np.asarray(kl64, np.float64).reshape(-1))
    n = len(s)
    if n == 1:
        return float(s[0] / 2), float(s[0])
    lo, hi = (n // 3, n - n // 3) if n >= 3 else (0, n)
    if hi - lo < 2:
        lo, hi = max(lo - 1, 0), min(hi + 1, n)
    d = np.diff(s[lo:hi])
    i = int(np.argmax(d))
    return float(0.5 * (s[lo + i] + s[lo + i + 1])), float(d[i])


def assert_gap(free, gap):
    """The condition under which fp32 and float64 agree on which rows are closed (a condition of the test, not a tolerance)."""
    assert gap > 1e-3 * max(1.0, free), f'the gap {gap:.3e} around free={free:.6g} is too narrow: choose another seed'


def free_bits(kl, free):
    """(kl_clip, closed) of the rule: max(free, kl) and 1.0 where kl <= free."""
    return torch.clamp(kl, min=free), (kl <= free).to(kl.dtype)


# ---------------------------------------------------------------------------------------------- the two-hot head
def twohot_encode(target, bins):
    """(rows, K) two-hot weights of symlog(target) on `bins`."""
    k, w_lo, w_hi = TC.twohot_rows(target, bins)
    y = torch.zeros(target.numel(), bins.numel(), dtype=bins.dtype)
    return y.scatter_(-1, k[:, None], w_lo[:, None]).scatter_add_(-1, (k + 1)[:, None], w_hi[:, None])


def twohot_head(logits, bins, target, I=1, scale=1.0):
    """dm_twohot_head_loss restated: logits (rows, K), target (rows / I,); returns (loss, dlogits, mean)."""
    t = target.repeat_interleave(I) if I > 1 else target
    return TC.twohot_compose(logits, bins, t, torch.ones_like(t), scale)


def head_output_layer(K, seed=0):
    """Closed-form values for the K-wide output layer of a two-hot head (a zero layer leaves nothing to compare): a tenth of the
    xavier range, as tests/test_gpu_twohot_critic.py fills the critic's."""
    rs = np.random.RandomState(seed + 199)
    lim = 0.1 * np.sqrt(6.0 / (400 + K))
    return (torch.tensor(rs.uniform(-lim, lim, (K, 400)), dtype=torch.float32),
            torch.tensor(0.05 * rs.uniform(-1, 1, K), dtype=torch.float32))


# ---------------------------------------------------------------------------------------------- the world-model step
def wm_step(p, conf, obs, in_state, forced_idx, kl_free=0.0, reward_bins=None, u_post=None, iwae_samples=1):
    """WorldModel.training_step on the convolution path (oracle.wm_training_step's order) with the two switches, in the dtype of
    the parameters p: kl_free > 0 clips both halves of the balanced KL at kl_free per row (I = 1 only); reward_bins (a (K,)
    tensor) replaces the Normal reward head by the two-hot head over those bins.  forced_idx (T, B I, S): the posterior indices
    (categorical latents); Gaussian latents take u_post (T, B I, S) instead.  Returns (loss_model, metrics, tensors)."""
    I = int(iwae_samples)
    T, B = obs['action'].shape[:2]
    dt = obs['image'].dtype
    embed = O.conv_encoder(p, obs['image'])
    h, z = in_state
    expand = lambda x: x.unsqueeze(2).expand(T, B, I, x.shape[-1]).reshape(T, B * I, x.shape[-1])
    embeds, actions = expand(embed), expand(obs['action'])
    reset_masks = expand((~obs['reset']).unsqueeze(-1).to(dt))
    posts, hs, zs = [], [], []
    for t in range(T):
        post, h, z, _ = O.cell_forward(p, conf, embeds[t], actions[t], reset_masks[t], h, z, None if u_post is None else u_post[t],
                                       None if forced_idx is None else forced_idx[t])
        z = z.to(dt)
        posts.append(post); hs.append(h); zs.append(z)
    posts, hs, zs = torch.stack(posts), torch.stack(hs), torch.stack(zs)
    priors = O.prior_head(p, hs)
    feat = torch.cat((hs, zs), -1).reshape(T, B, I, -1)
    decoded = O.conv_decoder(p, feat)
    loss_image = 0.5 * torch.square(decoded - obs['image'].unsqueeze(2)).sum(dim=[-1, -2, -3])
    out = O.mlp(p, 'wm.decoder.reward.model.model', feat, conf.reward_decoder_layers)
    if reward_bins is None:
        std = 0.3989422804
        loss_reward = -D.Normal(out, torch.ones_like(out) * std).log_prob(obs['reward'].unsqueeze(2)) * std ** 2
        reward_mean = out
    else:
        lr, _, mean = twohot_head(out.reshape(T * B * I, -1), reward_bins, obs['reward'].reshape(-1), I)
        loss_reward, reward_mean = lr.reshape(T, B, I), mean.reshape(T, B, I)
    tl = O.mlp(p, 'wm.decoder.terminal.model.model', feat, conf.terminal_decoder_layers)
    loss_terminal = -D.Bernoulli(logits=tl).log_prob(obs['terminal'].unsqueeze(2))
    S, C = conf.stoch_dim, conf.stoch_discrete
    kl = lambda a, b: row_kl(a.reshape(T * B * I, -1), b.reshape(T * B * I, -1), S, C).reshape(T, B, I)
    loss_kl_exact = kl(posts, priors)
    if I > 1:
        assert not kl_free, 'free bits clip the exact KL: I = 1'
        dpost, dprior = (_dist(x.reshape(T, B, I, -1), S, C) for x in (posts, priors))
        zs_tbi = zs.reshape(dpost.batch_shape + dpost.event_shape)
        loss_kl = dpost.log_prob(zs_tbi) - dprior.log_prob(zs_tbi)
    elif conf.kl_balance == 0.5:      # dreamer.py:241: the exact KL itself, its gradient into both sides unweighted
        loss_kl = torch.clamp(loss_kl_exact, min=kl_free) if kl_free else loss_kl_exact
    else:
        postgrad, priograd = kl(posts, priors.detach()), kl(posts.detach(), priors)
        if kl_free:
            postgrad, priograd = torch.clamp(postgrad, min=kl_free), torch.clamp(priograd, min=kl_free)
        loss_kl = (1 - conf.kl_balance) * postgrad + conf.kl_balance * priograd
    loss_tbi = conf.kl_weight * loss_kl + conf.image_weight * loss_image + conf.reward_weight * loss_reward + \
        conf.terminal_weight * loss_terminal
    loss = (-O.logavgexp(-loss_tbi, 2)).mean()
    with torch.no_grad():
        lae = lambda x: (-O.logavgexp(-x, 2)).detach()
        tensors = dict(loss_kl=lae(loss_kl_exact), loss_image=lae(loss_image), loss_reward=lae(loss_reward),
                       reward_rec=reward_mean.mean(2).detach(), loss_terminal=lae(loss_terminal))
        if kl_free:
            tensors['loss_kl_clip'], closed = free_bits(tensors['loss_kl'], kl_free)
        metrics = {k: tensors[k].mean() for k in tensors if k.startswith('loss_')}
        metrics['loss_model'] = loss.detach()
        if kl_free:
            metrics['kl_free_frac'] = closed.mean()
    return loss, metrics, tensors


def _dist(x, S, C):
    if C:
        return D.Independent(D.OneHotCategorical(logits=x.reshape(x.shape[:-1] + (S, C)), validate_args=False), 1)
    mean, std = O.gaussian_params(x)
    return D.Independent(D.Normal(mean, std), 1)
