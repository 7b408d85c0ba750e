"""-m gpu: the continuous-actor, Gaussian-latent and IWAE entry points, and the categorical kernels' untested dispatch
branches, against fp64 CPU restatements built from torch.distributions.

Conventions (as in test_gpu_primitives.py): every output buffer starts as NaN, every accumulating output from a nonzero
random base, so an unwritten element or an overwrite-instead-of-add fails.  Gradients come from fp64 autograd of the
restatement, never from a hand-derived formula.  Tolerances are element-wise bounds derived from fp32 conditioning:
`_EPS` (fp32 machine epsilon, 2^-23) times a small operation count times the magnitude of the intermediates the kernel
rounds (computed in fp64 from the same inputs), so they stay tight where a value is well conditioned and open up only
where fp32 itself cannot do better (cancellation in x - mean, 1 - sigmoid at saturation, sums of many terms).
"""
import ctypes
import math

import pytest
import torch
import torch.distributions as D
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
_EPS = 2.0 ** -23                 # fp32 machine epsilon: ulp(v) <= _EPS * |v|
_TINY = 2.0 ** -126               # smallest normal fp32: a flushed subnormal is an error of at most this
NAN = float('nan')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(DEV)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _close(a, b, tol, what=''):
    """|a - b| <= tol element-wise (tol a tensor or a scalar); prints the worst err/tol ratio so runs can report it."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(b)
    err = (a - b).abs()
    bad = ~(err <= tol)                              # NaN in a or b fails
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f'[tol] {what}: max err {float(err.max()) if err.numel() else 0:.3e}, worst err/tol {ratio:.3f}')
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e}, ' \
                          f'worst err/tol {ratio:.3e}'


def _at(t, floats):
    """Device pointer `floats` fp32 elements into `t` (a sub-matrix view for an ld > width call)."""
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


# ------------------------------------------------------------------------------------------- continuous actors
def _cont_params(rows, A, seed):
    """Raw (m | s) rows spread over the regimes the actor kernels branch on: ordinary values; m / 5 deep in tanh
    saturation (mean = +-5); s on both sides of softplus' threshold of 20 (and exactly 20); s << 0 (std -> its minimum);
    s = +-30 (sigmoid saturated)."""
    g = _gen(seed)
    m = torch.randn(rows, A, generator=g) * 3
    s = torch.randn(rows, A, generator=g) * 2
    cat = torch.randint(0, 5, (rows, A), generator=g)
    sign = torch.where(torch.rand(rows, A, generator=g) < 0.5, -1.0, 1.0)
    m = torch.where(cat == 1, sign * (25 + 40 * torch.rand(rows, A, generator=g)), m)
    s = torch.where(cat == 2, 20 + 3 * (torch.rand(rows, A, generator=g) - 0.5), s)
    s = torch.where((cat == 2) & (torch.rand(rows, A, generator=g) < 0.2), torch.full_like(s, 20.0), s)
    s = torch.where(cat == 3, -30 - 20 * torch.rand(rows, A, generator=g), s)
    s = torch.where(cat == 4, sign * 30.0, s)
    return torch.cat([m, s], 1).float()


def _cont_dist(kind, P, A):
    """functions.py tanh_normal (kind 1) / normal_tanh (kind 2) in fp64; entropy is the base Normal's (functions.py:77)."""
    m, s = P[:, :A], P[:, A:]
    if kind == 1:
        mean, std = 5 * torch.tanh(m / 5), F.softplus(s) + 0.1
    else:
        mean, std = torch.tanh(m), torch.sigmoid(s) + 0.01
    base = D.Independent(D.Normal(mean, std, validate_args=False), 1, validate_args=False)
    dist = base if kind == 2 else D.TransformedDistribution(base, [D.TanhTransform()], validate_args=False)
    return dist, base, mean, std


CONT_SHAPES = [(1, 38), (255, 1), (256, 12), (257, 4), (2500, 6), (15 * 2500, 6)]


@pytest.mark.parametrize('rows,A', CONT_SHAPES)
@pytest.mark.parametrize('kind', [1, 2], ids=['tanh_normal', 'normal_tanh'])
def test_continuous_actor_sample_and_loss(hip, kind, rows, A):
    """dm_sample_continuous and dm_actor_loss_continuous against torch.distributions in fp64, unscaled N(0, 1) noise.
    Sampling: actions vs fp64 tanh(mean + std eps) within 4 ulp of max(|mean|, |std eps|) (the rounding of the sum, which can
    cancel, dominates; tanh only shrinks it), and exactly as many +-1 actions as the fp64 values that round to +-1, up to those
    within the bound of the rounding boundary.  Loss: fed the kernel's own fp32 actions (plus +-0.99999994), so atanh sees
    identical inputs; loss / entropy / dparams within a bound from the magnitudes of z, x, mean, log std; rows whose fp64 loss
    is non-finite (an action of exactly +-1: the reference's un-clamped atanh) must be non-finite on the kernel too."""
    P = _cont_params(rows, A, seed=rows * 7 + A + kind).to(DEV)
    eps = torch.randn(rows, A, generator=_gen(rows + 3 * A)).to(DEV)
    act = _nan(rows, A)
    hip.call('dm_sample_continuous', kind, rows, A, hip.fptr(P), hip.fptr(eps), hip.fptr(act), hip.stream())
    torch.cuda.synchronize()
    Pd, ed = P.double().cpu(), eps.double().cpu()
    _, _, mean, std = _cont_dist(kind, Pd, A)
    x = mean + std * ed
    ref = torch.tanh(x) if kind == 1 else x
    bound = 4 * _EPS * torch.maximum(mean.abs(), (std * ed).abs())
    _close(act, ref, bound, f'sample kind {kind}')
    a = act.double().cpu()
    if kind == 1:
        edge = 1 - 2.0 ** -25                     # fp64 values at or above this round to +-1 in fp32
        sat_k, sat_r = a.abs() == 1, ref.abs() >= edge
        off = sat_k != sat_r
        assert not (off & ((ref.abs() - edge).abs() > bound)).any(), \
            f'{int(off.sum())} saturation mismatches away from the rounding boundary'
        print(f'[sat] kind 1 rows {rows} A {A}: {int(sat_k.sum())} of {sat_k.numel()} actions exactly +-1 '
              f'(fp64 reference: {int(sat_r.sum())})')

    # loss on the kernel's own actions, plus the largest floats below 1 in magnitude
    actions = act.clone()
    near = torch.arange(0, rows, 3, device=DEV)
    actions[near, 0] = torch.where(near % 2 == 0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24)).float()      # +-0.99999994
    adv = _rand(rows, seed=5, scale=2.0)
    w = (0.5 + torch.rand(rows, generator=_gen(6))).to(DEV)
    ent_w, scale = 3e-3, 0.7 / rows
    loss, ent, dpar = _nan(rows), _nan(rows), _nan(rows, 2 * A)
    hip.call('dm_actor_loss_continuous', kind, rows, A, hip.fptr(P), hip.fptr(actions), hip.fptr(adv), hip.fptr(w), ent_w,
             scale, hip.fptr(loss), hip.fptr(ent), hip.fptr(dpar), hip.stream())
    torch.cuda.synchronize()
    Pg = Pd.clone().requires_grad_(True)
    dist, base, mean, std = _cont_dist(kind, Pg, A)
    y = actions.double().cpu()
    ad, wd = adv.double().cpu(), w.double().cpu()
    logp = dist.log_prob(y)
    ref_loss = (-logp * ad - ent_w * base.entropy()) * wd
    fin = torch.isfinite(ref_loss)
    assert torch.equal(~torch.isfinite(loss.cpu()), ~fin), 'non-finite loss rows differ from the fp64 restatement'
    if kind == 1:
        assert int((~fin).sum()) == int((y.abs() == 1).any(1).sum())
    (ref_loss[fin] * scale).sum().backward()
    with torch.no_grad():
        mean, std = mean.detach(), std.detach()
        xs = torch.atanh(y) if kind == 1 else y
        xs = torch.where(torch.isfinite(xs), xs, torch.zeros_like(xs))
        z = (xs - mean) / std
        dz_ = (xs.abs() + mean.abs()) / std + z.abs()                    # |error of z| / _EPS
        mag = z.abs() * dz_ + std.log().abs() + 1
        if kind == 1:
            mag = mag + 3 * xs.abs() + 2
        ent_mag = (std.log().abs() + 1.5).sum(1)
        c = 8 + A                                                        # rounding steps per term + an A-term sum
        tol_loss = c * _EPS * wd * (ad.abs() * mag.sum(1) + ent_w * ent_mag)
        _close(loss.cpu()[fin], ref_loss.detach()[fin], tol_loss[fin], f'loss kind {kind}')
        _close(ent, base.entropy().detach(), c * _EPS * ent_mag, f'entropy kind {kind}')
        m_, s_ = Pd[:, :A], Pd[:, A:]
        t = torch.tanh(m_ / 5) if kind == 1 else torch.tanh(m_)
        dmean = 1 - t * t
        sg = torch.sigmoid(s_)
        dstd = sg if kind == 1 else sg * (1 - sg)
        dstd_err = dstd if kind == 1 else sg                             # 1 - sigmoid(s) cancels in fp32 as s -> +inf
        k = 8 * _EPS * scale * wd[:, None]
        tol_m = k * ad.abs()[:, None] * (dz_ / std * dmean + z.abs() / std)
        tol_s = k * ((ad.abs()[:, None] * (z * z + 1 + 2 * z.abs() * dz_) + ent_w) / std) * dstd_err
        gm, gs = Pg.grad[:, :A], Pg.grad[:, A:]
        _close(dpar.cpu()[fin, :A], gm[fin], tol_m[fin], f'dmean kind {kind}')
        _close(dpar.cpu()[fin, A:], gs[fin], tol_s[fin], f'dstd kind {kind}')


# ------------------------------------------------------------------------------------------- Gaussian latents
def _gauss_raw(rows, S, seed):
    """(mean | raw std) rows; a fifth of the raw stds sit at exactly +-30 (sigmoid saturated in fp32)."""
    g = _gen(seed)
    mean = torch.randn(rows, S, generator=g) * 2
    raw = torch.randn(rows, S, generator=g) * 3
    sat = torch.rand(rows, S, generator=g) < 0.2
    raw = torch.where(sat, torch.where(torch.rand(rows, S, generator=g) < 0.5, -30.0, 30.0), raw)
    return torch.cat([mean, raw], 1).float()


def _diag_normal(P, S):
    """functions.py diag_normal: Independent(Normal(mean, 2 sigmoid(raw) + 0.1), 1)."""
    return D.Independent(D.Normal(P[..., :S], 2 * torch.sigmoid(P[..., S:]) + 0.1, validate_args=False), 1,
                         validate_args=False)


GAUSS_SHAPES = [(1, 200), (3, 65), (5, 1), (2500, 30), (2500, 64), (2500, 200)]


@pytest.mark.parametrize('rows,S', GAUSS_SHAPES)
def test_gaussian_latent_sample(hip, rows, S):
    """dm_sample_onehot with C = 0 (gauss_sample_kernel): z = mean + std eps written at ldo > S from parameter rows at
    ldl > 2S, the padding untouched, idx zeroed.  Bound: 4 ulp of max(|mean|, |std eps|) (the rounding of the sum)."""
    ldp, ldo = 2 * S + 3, S + 5
    par = _nan(rows, ldp)
    par[:, :2 * S] = _gauss_raw(rows, S, seed=rows + S).to(DEV)
    eps = _rand(rows, S, seed=rows * 3 + S)
    z = _nan(rows, ldo)
    idx = torch.full((rows, S), -7, dtype=torch.int32, device=DEV)
    hip.call('dm_sample_onehot', rows, S, 0, hip.fptr(par), ldp, hip.fptr(eps), None, hip.fptr(z), ldo, hip.ptr(idx),
             hip.stream())
    torch.cuda.synchronize()
    Pd, ed = par[:, :2 * S].double().cpu(), eps.double().cpu()
    d = _diag_normal(Pd, S).base_dist
    ref = d.loc + d.scale * ed
    _close(z[:, :S], ref, 4 * _EPS * torch.maximum(d.loc.abs(), (d.scale * ed).abs()), 'gaussian z')
    assert torch.isnan(z[:, S:]).all(), 'z padding written'
    assert (idx == 0).all(), 'idx not zeroed'


@pytest.mark.parametrize('rows,S', GAUSS_SHAPES)
def test_gaussian_latent_kl_balance(hip, rows, S):
    """dm_kl_balance_fwd / _bwd with C = 0: KL(post || prior) and both entropies of diag_normal, and the balanced gradients
    scale_post * KL(post || sg prior) + scale_prior * KL(sg post || prior) with scale_post != scale_prior.  Bounds: an
    (8 + S)-step rounding of the summed magnitudes of log(s2 / s1), (s1^2 + d^2) / 2 s2^2 and 1/2 for KL; per element, the
    magnitudes the gradient formula rounds, with 1 - sigmoid's fp32 cancellation at raw = +30 (an error of ~ulp * sigmoid)."""
    post = _gauss_raw(rows, S, seed=rows + 2 * S).to(DEV)
    prior = _gauss_raw(rows, S, seed=rows + 3 * S + 1).to(DEV)
    kl, ep, eq = _nan(rows), _nan(rows), _nan(rows)
    hip.call('dm_kl_balance_fwd', rows, S, 0, hip.fptr(post), hip.fptr(prior), hip.fptr(kl), hip.fptr(ep), hip.fptr(eq),
             hip.stream())
    sp, sq = 0.2 / rows * 1.3, 0.8 / rows
    dpost, dprior = _nan(rows, 2 * S), _nan(rows, 2 * S)
    hip.call('dm_kl_balance_bwd', rows, S, 0, hip.fptr(post), hip.fptr(prior), sp, sq, hip.fptr(dpost), hip.fptr(dprior),
             hip.stream())
    torch.cuda.synchronize()
    a = post.double().cpu().requires_grad_(True)
    b = prior.double().cpu().requires_grad_(True)
    c = 8 + S
    with torch.no_grad():
        A, B = a.detach(), b.detach()
        s1, s2 = 2 * torch.sigmoid(A[:, S:]) + 0.1, 2 * torch.sigmoid(B[:, S:]) + 0.1
        g1, g2 = torch.sigmoid(A[:, S:]), torch.sigmoid(B[:, S:])
        dd = A[:, :S] - B[:, :S]
        dmag = A[:, :S].abs() + B[:, :S].abs()                           # |error of d| / _EPS
        kl_mag = ((s2 / s1).log().abs() + (s1 * s1 + dd * dd + 2 * dd.abs() * dmag) / (2 * s2 * s2) + 0.5).sum(1)
        _close(kl, D.kl_divergence(_diag_normal(A, S), _diag_normal(B, S)), c * _EPS * kl_mag, 'gaussian kl')
        _close(ep, _diag_normal(A, S).entropy(), c * _EPS * (s1.log().abs() + 1.5).sum(1), 'gaussian entropy post')
        _close(eq, _diag_normal(B, S).entropy(), c * _EPS * (s2.log().abs() + 1.5).sum(1), 'gaussian entropy prior')
    loss = sp * D.kl_divergence(_diag_normal(a, S), _diag_normal(b.detach(), S)) + \
        sq * D.kl_divergence(_diag_normal(a.detach(), S), _diag_normal(b, S))
    loss.sum().backward()
    k = 8 * _EPS
    _close(dpost[:, :S], a.grad[:, :S], k * sp * dmag / (s2 * s2), 'gaussian dpost mean')
    _close(dpost[:, S:], a.grad[:, S:], k * sp * (s1 / (s2 * s2) + 1 / s1) * 2 * g1, 'gaussian dpost raw')
    _close(dprior[:, :S], b.grad[:, :S], k * sq * dmag / (s2 * s2), 'gaussian dprior mean')
    _close(dprior[:, S:], b.grad[:, S:], k * sq * (1 / s2 + (s1 * s1 + dd * dd + 2 * dd.abs() * dmag) / s2 ** 3) * 2 * g2,
           'gaussian dprior raw')


# ------------------------------------------------------------------------------------------- categorical dispatch gaps
def _ref_sample(logits, u):
    """The shared inverse-CDF rule in fp64: idx = #{k: cdf_k <= u * cdf_last}, and each draw's distance to a CDF boundary."""
    p = torch.softmax(logits.double().cpu(), -1)
    cdf = torch.cumsum(p, -1)
    target = u.double().cpu().unsqueeze(-1) * cdf[..., -1:]
    idx = (cdf <= target).sum(-1).clamp(max=logits.shape[-1] - 1)
    margin = (cdf - target).abs().min(-1).values
    return idx, margin


@pytest.mark.parametrize('rows,groups,C,pad', [(300, 3, 16, 0), (77, 2, 64, 0), (50, 4, 65, 0), (9, 5, 100, 0), (130, 3, 32, 1)],
                         ids=['C16', 'C64', 'C65', 'C100', 'C32-odd-ld'])
def test_sample_onehot_dispatch(hip, rows, groups, C, pad):
    """dm_sample_onehot on the LPG = 16 / 64 wave kernels, the scalar C > 64 sampler, and C = 32 with an odd ldl (which must
    leave the float4 lane-per-group kernel for the wave kernel): indices equal the fp64 rule except within 1e-5 of a CDF
    boundary (the existing margin rule), the one-hot matches the index, row padding stays NaN, and forced indices pass through
    exactly."""
    width = groups * C
    ldl, ldo = width + pad, width + 3
    logits_full = _nan(rows, ldl)
    logits_full[:, :width] = _rand(rows, width, seed=C, scale=2.0)
    u = torch.rand(rows, groups, generator=_gen(C + 1)).to(DEV)
    onehot = _nan(rows, ldo)
    idx = torch.full((rows, groups), -7, dtype=torch.int32, device=DEV)
    hip.call('dm_sample_onehot', rows, groups, C, hip.fptr(logits_full), ldl, hip.fptr(u), None, hip.fptr(onehot), ldo,
             hip.ptr(idx), hip.stream())
    torch.cuda.synchronize()
    ref, margin = _ref_sample(logits_full[:, :width].reshape(rows, groups, C), u)
    got = idx.cpu().long()
    diff = got != ref
    assert (margin[diff] < 1e-5).all(), f'{int(diff.sum())} index mismatches away from CDF boundaries'
    assert torch.equal(onehot[:, :width].cpu().reshape(rows, groups, C), F.one_hot(got, C).float())
    assert torch.isnan(onehot[:, width:]).all(), 'one-hot padding written'
    forced = torch.randint(0, C, (rows, groups), generator=_gen(C + 2)).int().to(DEV)
    onehot.fill_(NAN)
    idx.fill_(-7)
    hip.call('dm_sample_onehot', rows, groups, C, hip.fptr(logits_full), ldl, None, hip.ptr(forced), hip.fptr(onehot), ldo,
             hip.ptr(idx), hip.stream())
    torch.cuda.synchronize()
    assert torch.equal(idx, forced)
    assert torch.equal(onehot[:, :width].cpu().reshape(rows, groups, C), F.one_hot(forced.cpu().long(), C).float())
    assert torch.isnan(onehot[:, width:]).all()


@pytest.mark.parametrize('C', [8, 16, 33, 64])
@pytest.mark.parametrize('accum', [0, 1])
def test_st_softmax_bwd_dispatch(hip, C, accum):
    """dm_st_softmax_bwd on every LPG (8, 16, 64, and 33 in the 64-lane kernel), with and without accumulation, at leading
    dimensions past the row width: dlogits (+)= d/dlogits sum(softmax(x) * dz) by fp64 autograd.  Bound: (8 + C) roundings of
    p (|g| + sum_j p_j |g_j|) (the butterfly sums), plus one of the accumulated base."""
    rows, groups = 37, 5
    width, ld = groups * C, groups * C + 5
    logits = _rand(rows, ld, seed=C, scale=2.0)
    dz = _rand(rows, ld, seed=C + 1)
    base = _rand(rows, ld, seed=C + 2) if accum else _nan(rows, ld)
    out = base.clone()
    hip.call('dm_st_softmax_bwd', rows, groups, C, hip.fptr(logits), ld, hip.fptr(dz), ld, hip.fptr(out), ld, accum,
             hip.stream())
    torch.cuda.synchronize()
    x = logits[:, :width].double().cpu().reshape(rows, groups, C).requires_grad_(True)
    g = dz[:, :width].double().cpu().reshape(rows, groups, C)
    p = torch.softmax(x, -1)
    (p * g).sum().backward()
    want = x.grad.reshape(rows, width)
    pd = p.detach()
    mag = (pd * (g.abs() + (pd * g.abs()).sum(-1, keepdim=True))).reshape(rows, width)
    tol = (8 + C) * _EPS * mag
    if accum:
        want = want + base[:, :width].double().cpu()
        tol = tol + _EPS * base[:, :width].double().cpu().abs()
    _close(out[:, :width], want, tol, f'st bwd C={C} accum={accum}')
    assert torch.equal(out[:, width:].isnan(), base[:, width:].isnan()) and \
        torch.equal(out[:, width:].nan_to_num(), base[:, width:].nan_to_num()), 'padding columns changed'


def _cat_mags(a, b):
    """Per (row, group, k): p, q, log p, log q and the fp32 error scale of log p and log q (|x_k| + |lse|)."""
    la, lb = a.logsumexp(-1, keepdim=True), b.logsumexp(-1, keepdim=True)
    lp, lq = a - la, b - lb
    ea, eb = a.abs() + la.abs(), b.abs() + lb.abs()
    return lp.exp(), lq.exp(), lp, lq, ea, eb


@pytest.mark.parametrize('rows,S,C', [(7, 1, 2), (5, 65, 8), (3, 130, 33), (9, 32, 64), (1001, 65, 8)])
def test_kl_balance_categorical_shapes(hip, rows, S, C):
    """dm_kl_balance_fwd / _bwd at group counts that make the 64-lane group loop run once, twice and three times, class counts
    2 ... 64, and row counts that are not a multiple of the four rows per block: KL, both entropies and the balanced gradients
    against OneHotCategorical in fp64.  Bounds: (8 + C + S) roundings of sum p |log p - log q| with the log-softmax error
    scale; per element the same scales for p ((lp - lq) - KL_group) and q - p."""
    post = _rand(rows, S * C, seed=S + C, scale=2.0)
    prior = _rand(rows, S * C, seed=S + C + 1, scale=2.0)
    kl, ep, eq = _nan(rows), _nan(rows), _nan(rows)
    hip.call('dm_kl_balance_fwd', rows, S, C, hip.fptr(post), hip.fptr(prior), hip.fptr(kl), hip.fptr(ep), hip.fptr(eq),
             hip.stream())
    sp, sq = 0.2 / rows, 0.8 / rows * 1.1
    dpost, dprior = _nan(rows, S * C), _nan(rows, S * C)
    hip.call('dm_kl_balance_bwd', rows, S, C, hip.fptr(post), hip.fptr(prior), sp, sq, hip.fptr(dpost), hip.fptr(dprior),
             hip.stream())
    torch.cuda.synchronize()

    def dist(x):
        return D.Independent(D.OneHotCategorical(logits=x.reshape(rows, S, C), validate_args=False), 1, validate_args=False)
    a = post.double().cpu().requires_grad_(True)
    b = prior.double().cpu().requires_grad_(True)
    with torch.no_grad():
        p, q, lp, lq, ea, eb = _cat_mags(a.reshape(rows, S, C), b.reshape(rows, S, C))
        kl_g = (p * (lp - lq)).sum(-1, keepdim=True)
        gmag = p * (ea + eb) * (1 + (lp - lq).abs())
        c = 8 + C + S
        _close(kl, D.kl_divergence(dist(a), dist(b)), c * _EPS * gmag.sum((1, 2)), 'kl')
        _close(ep, dist(a).entropy(), c * _EPS * (p * ea * (1 + lp.abs())).sum((1, 2)), 'entropy post')
        _close(eq, dist(b).entropy(), c * _EPS * (q * eb * (1 + lq.abs())).sum((1, 2)), 'entropy prior')
    loss = sp * D.kl_divergence(dist(a), dist(b.detach())) + sq * D.kl_divergence(dist(a.detach()), dist(b))
    loss.sum().backward()
    tol_p = (8 + C) * _EPS * sp * (p * (ea + eb) * (1 + (lp - lq).abs() + kl_g.abs()) + p * gmag.sum(-1, keepdim=True))
    tol_q = 8 * _EPS * sq * (q * eb + p * ea)
    _close(dpost, a.grad, tol_p.reshape(rows, -1), 'dpost')
    _close(dprior, b.grad, tol_q.reshape(rows, -1), 'dprior')


# ------------------------------------------------------------------------------------------- IWAE
@pytest.mark.parametrize('rows,S,C', [(7, 1, 33), (61, 32, 32), (5, 65, 64), (13, 32, 8), (16200, 65, 8)])
@pytest.mark.parametrize('weighted', [False, True], ids=['unweighted', 'row_w'])
def test_kl_sampled(hip, rows, S, C, weighted):
    """dm_kl_sampled_fwd / _bwd (IWAE's sampled KL, dreamer.py:340-343): out = log q(z) - log p(z) of the drawn one-hot under
    OneHotCategorical, summed over groups; gradients of sum(scale * row_w * out) by fp64 autograd (no gradient through z:
    log_prob goes through the index).  16200 x 65 groups wrap the 4096-block grid-stride loop.  Bounds: (8 + S) roundings of
    sum |log-softmax| error scales; per element 8 roundings of |w| (1[k = idx] + p (1 + |x_k| + |lse|))."""
    post = _rand(rows, S * C, seed=S * C, scale=2.0)
    prior = _rand(rows, S * C, seed=S * C + 1, scale=2.0)
    idx = torch.randint(0, C, (rows, S), generator=_gen(C)).int().to(DEV)
    row_w = (0.25 + torch.rand(rows, generator=_gen(S))).to(DEV) if weighted else None
    scale = 0.37
    out = _nan(rows)
    hip.call('dm_kl_sampled_fwd', rows, S, C, hip.fptr(post), hip.fptr(prior), hip.ptr(idx), hip.fptr(out), hip.stream())
    dpost, dprior = _nan(rows, S * C), _nan(rows, S * C)
    hip.call('dm_kl_sampled_bwd', rows, S, C, hip.fptr(post), hip.fptr(prior), hip.ptr(idx), scale, hip.fptr(row_w),
             hip.fptr(dpost), hip.fptr(dprior), hip.stream())
    torch.cuda.synchronize()
    a = post.double().cpu().requires_grad_(True)
    b = prior.double().cpu().requires_grad_(True)
    hot = F.one_hot(idx.long().cpu(), C).double()

    def dist(x):
        return D.Independent(D.OneHotCategorical(logits=x.reshape(rows, S, C), validate_args=False), 1, validate_args=False)
    ref = dist(a).log_prob(hot) - dist(b).log_prob(hot)
    wd = scale * (row_w.double().cpu() if weighted else torch.ones(rows, dtype=torch.float64))
    (wd * ref).sum().backward()
    with torch.no_grad():
        p, q, lp, lq, ea, eb = _cat_mags(a.reshape(rows, S, C), b.reshape(rows, S, C))
        _close(out, ref, (8 + S) * _EPS * ((hot * (ea + eb)).sum(-1) + 1).sum(-1), 'kl sampled')
        w3 = wd.abs()[:, None, None]
        _close(dpost, a.grad, (8 * _EPS * w3 * (hot + p * (1 + ea))).reshape(rows, -1), 'kl sampled dpost')
        _close(dprior, b.grad, (8 * _EPS * w3 * (hot + q * (1 + eb))).reshape(rows, -1), 'kl sampled dprior')


@pytest.mark.parametrize('rows,S', [(7, 1), (5, 30), (61, 65), (2500, 200), (5000, 210)])
@pytest.mark.parametrize('weighted', [False, True], ids=['unweighted', 'row_w'])
def test_kl_sampled_gauss(hip, rows, S, weighted):
    """dm_kl_sampled_gauss_fwd / _bwd (IWAE with Gaussian latents): out = log q(z) - log p(z) under diag_normal with z read
    from inside a feature matrix at ldz > S (models.py reads it in place), gradients of sum(scale * row_w * out) by fp64
    autograd with respect to post, prior AND z, the z gradient ADDED to a nonzero dz base at lddz > S (padding untouched).
    5000 x 210 wraps the 4096-block grid-stride loop.  Bounds from the magnitudes of (z - m) / s, log s and the 1 - sigmoid
    cancellation at raw = +30."""
    Dd = 37                                           # feature columns in front of z (h), as in feat = [h | z]
    ldz, lddz = Dd + S + 3, Dd + S + 2
    post = _gauss_raw(rows, S, seed=rows + S).to(DEV)
    prior = _gauss_raw(rows, S, seed=rows + S + 1).to(DEV)
    feat = _rand(rows, ldz, seed=S, scale=2.0)
    dzbuf = _rand(rows, lddz, seed=S + 1)
    dz0 = dzbuf.clone()
    row_w = (0.25 + torch.rand(rows, generator=_gen(S))).to(DEV) if weighted else None
    scale = 0.37
    out = _nan(rows)
    hip.call('dm_kl_sampled_gauss_fwd', rows, S, hip.fptr(post), hip.fptr(prior), _at(feat, Dd), ldz, hip.fptr(out),
             hip.stream())
    dpost, dprior = _nan(rows, 2 * S), _nan(rows, 2 * S)
    hip.call('dm_kl_sampled_gauss_bwd', rows, S, hip.fptr(post), hip.fptr(prior), _at(feat, Dd), ldz, scale, hip.fptr(row_w),
             hip.fptr(dpost), hip.fptr(dprior), _at(dzbuf, Dd), lddz, hip.stream())
    torch.cuda.synchronize()
    a = post.double().cpu().requires_grad_(True)
    b = prior.double().cpu().requires_grad_(True)
    zz = feat[:, Dd:Dd + S].double().cpu().requires_grad_(True)
    ref = _diag_normal(a, S).log_prob(zz) - _diag_normal(b, S).log_prob(zz)
    wd = scale * (row_w.double().cpu() if weighted else torch.ones(rows, dtype=torch.float64))
    (wd * ref).sum().backward()
    with torch.no_grad():
        A, B, Z = a.detach(), b.detach(), zz.detach()
        g1, g2 = torch.sigmoid(A[:, S:]), torch.sigmoid(B[:, S:])
        s1, s2 = 2 * g1 + 0.1, 2 * g2 + 0.1
        e1, e2 = Z - A[:, :S], Z - B[:, :S]
        m1, m2 = Z.abs() + A[:, :S].abs(), Z.abs() + B[:, :S].abs()          # |error of e| / _EPS
        mag = s1.log().abs() + s2.log().abs() + (e1.abs() / s1) * (m1 / s1 + e1.abs() / s1) + \
            (e2.abs() / s2) * (m2 / s2 + e2.abs() / s2) + 1
        _close(out, ref, (8 + S) * _EPS * mag.sum(1), 'gauss kl sampled')
        k = 8 * _EPS * wd.abs()[:, None]
        _close(dpost[:, :S], a.grad[:, :S], k * m1 / s1 ** 2, 'gauss kl sampled dpost mean')
        _close(dpost[:, S:], a.grad[:, S:], k * (1 / s1 + (e1 * e1 + 2 * e1.abs() * m1) / s1 ** 3) * 2 * g1,
               'gauss kl sampled dpost raw')
        _close(dprior[:, :S], b.grad[:, :S], k * m2 / s2 ** 2, 'gauss kl sampled dprior mean')
        _close(dprior[:, S:], b.grad[:, S:], k * (1 / s2 + (e2 * e2 + 2 * e2.abs() * m2) / s2 ** 3) * 2 * g2,
               'gauss kl sampled dprior raw')
        base = dz0[:, Dd:Dd + S].double().cpu()
        _close(dzbuf[:, Dd:Dd + S], base + zz.grad, k * (m1 / s1 ** 2 + m2 / s2 ** 2) + _EPS * base.abs(), 'gauss kl sampled dz')
    assert torch.equal(dzbuf[:, :Dd], dz0[:, :Dd]) and torch.equal(dzbuf[:, Dd + S:], dz0[:, Dd + S:]), 'dz outside z changed'


def _reduce_inputs(TB, I, W, special, seed):
    x = torch.randn(TB, I, W, generator=_gen(seed)) * 3
    if special == 'equal':                            # every sample's loss equal: weights exactly 1/I
        x = x[:, :1].expand(TB, I, W).contiguous()
    elif special == 'spread':                         # per-sample losses > 100 apart: one weight ~ 1, the rest underflow
        x = x + 120.0 * torch.arange(I, dtype=torch.float32)[None, :, None] * torch.where(
            torch.rand(TB, 1, 1, generator=_gen(seed + 1)) < 0.5, 1.0, -1.0)
    return x.float()


REDUCE_CASES = [
    # (mode, TB, I, W, special)
    (0, 5, 1, 7, None), (0, 33, 3, 1536, None), (0, 700, 2, 1536, None), (2, 3, 16, 7, None), (2, 257, 1, 1, None),
    (2, 700, 3, 1536, None),
    (1, 1, 1, 1, None), (1, 257, 16, 1, None), (1, 65, 3, 1, 'equal'), (1, 260, 2, 1, 'spread'), (1, 255, 16, 1, 'spread'),
    (1, 1100000, 2, 1, None),
]


@pytest.mark.parametrize('mode,TB,I,W,special', REDUCE_CASES)
def test_reduce_i(hip, mode, TB, I, W, special):
    """dm_reduce_i, x (TB, I, W) -> (TB, W): mode 0 mean, mode 2 sum, mode 1 -logavgexp_i(-x) (functions.py:97-102) with the
    importance weights w_out = softmax_i(-x) that sum to 1 per row; equal inputs (weights 1/I), losses 100+ apart (one weight
    ~ 1, the others flush or underflow), and TB * W past 4096 x 256 so the grid-stride loop wraps.  Bounds: (8 + I) roundings
    of sum_i |x_i| (mode 0 / 2) or of |max| + |log sum| + log I (mode 1); weights (8 + I) roundings of w (1 + |x_i - max|),
    the second term the rounding of exp's argument, plus one smallest normal (a subnormal weight may flush)."""
    x = _reduce_inputs(TB, I, W, special, seed=TB + I + W).to(DEV)
    out = _nan(TB, W)
    w_out = _nan(TB, I) if mode == 1 else None
    hip.call('dm_reduce_i', TB, I, W, hip.fptr(x), mode, hip.fptr(out), hip.fptr(w_out), hip.stream())
    torch.cuda.synchronize()
    xd = x.double().cpu()
    c = (8 + I) * _EPS
    if mode == 1:
        neg = -xd[:, :, 0]
        ref = -(torch.logsumexp(neg, 1) - math.log(I))
        mx = neg.max(1).values
        _close(out[:, 0], ref, c * (mx.abs() + (torch.logsumexp(neg, 1) - mx).abs() + math.log(I) + 1), 'reduce_i mode 1')
        wref = torch.softmax(neg, 1)
        # exp(-x_i - max) carries the rounding of its argument: a relative error of ~ulp * |x_i - max| on top of the sum's
        _close(w_out, wref, c * wref * (1 + (neg - mx[:, None]).abs()) + _TINY, 'reduce_i weights')
        _close(w_out.double().sum(1), torch.ones(TB, dtype=torch.float64), c, 'reduce_i weights sum')
        if special == 'equal':      # exp(0) = 1 and a sum of I ones are exact: every weight is RN(1/I)
            assert torch.equal(w_out.cpu(), torch.full((TB, I), 1.0 / I, dtype=torch.float32))
    else:
        ref = xd.mean(1) if mode == 0 else xd.sum(1)
        _close(out, ref, c * xd.abs().sum(1) / (I if mode == 0 else 1), f'reduce_i mode {mode}')


@pytest.mark.parametrize('n', [1, 257, 600001])
def test_combine_rows(hip, n):
    """dm_combine_rows, out = sum_j w_j x_j for every count 1 ... 8; n = 600001 wraps the 2048-block grid-stride loop.
    Bound: (8 + count) roundings of sum_j |w_j x_j|."""
    xs = [_rand(n, seed=10 + j) for j in range(8)]
    ws = [0.5 + 0.3 * j * (-1) ** j for j in range(8)]
    for count in range(1, 9):
        out = _nan(n)
        ptrs = (ctypes.c_void_p * count)(*[x.data_ptr() for x in xs[:count]])
        wts = (ctypes.c_float * count)(*ws[:count])
        hip.call('dm_combine_rows', count, n, ptrs, wts, hip.fptr(out), hip.stream())
        torch.cuda.synchronize()
        terms = torch.stack([float(ctypes.c_float(w).value) * x.double().cpu() for w, x in zip(ws, xs[:count])])
        _close(out, terms.sum(0), (8 + count) * _EPS * terms.abs().sum(0), f'combine_rows count {count}')


@pytest.mark.parametrize('rows,n,ldx', [(1, 1, 1), (7, 5, 9), (3000, 400, 403), (1100000, 1, 3)])
def test_scale_rows(hip, rows, n, ldx):
    """dm_scale_rows, x[r, :n] *= w[r] * scale at ldx > n; 1.1 M one-column rows exceed the 4096-block cap.  The padding
    columns are untouched.  Bound: two roundings (w * scale, then the product)."""
    x = _rand(rows, ldx, seed=n)
    x0 = x.clone()
    w = _rand(rows, seed=n + 1)
    scale = 0.3
    hip.call('dm_scale_rows', rows, n, hip.fptr(x), ldx, hip.fptr(w), scale, hip.stream())
    torch.cuda.synchronize()
    ref = x0[:, :n].double().cpu() * w.double().cpu()[:, None] * float(ctypes.c_float(scale).value)
    _close(x[:, :n], ref, 4 * _EPS * ref.abs(), 'scale_rows')
    assert torch.equal(x[:, n:], x0[:, n:]), 'padding columns changed'


def test_combine(hip):
    """dm_combine, out[0] = sum_i w_i x_i for every count 1 ... 16.  Bound: (8 + count) roundings of sum |w_i x_i|."""
    x = _rand(16, seed=3, scale=5.0)
    ws = [(-1) ** i * (0.1 + 0.37 * i) for i in range(16)]
    for count in range(1, 17):
        out = _nan(1)
        hip.call('dm_combine', count, hip.fptr(x), (ctypes.c_float * count)(*ws[:count]), hip.fptr(out), hip.stream())
        torch.cuda.synchronize()
        terms = torch.tensor([float(ctypes.c_float(w).value) for w in ws[:count]], dtype=torch.float64) * x[:count].double().cpu()
        _close(out, terms.sum().reshape(1), (8 + count) * _EPS * terms.abs().sum(), f'combine count {count}')


# ------------------------------------------------------------------------------------------- empty and refused calls
def test_empty_calls_leave_outputs_untouched(hip):
    """rows = 0 on every entry point above returns OK and writes nothing (every output a NaN sentinel, idx -7)."""
    buf = _nan(4096)
    keep = torch.full((256,), -7, dtype=torch.int32, device=DEV)
    src = _rand(4096, seed=1)
    idx = torch.zeros(256, dtype=torch.int32, device=DEV)
    f, s, i = hip.fptr(buf), hip.stream(), hip.ptr(keep)
    q = hip.fptr(src)
    hip.call('dm_sample_continuous', 1, 0, 4, q, q, f, s)
    hip.call('dm_actor_loss_continuous', 2, 0, 4, q, q, q, q, 1e-3, 1.0, f, f, f, s)
    hip.call('dm_sample_onehot', 0, 8, 0, q, 16, q, None, f, 8, i, s)
    hip.call('dm_sample_onehot', 0, 8, 16, q, 128, q, None, f, 128, i, s)
    hip.call('dm_kl_balance_fwd', 0, 8, 0, q, q, f, f, f, s)
    hip.call('dm_kl_balance_bwd', 0, 8, 0, q, q, 1.0, 1.0, f, f, s)
    hip.call('dm_kl_balance_fwd', 0, 8, 8, q, q, f, f, f, s)
    hip.call('dm_kl_balance_bwd', 0, 8, 8, q, q, 1.0, 1.0, f, f, s)
    hip.call('dm_st_softmax_bwd', 0, 8, 8, q, 64, q, 64, f, 64, 0, s)
    hip.call('dm_kl_sampled_fwd', 0, 8, 8, q, q, hip.ptr(idx), f, s)
    hip.call('dm_kl_sampled_bwd', 0, 8, 8, q, q, hip.ptr(idx), 1.0, None, f, f, s)
    hip.call('dm_kl_sampled_gauss_fwd', 0, 8, q, q, q, 8, f, s)
    hip.call('dm_kl_sampled_gauss_bwd', 0, 8, q, q, q, 8, 1.0, None, f, f, f, 8, s)
    for mode in (0, 1, 2):
        hip.call('dm_reduce_i', 0, 3, 1, q, mode, f, f if mode == 1 else None, s)
    ptrs = (ctypes.c_void_p * 2)(src.data_ptr(), src.data_ptr())
    hip.call('dm_combine_rows', 2, 0, ptrs, (ctypes.c_float * 2)(1.0, 2.0), f, s)
    scaled = src.clone()
    hip.call('dm_scale_rows', 0, 4, hip.fptr(scaled), 4, q, 2.0, s)
    torch.cuda.synchronize()
    assert torch.equal(scaled, src), 'dm_scale_rows with rows = 0 changed x'
    assert torch.isnan(buf).all(), f'{int((~torch.isnan(buf)).sum())} sentinel elements written by an empty call'
    assert (keep == -7).all(), 'idx written by an empty call'


def test_out_of_range_arguments_are_refused(hip):
    """Arguments outside what a kernel handles are refused on the host (DreamerHipError) before any launch: nothing written."""
    buf = _nan(4096)
    src = _rand(4096, seed=2)
    f, q, s = hip.fptr(buf), hip.fptr(src), hip.stream()
    refused = [
        ('dm_reduce_i', 4, 3, 1, q, 3, f, None, s),              # mode 3
        ('dm_reduce_i', 4, 3, 2, q, 1, f, f, s),                 # mode 1 needs W = 1
        ('dm_combine_rows', 9, 16, (ctypes.c_void_p * 9)(*[src.data_ptr()] * 9), (ctypes.c_float * 9)(*[1.0] * 9), f, s),
        ('dm_sample_continuous', 0, 4, 4, q, q, f, s),           # kind 0 is the one-hot actor
        ('dm_actor_loss_continuous', 0, 4, 4, q, q, q, q, 1e-3, 1.0, f, f, f, s),
        ('dm_st_softmax_bwd', 4, 2, 65, q, 130, q, 130, f, 130, 0, s),      # C > 64 has no kernel
    ]
    for name, *args in refused:
        with pytest.raises(hip.DreamerHipError):
            hip.call(name, *args)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all(), 'a refused call wrote its output'
