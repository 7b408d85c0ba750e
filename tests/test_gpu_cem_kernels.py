"""-m gpu: the planning kernels of csrc/cem.hip - dm_cem_draw and dm_cem_update against host restatements.

Every tolerance is a first-order rounding bound with u = 2^-24, derived from the operation order the kernels state in the comment at
the head of csrc/cem.hip; _close prints err / tol.  M = B J rows, row m = b J + j; (Hp, M, ...) arrays are time-major."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
U_MAX = np.float32(1.0 - 2.0 ** -24)
FLT_MAX = float(np.finfo(np.float32).max)
PAD = 64      # sentinel elements past the end of every output


def _close(got, ref, tol, what):
    got, ref, tol = (np.asarray(x, dtype=np.float64) for x in (got, ref, tol))
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print(f'[tol] {what}: max err {float(err.max()) if err.size else 0.0:.3e}, worst err/tol {ratio:.3f}')
    assert not np.isnan(err).any() and (err <= tol).all(), f'{what}: {int((err > tol).sum())}/{err.size} beyond the bound, err/tol {ratio:.3f}'


def _padded(n, fill, dtype=torch.float32):
    return torch.full((n + PAD,), fill, dtype=dtype, device=DEV)


def _intact(buf, n, fill, what):
    assert bool((buf[n:] == fill).all()), f'{what}: written past its end'


# ------------------------------------------------------------------------------------------------ draw
def _draw(hip, kind, B, J, Hp, A, prop, noise, want_idx=True):
    M = B * J
    actions = _padded(Hp * M * A, -7.0)
    act_idx = _padded(Hp * M, -1, torch.int32) if want_idx else None
    hip.call('dm_cem_draw', kind, B, J, Hp, A, hip.fptr(prop), hip.fptr(noise), hip.fptr(actions), hip.ptr(act_idx), hip.stream())
    _intact(actions, Hp * M * A, -7.0, 'actions')
    if want_idx:
        _intact(act_idx, Hp * M, -1, 'act_idx')
    return actions[:Hp * M * A].view(Hp, M, A), (act_idx[:Hp * M].view(Hp, M) if want_idx else None)


def _onehot_case(B, J, Hp, A, seed):
    """Probabilities (B, Hp, A) with one class at exactly 0 (A >= 2) and uniforms (Hp, M) whose first entries are 0 and the
    largest float below 1."""
    rs = np.random.RandomState(seed)
    p = rs.dirichlet(np.full(A, 0.7), size=(B, Hp)).astype(np.float32)
    if A >= 2:
        p[..., rs.randint(A)] = 0.0
    u = rs.uniform(0, 1, (Hp, B * J)).astype(np.float32)
    u = np.minimum(u, U_MAX)
    flat = u.reshape(-1)
    flat[0] = 0.0
    flat[-1] = U_MAX
    if flat.size > 2:
        flat[1] = U_MAX
    return p, u


def _onehot_rule(p, u, J):
    """The stated rule in fp32 on the host: total and cdf by sequential adds in class order, idx = #{k : cdf_k <= fl(u total)}
    clamped to A - 1.  numpy's float32 arithmetic rounds every operation."""
    B, Hp, A = p.shape
    M = u.shape[1]
    pr = np.repeat(p.transpose(1, 0, 2), J, axis=1)      # (Hp, M, A): row m reads environment m // J
    total = np.zeros((Hp, M), np.float32)
    for k in range(A):
        total = total + pr[..., k]
    target = u * total
    cdf, idx = np.zeros((Hp, M), np.float32), np.zeros((Hp, M), np.int32)
    for k in range(A):
        cdf = cdf + pr[..., k]
        idx += (cdf <= target)
    return np.minimum(idx, A - 1), pr


GRID = list(itertools.product((1, 3), (1, 2, 64, 65, 1000), (1, 3, 12), (1, 2, 6, 18, 29, 64)))


def test_draw_onehot_is_the_stated_rule_over_the_grid(hip):
    """Exact: the index is an integer function of fp32 sums whose order the kernel states, so the host restatement in numpy float32
    has the same bits and the comparison has no tolerance.  Against dm_sample_onehot on log(prop) the index must agree wherever the
    uniform is not within 1e-5 of a boundary of the float64 CDF (that entry goes through exp(log p) and a division, 3 roundings of
    2^-24 per class on A <= 64 classes: its CDF moves by less than 1e-5)."""
    agree = rows_total = 0
    for n, (B, J, Hp, A) in enumerate(GRID):
        M = B * J
        p, u = _onehot_case(B, J, Hp, A, seed=n)
        want, pr = _onehot_rule(p, u, J)
        actions, act_idx = _draw(hip, 0, B, J, Hp, A, torch.from_numpy(p).to(DEV), torch.from_numpy(u).to(DEV))
        got = act_idx.cpu().numpy()
        assert np.array_equal(got, want), (B, J, Hp, A, int((got != want).sum()))
        onehot = np.zeros((Hp, M, A), np.float32)
        np.put_along_axis(onehot, want[..., None].astype(np.int64), 1.0, axis=2)
        assert np.array_equal(actions.cpu().numpy(), onehot), (B, J, Hp, A)
        # dm_sample_onehot(rows, 1, A, log(prop)) on the same rows and uniforms
        rows = Hp * M
        logits = torch.from_numpy(pr.reshape(rows, A)).to(DEV).log().contiguous()
        oh2 = torch.empty(rows, A, device=DEV)
        idx2 = torch.empty(rows, dtype=torch.int32, device=DEV)
        hip.call('dm_sample_onehot', rows, 1, A, hip.fptr(logits), A, hip.fptr(torch.from_numpy(u.reshape(-1).copy()).to(DEV)), None,
                 hip.fptr(oh2), A, hip.ptr(idx2), hip.stream())
        p64 = pr.reshape(rows, A).astype(np.float64)
        cdf64 = np.cumsum(p64, 1) / p64.sum(1, keepdims=True)
        clear = (np.abs(cdf64 - u.reshape(rows, 1).astype(np.float64)) > 1e-5).all(1)
        assert np.array_equal(idx2.cpu().numpy()[clear], got.reshape(-1)[clear]), (B, J, Hp, A)
        agree += int(clear.sum())
        rows_total += rows
    print(f'[draw] {len(GRID)} shapes, {rows_total} rows, {agree} compared against dm_sample_onehot')
    assert agree > 0.9 * rows_total


def test_draw_onehot_never_picks_a_zero_class_below_the_top(hip):
    """A class of probability 0 adds nothing to the CDF: for u < 1 - 2^-20 it is never drawn."""
    B, J, Hp, A = 3, 65, 3, 6
    p, u = _onehot_case(B, J, Hp, A, seed=5)
    u = np.minimum(u, np.float32(1 - 2.0 ** -20))
    _, act_idx = _draw(hip, 0, B, J, Hp, A, torch.from_numpy(p).to(DEV), torch.from_numpy(u).to(DEV))
    idx = act_idx.cpu().numpy().astype(np.int64)
    pr = np.repeat(p.transpose(1, 0, 2), J, axis=1)
    assert (np.take_along_axis(pr, idx[..., None], 2) > 0).all()


@pytest.mark.parametrize('kind', [1, 2])
@pytest.mark.parametrize('B,J,Hp,A', [(1, 1, 1, 1), (3, 65, 3, 6), (2, 1000, 12, 17), (1, 2, 64, 64)])
def test_draw_continuous_is_bit_equal(hip, kind, B, J, Hp, A):
    """action = clamp(fl(mean + fl(std eps)), -1, 1): two fp32 operations on the host (torch's CPU mul and add round separately)."""
    gen = torch.Generator().manual_seed(100 * kind + J)
    M = B * J
    mean = torch.empty(B, Hp, A).uniform_(-1.2, 1.2, generator=gen)
    std = torch.empty(B, Hp, A).uniform_(0.05, 1.0, generator=gen)
    eps = torch.randn(Hp, M, A, generator=gen)
    prop = torch.cat((mean, std), -1).contiguous()
    actions, _ = _draw(hip, kind, B, J, Hp, A, prop.to(DEV), eps.to(DEV), want_idx=False)
    ex = lambda x: x.permute(1, 0, 2).repeat_interleave(J, dim=1)      # (B, Hp, A) -> (Hp, M, A)
    raw = ex(mean) + ex(std) * eps
    want = raw.clamp(-1.0, 1.0)
    if Hp * M * A > 100:
        assert (raw > 1).any() and (raw < -1).any() and ((raw > -1) & (raw < 1)).any(), 'the case straddles both clamps'
    assert torch.equal(actions.cpu(), want)


# ------------------------------------------------------------------------------------------------ update
def _update(hip, kind, B, J, K, Hp, A, gamma, reward, terminal, value, actions, act_idx, prop_in, alpha, floor, alias=False):
    M, W = B * J, (A if kind == 0 else 2 * A)
    dev = lambda x: None if x is None else x.to(DEV).contiguous()
    reward, terminal, value, actions, act_idx = (dev(x) for x in (reward, terminal, value, actions, act_idx))
    pin = prop_in.to(DEV).clone().contiguous()
    o = dict(ret=_padded(M, -7.0), elite=_padded(B * K, -1, torch.int32), first=_padded(B * A, -7.0), stats=_padded(B * 4, -7.0))
    pout = pin if alias else _padded(B * Hp * W, -7.0)
    hip.call('dm_cem_update', kind, B, J, K, Hp, A, gamma, hip.fptr(reward), hip.fptr(terminal), hip.fptr(value), hip.fptr(actions),
             hip.ptr(act_idx), hip.fptr(pin), alpha, floor, hip.fptr(pout), hip.fptr(o['ret']), hip.ptr(o['elite']), hip.fptr(o['first']),
             hip.fptr(o['stats']), hip.stream())
    for k, n, fill in (('ret', M, -7.0), ('elite', B * K, -1), ('first', B * A, -7.0), ('stats', B * 4, -7.0)):
        _intact(o[k], n, fill, k)
    if not alias:
        _intact(pout, B * Hp * W, -7.0, 'prop_out')
        assert torch.equal(pin.cpu(), prop_in), 'prop_in was written'
    return dict(ret=o['ret'][:M].cpu().numpy(), elite=o['elite'][:B * K].view(B, K).cpu().numpy(),
                first=o['first'][:B * A].view(B, A).cpu().numpy(), stats=o['stats'][:B * 4].view(B, 4).cpu().numpy(),
                prop=pout.reshape(-1)[:B * Hp * W].view(B, Hp, W).cpu().numpy())


def _case(kind, B, J, Hp, A, seed, quantised):
    """Inputs of one update.  quantised: every return is one of four values (the reward of the first step is a multiple of 0.25, the
    rest 0, no terminals, no value), so ties are everywhere; with J >= 3 candidate 1 of every environment returns NaN and
    candidate 2 +inf."""
    gen = torch.Generator().manual_seed(seed)
    M = B * J
    if quantised:
        reward = torch.zeros(Hp, M)
        reward[0] = torch.randint(0, 4, (M,), generator=gen).float() * 0.25
        terminal, value = torch.zeros(Hp, M), None
        if J >= 3:
            reward[0, 1::J] = float('nan')
            reward[0, 2::J] = float('inf')
    else:
        reward = torch.randn(Hp, M, generator=gen)
        terminal = torch.rand(Hp, M, generator=gen) * (torch.rand(Hp, M, generator=gen) < 0.3)
        value = torch.randn(M, generator=gen) * 3
    if kind == 0:
        act_idx = torch.randint(0, A, (Hp, M), generator=gen).to(torch.int32)
        actions = torch.nn.functional.one_hot(act_idx.long(), A).float()
        pin = torch.softmax(torch.randn(B, Hp, A, generator=gen), -1)
    else:
        act_idx = None
        actions = torch.empty(Hp, M, A).uniform_(-1, 1, generator=gen)
        pin = torch.cat((torch.randn(B, Hp, A, generator=gen) * 0.3, torch.empty(B, Hp, A).uniform_(0.1, 1.0, generator=gen)), -1)
    return dict(reward=reward, terminal=terminal, value=value, actions=actions, act_idx=act_idx, prop_in=pin.contiguous())


def _check_update(kind, B, J, K, Hp, A, gamma, alpha, floor, c, got, what):
    """Every output of one dm_cem_update call against the host."""
    M, K_ = B * J, float(K)
    g32, a32, f32 = (float(np.float32(x)) for x in (gamma, alpha, floor))
    r, tm = c['reward'].double().numpy(), c['terminal'].double().numpy()
    # ret: sum_t g^(t-1) w_t r_t (+ g^Hp w_(Hp+1) v).  Stated order: g carries t - 1 roundings, w 2 (t - 1), a term two more, the sum
    # Hp + 1 adds: |err| <= (4 Hp + 3) u sum |terms|
    w, ret64, mag = np.ones(M), np.zeros(M), np.zeros(M)
    for t in range(Hp):
        term = g32 ** t * w * r[t]
        ret64, mag, w = ret64 + term, mag + np.abs(term), w * (1.0 - tm[t])
    if c['value'] is not None:
        term = g32 ** Hp * w * c['value'].double().numpy()
        ret64, mag = ret64 + term, mag + np.abs(term)
    ret = got['ret']
    fin = np.isfinite(ret64)
    assert np.array_equal(np.isnan(ret), np.isnan(ret64)) and np.array_equal(np.isposinf(ret), np.isposinf(ret64)), what
    _close(ret[fin], ret64[fin], (4 * Hp + 3) * U * mag[fin] + 1e-45, f'{what} ret')
    # elite: the stated rule on the kernel's own ret
    key = np.where(np.isfinite(ret), ret, np.float32(-FLT_MAX)).astype(np.float32).reshape(B, J)
    order = np.stack([np.lexsort((np.arange(J), -key[b].astype(np.float64))) for b in range(B)])
    assert np.array_equal(got['elite'], order[:, :K].astype(np.int32)), what
    el = order[:, :K]                                   # (B, K) candidates in rank order
    rows = el + np.arange(B)[:, None] * J               # their rows m
    acts = c['actions'].numpy()
    assert np.array_equal(got['first'], acts[0, rows[:, 0]]), what
    st = got['stats']
    ek = np.take_along_axis(key, el, 1).astype(np.float64)
    assert np.array_equal(st[:, 0], ek[:, 0].astype(np.float32)), what
    for b in range(B):      # mean elite return: a sequential fp32 sum of K keys, then one division
        if np.abs(np.cumsum(ek[b])).max() > FLT_MAX:
            assert st[b, 1] == -np.inf, (what, st[b, 1])
        else:
            _close(st[b, 1], ek[b].mean(), (K + 1) * U * np.abs(ek[b]).mean(), f'{what} mean elite return[{b}]')
    assert (st[:, 0] >= st[:, 1]).all(), what
    pin = c['prop_in'].double().numpy()
    if kind == 0:
        ai = c['act_idx'].numpy()
        cnt = np.zeros((B, Hp, A), np.int64)
        for b in range(B):
            for t in range(Hp):
                cnt[b, t] = np.bincount(ai[t, rows[b]], minlength=A)
        # freq = fl(cnt / K), mix, (1 - floor) mix + floor / A: at most 8 roundings on non-negative terms
        ref = (1 - f32) * (a32 * pin + (1 - a32) * cnt / K_) + f32 / A
        _close(got['prop'], ref, 8 * U * ref, f'{what} prop_out')
        p0 = got['prop'][:, 0].astype(np.float64)
        plogp = np.where(p0 > 0, p0 * np.log(np.where(p0 > 0, p0, 1.0)), 0.0)
        # entropy of the kernel's own prop_out[b][0]: logf within 2 ulp, a product and A sequential adds per class
        _close(st[:, 2], -plogp.sum(1), (A + 4) * U * np.abs(plogp).sum(1) + 4 * U, f'{what} entropy')
        assert np.array_equal(st[:, 3], got['prop'][np.arange(B), 0, ai[0, rows[:, 0]]]), what
    else:
        x = np.stack([acts[:, rows[b]] for b in range(B)]).astype(np.float64)      # (B, Hp, K, A)
        mean_e, std_e = x.mean(2), x.std(2)
        # two passes in rank order: the mean is a sequential sum of K terms and a division, |err| <= (K + 1) u mean|x| = dm; the
        # deviations from a mean that is off by dm have the variance var + dm^2 exactly (their own mean is 0), so the std moves by
        # at most min(dm, dm^2 / 2 std); then K + 1 products, adds and a division on non-negative terms and sqrtf: (K + 6) u std
        dm = (K + 1) * U * np.abs(x).mean(2)
        with np.errstate(divide='ignore', invalid='ignore'):
            ds = np.minimum(dm, np.where(std_e > 0, dm * dm / (2 * std_e), dm)) + (K + 6) * U * std_e
        mean_ref = a32 * pin[..., :A] + (1 - a32) * mean_e
        std_mix = a32 * pin[..., A:] + (1 - a32) * std_e
        _close(got['prop'][..., :A], mean_ref, dm + 4 * U * (np.abs(a32 * pin[..., :A]) + np.abs(mean_e)), f'{what} mean_out')
        _close(got['prop'][..., A:], np.maximum(std_mix, f32), ds + 4 * U * np.abs(std_mix), f'{what} std_out')
        s0 = got['prop'][:, 0, A:].astype(np.float64)
        _close(st[:, 2], np.log(s0).sum(1), (A + 4) * U * np.abs(np.log(s0)).sum(1) + 4 * U, f'{what} sum log std')
        assert (st[:, 3] == 0).all(), what
    return order


SHAPES = [(1, 1, 1, 1), (3, 65, 3, 6), (2, 1000, 12, 18), (1, 300, 64, 64)]


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('B,J,Hp,A', SHAPES)
def test_update_with_ties_nan_and_inf(hip, kind, B, J, Hp, A):
    """Returns quantised to four values, a NaN and a +inf return per environment, K in {1, 2, J - 1, J}: the elites are the stated
    comparison count on the kernel's own ret, and every other output follows from them."""
    c = _case(kind, B, J, Hp, A, seed=7 * J + kind, quantised=True)
    for K in sorted({k for k in (1, 2, J - 1, J) if 1 <= k <= J}):
        got = _update(hip, kind, B, J, K, Hp, A, 0.97, alpha=0.0, floor=0.01, **c)
        order = _check_update(kind, B, J, K, Hp, A, 0.97, 0.0, 0.01, c, got, f'kind {kind} {(B, J, K, Hp, A)}')
        if J >= 3 and K < J - 1:      # NaN and +inf rank last, behind every finite return
            assert not np.isin(got['elite'], (1, 2)).any()
        if J >= 3:
            assert set(order[0, -2:]) == {1, 2}


@pytest.mark.parametrize('kind', [0, 2])
@pytest.mark.parametrize('B,J,Hp,A', SHAPES)
def test_update_against_float64(hip, kind, B, J, Hp, A):
    """Random rewards, terminals in [0, 1) and a value; alpha = 0.25 mixes the previous proposal in.  Aliasing prop_out with prop_in
    and running the call twice give the same bits."""
    c = _case(kind, B, J, Hp, A, seed=11 * J + kind, quantised=False)
    K = max(1, J // 10)
    floor = 0.05 if kind == 0 else 0.3
    got = _update(hip, kind, B, J, K, Hp, A, 0.99, alpha=0.25, floor=floor, **c)
    _check_update(kind, B, J, K, Hp, A, 0.99, 0.25, floor, c, got, f'kind {kind} {(B, J, K, Hp, A)}')
    if kind != 0:
        assert (got['prop'][..., A:] >= np.float32(floor)).all()
    again = _update(hip, kind, B, J, K, Hp, A, 0.99, alpha=0.25, floor=floor, **c)
    alias = _update(hip, kind, B, J, K, Hp, A, 0.99, alpha=0.25, floor=floor, alias=True, **c)
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=True), f'{k}: a second call gave other bits'
        assert np.array_equal(got[k], alias[k], equal_nan=True), f'{k}: prop_out aliasing prop_in gave other bits'


def test_update_std_survives_cancellation(hip):
    """Elite actions 0.9 +- 1e-4: the two-pass std is within its bound; a one-pass E[x^2] - mean^2 in fp32 on the host is not (it
    loses K u x^2 / 2 std, two hundred times the std's bound), so the bound tells the two apart."""
    B, J, K, Hp, A = 1, 200, 100, 1, 2
    gen = torch.Generator().manual_seed(0)
    sign = (torch.rand(Hp, J, A, generator=gen) < 0.5).float() * 2 - 1
    actions = (0.9 + 1e-4 * sign).float()
    reward = torch.randperm(J, generator=gen).float().view(Hp, J)      # distinct returns: the elites are the top K
    c = dict(reward=reward, terminal=torch.zeros(Hp, J), value=None, actions=actions, act_idx=None,
             prop_in=torch.cat((torch.zeros(B, Hp, A), torch.ones(B, Hp, A)), -1))
    got = _update(hip, 1, B, J, K, Hp, A, 0.99, alpha=0.0, floor=0.0, **c)
    order = _check_update(1, B, J, K, Hp, A, 0.99, 0.0, 0.0, c, got, 'cancellation')
    x = actions[0, order[0, :K]].numpy()                      # (K, A) float32, rank order
    std64 = x.astype(np.float64).std(0)
    dm = (K + 1) * U * np.abs(x.astype(np.float64)).mean(0)
    tol = np.minimum(dm, dm * dm / (2 * std64)) + (K + 6) * U * std64
    s1, s2 = np.zeros(A, np.float32), np.zeros(A, np.float32)
    for r in range(K):
        s1, s2 = s1 + x[r], s2 + x[r] * x[r]
    var1 = s2 / np.float32(K) - (s1 / np.float32(K)) ** 2
    std1 = np.sqrt(np.maximum(var1, 0))
    print(f'[cancel] std64 {std64}, kernel {got["prop"][0, 0, A:]}, one-pass fp32 {std1}, tol {tol}')
    assert (np.abs(got['prop'][0, 0, A:].astype(np.float64) - std64) <= tol).all()
    assert (np.abs(std1.astype(np.float64) - std64) > tol).all(), 'the one-pass form passed: the bound cannot tell'
