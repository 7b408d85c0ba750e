"""-m gpu: the three kernel entries of the world model's free bits and symlog two-hot reward head.

  dm_kl_free_fwd / dm_kl_free_bwd   (S, C) in {(1, 2), (3, 5), (32, 32), (33, 32), (4, 63), (4, 64), (30, 0)} x rows in {1, 3, 4, 5,
      257}: rows around the forward's four rows per workgroup; (33, 32) forward plain and backward staged, (4, 64) both plain,
      (30, 0) Gaussian.  Each shape with 16-byte-aligned pointers, with every pointer one float off (the scalar staging path) and
      with dm_kl_staged_enable(0).  Three values of `free` per case: below every row's KL, above every row's KL, and the midpoint
      of the widest gap between neighbouring order statistics of the float64 row KLs in the central third - the test asserts on the
      CPU that this gap exceeds 1e-3 max(1, free), under which fp32 and float64 agree on the closed rows.  Asserted: kl and both
      entropies torch.equal to dm_kl_balance_fwd's; kl_clip == maximum(free, kl) exactly; closed == the float64 gate; dpost and
      dprior torch.equal to dm_kl_balance_bwd's on open rows and +0.0 (sign bit clear) on closed rows; guard bands around every
      output untouched; a second run gives the same bits.  Outputs are NaN-filled before each call.
  dm_twohot_head_loss   K in {2, 3, 31, 32, 33, 64, 65, 255, 256} x rows in {1, 2, 63, 64, 65, 257} x ld in {K, K + 3} x I in {1, 2,
      3} (rows rounded up to a multiple of I).  Targets: both ends of the support, beyond each end, exact bin positions, 0 and
      random values.  Asserted: for I = 1 loss, dlogits and mean bit-equal to dm_twohot_loss with weight 1, rows_total = rows and
      the same scale; the mean-only form bit-equal to dm_twohot_decode; every optional-output combination the bits of the full
      form; for I > 1 bit-equal to the I = 1 call on the expanded target; against float64 within the rule of
      tests/test_gpu_twohot_kernels.py - max(4 x the torch-fp32 composition's worst error on the same pool, 8 ulp) - with both
      numbers printed per K; guard bands; repeatability."""
import functools

import numpy as np
import pytest
import torch

from tests import twohot_case as TC
from tests import wm_v3_case as WC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN, GUARD = float('nan'), 777.0
KL_SHAPES = [(1, 2), (3, 5), (32, 32), (33, 32), (4, 63), (4, 64), (30, 0)]
KL_ROWS = [1, 3, 4, 5, 257]
SP, SQ = 0.2 / 7, 0.8 / 7 * 1.1


# ---------------------------------------------------------------------------------------------- free bits
@functools.lru_cache(maxsize=None)
def _kl_case(S, C, rows):
    """The case's inputs, their float64 row KLs and the three `free` values.  A row whose float64 KL is below 0.05 is drawn again
    (one group of two classes gives KLs of 1e-8 among 257 rows, where fp32 cannot tell the row from a closed one at any `free`
    below it): every row's KL is far above its fp32 error, so half the smallest lies below every row in fp32 too."""
    W = S * (C or 2)
    g = torch.Generator().manual_seed(7000 + 100 * S + C + 13 * rows)
    post = torch.randn(rows, W, generator=g) * 2
    prior = torch.randn(rows, W, generator=g) * 2
    for _ in range(64):
        kl64 = WC.row_kl(post.double(), prior.double(), S, C)
        low = kl64 < 0.05
        if not bool(low.any()):
            break
        prior[low] = torch.randn(int(low.sum()), W, generator=g) * 2
    assert float(kl64.min()) >= 0.05
    mid, gap = WC.mid_free(kl64.numpy())
    WC.assert_gap(mid, gap)
    return dict(post=post.reshape(-1), prior=prior.reshape(-1), kl64=kl64, frees=(0.5 * float(kl64.min()), mid, 2.0 * float(kl64.max())))


def _buf(n, off, fill):
    """n floats at 4 off bytes past a 16-byte boundary, 64 guard floats on either side; (whole, view)."""
    whole = torch.full((n + 128 + off,), GUARD, device=DEV)
    view = whole[64 + off:64 + off + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 4 * off
    return whole, view


def _guards_ok(whole, view):
    lo = (view.data_ptr() - whole.data_ptr()) // 4
    return bool((whole[:lo] == GUARD).all() and (whole[lo + view.numel():] == GUARD).all())


def _kl_run(hip, rows, S, C, post, prior, off, free):
    """free None: the pair without the gate.  Returns the outputs on the CPU after checking the guard bands."""
    W = S * (C or 2)
    names = ('kl', 'ent_post', 'ent_prior') + (('kl_clip', 'closed') if free is not None else ())
    bufs = {k: _buf(rows, off, NAN) for k in names}
    bufs.update({k: _buf(rows * W, off, NAN) for k in ('dpost', 'dprior')})
    v = {k: b[1] for k, b in bufs.items()}
    if free is None:
        hip.call('dm_kl_balance_fwd', rows, S, C, hip.fptr(post), hip.fptr(prior), hip.fptr(v['kl']), hip.fptr(v['ent_post']),
                 hip.fptr(v['ent_prior']), hip.stream())
        hip.call('dm_kl_balance_bwd', rows, S, C, hip.fptr(post), hip.fptr(prior), SP, SQ, hip.fptr(v['dpost']), hip.fptr(v['dprior']),
                 hip.stream())
    else:
        hip.call('dm_kl_free_fwd', rows, S, C, hip.fptr(post), hip.fptr(prior), free, hip.fptr(v['kl']), hip.fptr(v['kl_clip']),
                 hip.fptr(v['closed']), hip.fptr(v['ent_post']), hip.fptr(v['ent_prior']), hip.stream())
        hip.call('dm_kl_free_bwd', rows, S, C, hip.fptr(post), hip.fptr(prior), hip.fptr(v['closed']), SP, SQ, hip.fptr(v['dpost']),
                 hip.fptr(v['dprior']), hip.stream())
    torch.cuda.synchronize()
    for k, (whole, view) in bufs.items():
        assert _guards_ok(whole, view), f'({rows}, {S}, {C}) off {off} free {free}: the guard band of {k} was written'
    return {k: x.cpu().view(rows, -1) for k, x in v.items()}


def _kl_check(hip, rows, S, C, off):
    case = _kl_case(S, C, rows)
    W = S * (C or 2)
    n = rows * W
    post = _buf(n, off, 0.0)[1].copy_(case['post'])
    prior = _buf(n, off, 0.0)[1].copy_(case['prior'])
    ref = _kl_run(hip, rows, S, C, post, prior, off, None)
    assert all(bool(torch.isfinite(x).all()) for x in ref.values())
    kl64, counts = case['kl64'], []
    for free in case['frees']:
        got = _kl_run(hip, rows, S, C, post, prior, off, free)
        again = _kl_run(hip, rows, S, C, post, prior, off, free)
        what = f'({rows}, {S}, {C}) off {off} free {free:.6g}'
        for k in got:
            assert bool(torch.isfinite(got[k]).all()), f'{what}: {k} holds a non-finite value (an element not written?)'
            assert torch.equal(got[k], again[k]) and not bool((torch.signbit(got[k]) != torch.signbit(again[k])).any()), f'{what}: {k} not repeatable'
        for k in ('kl', 'ent_post', 'ent_prior'):
            assert torch.equal(got[k], ref[k]), f'{what}: {k} differs from dm_kl_balance_fwd'
        f32 = torch.tensor(free, dtype=torch.float32)
        assert torch.equal(got['kl_clip'], torch.maximum(f32, got['kl'])), f'{what}: kl_clip'
        gate = (kl64 <= free).view(rows, 1)
        assert torch.equal(got['closed'], gate.float()), f'{what}: closed differs from the float64 gate'
        for k in ('dpost', 'dprior'):
            want = torch.where(gate, torch.zeros(()), ref[k])
            assert torch.equal(got[k], want), f'{what}: {k}'
            assert not bool(torch.signbit(got[k][gate.view(-1)]).any()), f'{what}: a closed row of {k} holds -0.0'
        counts.append(int(gate.sum()))
    assert counts[0] == 0 and counts[2] == rows and (rows == 1 or 0 < counts[1] < rows), counts


@pytest.mark.parametrize('S,C', KL_SHAPES)
def test_kl_free_aligned(hip, S, C):
    assert hip.lib().dm_kl_staged_enable(-1) == 1, 'the staged kernels are on by default'
    for rows in KL_ROWS:
        _kl_check(hip, rows, S, C, 0)


@pytest.mark.parametrize('S,C', KL_SHAPES)
def test_kl_free_pointers_one_float_off(hip, S, C):
    for rows in KL_ROWS:
        _kl_check(hip, rows, S, C, 1)


@pytest.mark.parametrize('S,C', KL_SHAPES)
def test_kl_free_with_the_staged_kernels_off(hip, S, C):
    lib = hip.lib()
    try:
        assert lib.dm_kl_staged_enable(0) == 0
        for rows in KL_ROWS:
            _kl_check(hip, rows, S, C, 0)
    finally:
        lib.dm_kl_staged_enable(1)


def test_kl_free_staged_and_plain_agree(hip):
    """The switch changes the kernel, not the bits: (5, 32, 32) with the gate in the middle, on against off."""
    rows, S, C = 5, 32, 32
    case = _kl_case(S, C, rows)
    n = rows * S * C
    post, prior = case['post'].to(DEV), case['prior'].to(DEV)
    lib, free = hip.lib(), case['frees'][1]
    try:
        on = _kl_run(hip, rows, S, C, post, prior, 0, free)
        lib.dm_kl_staged_enable(0)
        off = _kl_run(hip, rows, S, C, post, prior, 0, free)
    finally:
        lib.dm_kl_staged_enable(1)
    for k in on:
        assert torch.equal(on[k], off[k]), k


# ---------------------------------------------------------------------------------------------- the two-hot head
KS = [2, 3, 31, 32, 33, 64, 65, 255, 256]
ROWS = [1, 2, 63, 64, 65, 257]
POOL, SCALE = 258, 0.25      # 258: a multiple of every I


@functools.lru_cache(maxsize=None)
def _pool(K, I):
    """POOL logit rows and POOL / I targets; on the CPU the float64 reference on the expanded target and the fp32 composition's
    worst errors against it."""
    g = torch.Generator().manual_seed(3000 + 10 * K + I)
    bins = torch.linspace(-20.0, 20.0, K)
    logits = torch.randn(POOL, K, generator=g) * 3
    logits[3] = 1.5                                      # all-equal logits
    logits[4, (K * 2) // 3] += 80.0                      # a spike
    nt = POOL // I
    target = torch.randn(nt, generator=g) * 100
    ends = TC.symexp(bins.double())
    for i in range(nt):      # every short prefix sees the special targets
        m = i % 8
        if m < 6:
            target[i] = (float(ends[0]), float(ends[-1]), 1e9, -1e9, float(ends[(i // 8) % K]), 0.0)[m]
    d = lambda t: t.double()
    ref = WC.twohot_head(d(logits), d(bins), d(target), I, SCALE)
    f32 = WC.twohot_head(logits, bins, target, I, SCALE)
    E = dict(loss=float((d(f32[0]) - ref[0]).abs().max()), dlogits=float((d(f32[1]) - ref[1]).abs().max()),
             mean=float(((d(f32[2]) - ref[2]).abs() / (1 + ref[2].abs())).max()))
    return dict(bins=bins, logits=logits, target=target, ref=ref, E=E)


def _head(hip, K, I, rows, ld, lg, bins, target, loss=True, dlogits=True, mean=True):
    out = dict(loss=_buf(rows, 0, NAN), dlogits=_buf(rows * K, 0, NAN), mean=_buf(rows, 0, NAN))
    want = dict(loss=loss, dlogits=dlogits, mean=mean)
    hip.call('dm_twohot_head_loss', rows, I, K, hip.fptr(lg), ld, hip.fptr(bins), hip.fptr(target), SCALE,
             *(hip.fptr(out[k][1]) if want[k] else None for k in ('loss', 'dlogits', 'mean')), hip.stream())
    torch.cuda.synchronize()
    for k, (whole, view) in out.items():
        assert _guards_ok(whole, view), (k, K, I, rows, ld)
        if not want[k]:
            assert bool(torch.isnan(view).all()), f'{k} was not asked for'
    return {k: v[1].clone() for k, v in out.items()}


@pytest.mark.parametrize('K', KS)
def test_twohot_head_loss(hip, K):
    worst = dict(loss=0.0, dlogits=0.0, mean=0.0)
    Es = {}
    for I in (1, 2, 3):
        P = _pool(K, I)
        E, ref = P['E'], P['ref']
        Es[I] = E
        bins, target_all = P['bins'].to(DEV), P['target'].to(DEV)
        for ld in (K, K + 3):
            lg_all = torch.full((POOL, ld), 1e30)      # the padding columns hold garbage nobody may read into a result
            lg_all[:, :K] = P['logits']
            lg_all = lg_all.to(DEV)
            for rows0 in ROWS:
                rows = -(-rows0 // I) * I
                lg, target = lg_all[:rows], target_all[:rows // I]
                full = _head(hip, K, I, rows, ld, lg, bins, target)
                what = (K, I, rows, ld)
                assert all(bool(torch.isfinite(v).all()) for v in full.values()), what
                again = _head(hip, K, I, rows, ld, lg, bins, target)
                assert all(torch.equal(full[k], again[k]) for k in full), what
                # every optional-output combination: the bits of the full form
                for combo in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
                    part = _head(hip, K, I, rows, ld, lg, bins, target, *map(bool, combo))
                    for k, on in zip(('loss', 'dlogits', 'mean'), combo):
                        assert not on or torch.equal(part[k], full[k]), (what, combo, k)
                # the mean-only form = dm_twohot_decode
                only = _head(hip, K, I, rows, ld, lg, bins, None, False, False, True)
                dw, dec = _buf(rows, 0, NAN)
                hip.call('dm_twohot_decode', rows, K, hip.fptr(lg), ld, hip.fptr(bins), hip.fptr(dec), hip.stream())
                torch.cuda.synchronize()
                assert _guards_ok(dw, dec) and torch.equal(only['mean'], dec) and torch.equal(full['mean'], dec), what
                # I = 1 on the expanded target: dm_twohot_loss with weight 1 and, for I > 1, the head call itself
                expanded = target.repeat_interleave(I).contiguous()
                ones = torch.ones(rows, device=DEV)
                cl, cd, cv = (_buf(n, 0, NAN)[1] for n in (rows, rows * K, rows))
                hip.call('dm_twohot_loss', rows, rows, K, hip.fptr(lg), ld, hip.fptr(bins), hip.fptr(expanded), hip.fptr(ones), SCALE,
                         hip.fptr(cl), hip.fptr(cd), hip.fptr(cv), hip.stream())
                torch.cuda.synchronize()
                flat = full if I == 1 else _head(hip, K, 1, rows, ld, lg, bins, expanded)
                for k, c in (('loss', cl), ('dlogits', cd), ('mean', cv)):
                    assert torch.equal(flat[k], c), (what, k, 'dm_twohot_loss with weight 1')
                    assert torch.equal(full[k], flat[k]), (what, k, 'row r against target r // I')
                # against float64
                got = dict(loss=full['loss'].double().cpu().numpy(), dlogits=full['dlogits'].view(rows, K).double().cpu().numpy(),
                           mean=full['mean'].double().cpu().numpy())
                r64 = dict(loss=ref[0][:rows].numpy(), dlogits=ref[1][:rows].numpy(), mean=ref[2][:rows].numpy())
                for name in ('loss', 'dlogits', 'mean'):
                    err = np.abs(got[name] - r64[name])
                    size = (1 + np.abs(r64[name])) if name == 'mean' else 1.0
                    bar = np.maximum(4 * E[name] * size, 8 * TC.ulp32(r64[name]))
                    worst[name] = max(worst[name], float((err / size).max()))
                    assert (err <= bar).all(), (name, what, float((err / size).max()), E[name])
    print(f'K={K}: ' + ', '.join(f'{n} kernel {worst[n]:.3e} / composition {max(Es[I][n] for I in Es):.3e}' for n in worst))
