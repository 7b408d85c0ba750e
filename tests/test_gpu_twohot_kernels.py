"""-m gpu: the three kernels of csrc/twohot.hip against the restatements of tests/twohot_case.py.

  dm_twohot_decode / dm_twohot_loss   against float64 for K in {2, 3, 31, 32, 33, 64, 65, 255, 256} x rows in {1, 2, 63, 64, 65, 257}
      x ld in {K, K + 3}.  The tolerance is not fixed in advance: the plain torch-fp32 composition (log_softmax, gather, softmax .
      bins, expm1) runs on the CPU on the K's pool of 257 rows - every case uses its first `rows` rows - and its worst error
      against float64 is E; the kernel must stay within max(4 E, 8 ulp of the result) (4 x: the lane butterfly sums in another
      order).  Loss and dlogits: absolute errors; value: relative to 1 + |v| (a decoded value reaches e^20); the row sum of dlogits:
      against the composition's worst |row sum|, floor 8 ulp of scale weight (the size of the terms, the result itself being 0).
      The comparison is on values, never on the bin index: loss and gradient are continuous in the target across a bin edge.
      Both numbers per K are printed.  Also: the dlogits tail [rows, rows_total) is +0.0 exactly, guard bands around every output
      survive, repeat calls are bit-identical, the loss-only and value-less forms give the same bits, decode = the loss call's value.
  dm_return_norm   bit-equal (out[5], the two state floats, adv) to the numpy-float32 restatement on the sorted input, for
      n in {1, 2, 3, 64, 65, 1023, 1024, 1025, 40 000} (and 2^20 + 3 once), the q pairs (0.05, 0.95), (0, 1), (0.5, 0.5), heavy
      ties, all-equal, mixed signs, +-0 with denormals, a 0.9 +- 1e-4 cluster; three consecutive updating calls for decay in
      {0, 0.5, 0.99}; update = 0 leaves the state alone; the limit holds the scale when the range is below it."""
import functools

import numpy as np
import pytest
import torch

from tests import twohot_case as TC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KS = [2, 3, 31, 32, 33, 64, 65, 255, 256]
ROWS = [1, 2, 63, 64, 65, 257]
POOL, SCALE, GUARD = 257, 0.25, 777.0


@functools.lru_cache(maxsize=None)
def _pool(K):
    """The K's inputs and, on the CPU, the float64 reference and the fp32 composition's worst errors against it."""
    g = torch.Generator().manual_seed(1000 + K)
    bins = torch.linspace(-20.0, 20.0, K)
    logits = torch.randn(POOL, K, generator=g) * 3
    logits[3] = 1.5                                      # all-equal logits
    logits[4, (K * 2) // 3] += 80.0                      # a spike
    target = torch.randn(POOL, generator=g) * 100
    on_bin = TC.symexp(bins.double())[torch.arange(POOL) % K].float()      # exactly on a bin (as near as fp32 gets)
    for i in range(POOL):       # every short prefix sees the special targets: row 0 on a bin, then 0, +-1e9 (clamped), 1e-30
        m = i % 8
        if m in (0, 1, 2, 3, 5):
            target[i] = (on_bin[i], 0.0, 1e9, -1e9, 0.0, 1e-30)[m]
    weight = torch.rand(POOL, generator=g)
    weight[1::7] = 0.0
    weight[2::5] = 1.0
    d = lambda t: t.double()
    ref = TC.twohot_compose(d(logits), d(bins), d(target), d(weight), SCALE)
    f32 = TC.twohot_compose(logits, bins, target, weight, SCALE)
    E = dict(loss=float((d(f32[0]) - ref[0]).abs().max()), dlogits=float((d(f32[1]) - ref[1]).abs().max()),
             value=float(((d(f32[2]) - ref[2]).abs() / (1 + ref[2].abs())).max()), rowsum=float(d(f32[1]).sum(-1).abs().max()))
    return dict(bins=bins, logits=logits, target=target, weight=weight, ref=ref, E=E)


def _guarded(n, fill=GUARD):
    """A buffer of n floats with 64 guard floats on either side; returns (whole, the n-float view)."""
    whole = torch.full((n + 128,), fill, device=DEV)
    return whole, whole[64:64 + n]


def _guards_ok(whole, n, fill=GUARD):
    return bool((whole[:64] == fill).all() and (whole[64 + n:] == fill).all())


def _run_loss(hip, K, rows, rows_total, ld, P, with_dlogits=True, with_value=True):
    lg = torch.full((rows, ld), 1e30)      # the padding columns hold garbage nobody may read into a result
    lg[:, :K] = P['logits'][:rows]
    lg, bins = lg.to(DEV), P['bins'].to(DEV)
    target, weight = P['target'][:rows].to(DEV), P['weight'][:rows].to(DEV)
    lw, loss = _guarded(rows)
    dw, dl = _guarded(rows_total * K)
    vw, val = _guarded(rows)
    hip.call('dm_twohot_loss', rows, rows_total, K, hip.fptr(lg), ld, hip.fptr(bins), hip.fptr(target), hip.fptr(weight), SCALE,
             hip.fptr(loss), hip.fptr(dl) if with_dlogits else None, hip.fptr(val) if with_value else None, hip.stream())
    torch.cuda.synchronize()
    assert _guards_ok(lw, rows) and _guards_ok(dw, rows_total * K) and _guards_ok(vw, rows), (K, rows, ld)
    if not with_dlogits:
        assert bool((dl == GUARD).all())
    if not with_value:
        assert bool((val == GUARD).all())
    return loss.clone(), dl.view(rows_total, K).clone(), val.clone(), lg, bins


@pytest.mark.parametrize('K', KS)
def test_twohot_loss_and_decode_against_float64(hip, K):
    P = _pool(K)
    E, (rl, rd, rv) = P['E'], P['ref']
    worst = dict(loss=0.0, dlogits=0.0, value=0.0, rowsum=0.0)
    for rows in ROWS:
        for ld in (K, K + 3):
            rows_total = rows + 3
            loss, dl, val, lg, bins = _run_loss(hip, K, rows, rows_total, ld, P)
            tail = dl[rows:]
            assert bool((tail == 0).all()) and not bool(torch.signbit(tail).any()), 'the rows behind the loss rows are +0.0'
            # repeat call, loss-only form, value-less form: the same bits
            again = _run_loss(hip, K, rows, rows_total, ld, P)
            assert torch.equal(loss, again[0]) and torch.equal(dl, again[1]) and torch.equal(val, again[2])
            assert torch.equal(loss, _run_loss(hip, K, rows, rows_total, ld, P, with_dlogits=False)[0])
            novalue = _run_loss(hip, K, rows, rows_total, ld, P, with_value=False)
            assert torch.equal(loss, novalue[0]) and torch.equal(dl, novalue[1])
            vw, dec = _guarded(rows)
            hip.call('dm_twohot_decode', rows, K, hip.fptr(lg), ld, hip.fptr(bins), hip.fptr(dec), hip.stream())
            torch.cuda.synchronize()
            assert _guards_ok(vw, rows) and torch.equal(dec, val), 'decode = the value of the loss call'
            got = dict(loss=loss.double().cpu().numpy(), dlogits=dl[:rows].double().cpu().numpy(), value=val.double().cpu().numpy())
            ref = dict(loss=rl[:rows].numpy(), dlogits=rd[:rows].numpy(), value=rv[:rows].numpy())
            for name in ('loss', 'dlogits', 'value'):
                err = np.abs(got[name] - ref[name])
                size = (1 + np.abs(ref[name])) if name == 'value' else 1.0
                bar = np.maximum(4 * E[name] * size, 8 * TC.ulp32(ref[name]))
                worst[name] = max(worst[name], float((err / size).max()))
                assert (err <= bar).all(), (name, K, rows, ld, float((err / size).max()), E[name])
            rowsum = np.abs(got['dlogits'].sum(-1))
            bar = np.maximum(4 * E['rowsum'], 8 * TC.ulp32(SCALE * P['weight'][:rows].numpy()))
            worst['rowsum'] = max(worst['rowsum'], float(rowsum.max()))
            assert (rowsum <= bar).all(), ('rowsum', K, rows, ld, float(rowsum.max()), E['rowsum'])
    print(f'K={K}: ' + ', '.join(f'{n} kernel {worst[n]:.3e} / composition {E[n]:.3e}' for n in worst))


# ---------------------------------------------------------------------------------------------- dm_return_norm
def _data(kind, n, rs):
    if kind == 'ties':
        return rs.randint(0, 4, n).astype(np.float32)
    if kind == 'equal':
        return np.full(n, 2.5, np.float32)
    if kind == 'mixed':
        return (rs.randn(n) * 50).astype(np.float32)
    if kind == 'zeros':      # +-0, denormals, +-1
        return rs.choice(np.array([0.0, -0.0, 1e-40, -1e-40, 3e-39, 1.0, -1.0], np.float32), n)
    if kind == 'cluster':
        return (0.9 + 1e-4 * rs.uniform(-1, 1, n)).astype(np.float32)
    raise AssertionError(kind)


def _call(hip, x, q, decay, limit, update, state, adv):
    n = len(x)
    xd = torch.from_numpy(x).to(DEV)
    ow, out = _guarded(5)
    aw, ad = _guarded(len(adv))
    ad.copy_(torch.from_numpy(adv))
    hip.call('dm_return_norm', n, hip.fptr(xd), q[0], q[1], decay, limit, update, hip.fptr(state), hip.fptr(out), hip.fptr(ad), len(adv),
             hip.stream())
    torch.cuda.synchronize()
    assert _guards_ok(ow, 5) and _guards_ok(aw, len(adv))
    return out.cpu().numpy(), ad.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('n', [1, 2, 3, 64, 65, 1023, 1024, 1025, 40000])
def test_return_norm_is_bit_equal_to_the_fp32_restatement(hip, n):
    rs = np.random.RandomState(n)
    for kind in ('ties', 'equal', 'mixed', 'zeros', 'cluster'):
        for q in ((0.05, 0.95), (0.0, 1.0), (0.5, 0.5)):
            for decay in (0.0, 0.5, 0.99):
                sw, state = _guarded(2)
                state.copy_(torch.tensor([-1.0, 2.0]))
                host = np.array([-1.0, 2.0], np.float32)
                for call in range(3):
                    x = _data(kind, n, rs) * np.float32(1 + call)
                    adv = (rs.randn(min(n, 37) + call) * 7).astype(np.float32)
                    out, ad = _call(hip, x, q, decay, 1.0, 1, state, adv)
                    want, host, wadv = TC.return_norm_f32(x, q[0], q[1], decay, 1.0, 1, host, adv)
                    what = (n, kind, q, decay, call)
                    assert np.array_equal(_bits(out), _bits(want)), (what, out, want)
                    assert np.array_equal(_bits(state.cpu().numpy()), _bits(host)), what
                    assert np.array_equal(_bits(ad), _bits(wadv)), what
                    assert _guards_ok(sw, 2)
                # update = 0: the state is read, not written; the scale comes from it
                x = _data(kind, n, rs)
                before = state.clone()
                out, ad = _call(hip, x, q, decay, 1.0, 0, state, adv)
                want, _, wadv = TC.return_norm_f32(x, q[0], q[1], decay, 1.0, 0, host, adv)
                assert torch.equal(state, before) and np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(ad), _bits(wadv))
                assert np.array_equal(_bits(out[2:4]), _bits(host))


def test_return_norm_limit_order_statistics_and_a_large_n(hip):
    rs = np.random.RandomState(7)
    # a range below the limit: the limit is the scale, the advantages are divided by it
    x = _data('cluster', 1025, rs)
    state = torch.zeros(2, device=DEV)
    adv = np.array([3.0, -6.0], np.float32)
    out, ad = _call(hip, x, (0.05, 0.95), 0.0, 2.0, 1, state, adv)
    assert out[3] - out[2] < 2.0 and out[4] == 2.0 and ad.tolist() == [1.5, -3.0]
    out, ad = _call(hip, x, (0.05, 0.95), 0.0, 1e-6, 1, state, adv)
    assert out[4] == np.float32(out[3] - out[2]) > 1e-6
    # q = (0, 1) and (0.5, 0.5) on an odd n are order statistics themselves: minimum, maximum, median
    x = _data('mixed', 1023, rs)
    s = np.sort(x)
    out, _ = _call(hip, x, (0.0, 1.0), 0.0, 1.0, 1, state, adv)
    assert out[0] == s[0] and out[1] == s[-1]
    out, _ = _call(hip, x, (0.5, 0.5), 0.0, 1.0, 1, state, adv)
    assert out[0] == out[1] == s[511]
    # n above 2^20, n_adv = 0 with a null adv
    x = _data('mixed', (1 << 20) + 3, rs)
    xd, out = torch.from_numpy(x).to(DEV), torch.empty(5, device=DEV)
    before = state.cpu().numpy()
    hip.call('dm_return_norm', len(x), hip.fptr(xd), 0.05, 0.95, 0.5, 1.0, 1, hip.fptr(state), hip.fptr(out), None, 0, hip.stream())
    want, _, _ = TC.return_norm_f32(x, 0.05, 0.95, 0.5, 1.0, 1, before, np.zeros(0, np.float32))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
