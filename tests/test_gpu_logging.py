"""-m gpu: the four logging kernels of csrc/logging.hip against numpy float64 / a Python loop.

  dm_metric_accum     n {1, 48, 64, 256}, six successive calls of values that include NaN, +-inf and -0.0 under every rule: sum and
                      count EQUAL to a Python loop `s += float(v)` under the rule, max equal, rule-0 slots untouched.
  dm_batch_stats      n {1, 63, 64, 65, 257, 2500}: the means within 2^-23 |mean| + 1e-12 mean|x| of the float64 mean (one fp32
                      rounding of an fp64 sum whose own error is below n 2^-53), the reset mean and the max equal; NaN; no terminal.
  dm_masked_mean      T {1, 3, 5, 7} with take_rows 5, B {1, 3, 65}, ldx > B, at the same bar; NaNs skipped, empty sets, inf.
  dm_export_image_u8  (T,B) {(1,1), (2,3)}, take_b {1, B, 999}, C {1, 3}, H = W {7, 64}: np.array_equal to numpy's float32 rule.
  host checks         nothing launched: NULL pointers, n > 256, C = 2, H != W, a rule above 4 (the Python wrapper's)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN, INF = float('nan'), float('inf')
POOL = [NAN, INF, -INF, -0.0, 0.0, 1.5, -2.25, 3e38, -3e38, 1e-40, 0.1, 7.0]


def _bar(ref_mean, mean_abs):
    return 2.0 ** -23 * abs(ref_mean) + 1e-12 * mean_abs


def _counted(rule, v):
    return (rule == 1 and not math.isnan(v)) or (rule == 2 and math.isfinite(v)) or rule == 3


def _accum_case(hip, n, rules, seed):
    from pydreamer_amd import train as TR
    rs = np.random.RandomState(seed)
    rules_dev = TR.rules_tensor(rules, DEV)
    # sentinels in the accumulators: what a rule-0 slot must keep
    s0, m0, c0 = rs.randn(n), rs.randn(n), rs.randint(0, 9, n).astype(np.int64)
    for i, r in enumerate(rules):
        if r != 0:
            s0[i], m0[i], c0[i] = 0.0, -INF, 0
    acc_s, acc_m, acc_c = (torch.from_numpy(a.copy()).to(DEV) for a in (s0, m0, c0))
    ref_s, ref_m, ref_c = [float(x) for x in s0], [float(x) for x in m0], [int(x) for x in c0]
    for call in range(6):
        vals = np.array([POOL[j] for j in rs.randint(0, len(POOL), n)], np.float32)
        if call == 0:
            vals[:min(n, len(POOL))] = np.array(POOL, np.float32)[:n]
        hip.call('dm_metric_accum', n, hip.fptr(torch.from_numpy(vals).to(DEV)), hip.ptr(rules_dev), hip.ptr(acc_s), hip.ptr(acc_m),
                 hip.ptr(acc_c), hip.stream())
        for i, r in enumerate(rules):
            v = float(vals[i])
            counted = _counted(r, v)
            if counted:
                ref_s[i] += v
                ref_c[i] += 1
            if (r == 2 and counted) or r == 4:
                ref_m[i] = NAN if (math.isnan(v) or math.isnan(ref_m[i])) else max(ref_m[i], v)
    got_s, got_m, got_c = acc_s.cpu().numpy(), acc_m.cpu().numpy(), acc_c.cpu().numpy()
    assert np.array_equal(got_c, np.array(ref_c)), (got_c, ref_c)
    assert np.array_equal(got_s, np.array(ref_s), equal_nan=True), (got_s, ref_s)
    ok = ~np.isnan(got_s)
    assert np.array_equal(np.signbit(got_s[ok]), np.signbit(np.array(ref_s)[ok]))
    assert np.array_equal(got_m, np.array(ref_m), equal_nan=True), (got_m, ref_m)


@pytest.mark.parametrize('n', [1, 48, 64, 256])
def test_metric_accum(hip, n):
    if n == 1:
        for rule in range(5):
            _accum_case(hip, 1, [rule], seed=rule)
    else:
        for shift in range(5):      # every slot meets every rule, so the twelve special values of call 0 do too
            _accum_case(hip, n, [(i + shift) % 5 for i in range(n)], seed=n + shift)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 2500])
def test_batch_stats(hip, n):
    from pydreamer_amd import train as TR
    rs = np.random.RandomState(n)
    reward = (rs.randn(n) * 3 + 0.5).astype(np.float32)
    reset = rs.rand(n) < 0.3
    terminal = (rs.rand(n) < 0.2).astype(np.float32) * rs.rand(n).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    out = TR.batch_stats(dev(reward), dev(reset), dev(terminal)).cpu().numpy()
    for got, x, what in ((out[0], reward, 'reward'), (out[2], terminal, 'terminal')):
        ref = float(x.astype(np.float64).mean())
        bar = _bar(ref, float(np.abs(x.astype(np.float64)).mean()))
        print(f'n {n} mean {what}: got {got:.9g} float64 {ref:.9g} |err| {abs(float(got) - ref):.3e} bar {bar:.3e}')
        assert abs(float(got) - ref) <= bar, (what, got, ref, bar)
    assert out[1] == np.float32(reset.sum()) / np.float32(n)
    assert out[3] == reward.max()
    # no terminal column; the same bits for the rest
    out2 = TR.batch_stats(dev(reward), dev(reset), None).cpu().numpy()
    assert out2[2] == 0.0 and out2[0] == out[0] and out2[1] == out[1] and out2[3] == out[3]
    # a NaN reward: the mean and the max
    reward[n // 2] = NAN
    out3 = TR.batch_stats(dev(reward), dev(reset), dev(terminal)).cpu().numpy()
    assert np.isnan(out3[0]) and np.isnan(out3[3]) and out3[1] == out[1] and out3[2] == out[2]


@pytest.mark.parametrize('B', [1, 3, 65])
@pytest.mark.parametrize('T', [1, 3, 5, 7])
def test_masked_mean(hip, T, B):
    from pydreamer_amd import train as TR
    rs = np.random.RandomState(100 * T + B)
    ldx, rows = B + 3, min(5, T)
    wide = (rs.randn(T, ldx) * 2 - 1).astype(np.float32)
    keep = rs.rand(B) < 0.6
    keep[rs.randint(B)] = True
    xd = torch.from_numpy(wide).to(DEV)
    view = xd[:, :B]      # ldx > B: the columns beyond B are never read
    kd = torch.from_numpy(keep).to(DEV)

    def check(got, sel, what):
        ref = float(sel.astype(np.float64).mean())
        bar = _bar(ref, float(np.abs(sel.astype(np.float64)).mean()))
        print(f'T {T} B {B} {what}: got {float(got):.9g} float64 {ref:.9g} |err| {abs(float(got) - ref):.3e} bar {bar:.3e}')
        assert abs(float(got) - ref) <= bar, (what, float(got), ref, bar)

    x = wide[:rows, :B]
    check(TR.masked_mean(view, 5, None, skip_nan=False).item(), x, 'all columns')
    check(TR.masked_mean(view, 5, kd, skip_nan=False).item(), x[:, keep], 'kept columns')
    check(TR.masked_mean(view, 5, kd, skip_nan=True).item(), x[:, keep], 'kept columns, skip_nan without NaNs')
    # NaNs sprinkled in: skipped with skip_nan = 1, poison with 0
    holes = rs.rand(T, B) < 0.3
    holes[0, np.flatnonzero(keep)[0]] = True
    w2 = wide.copy()
    w2[:, :B][holes] = NAN
    v2 = torch.from_numpy(w2).to(DEV)[:, :B]
    sel = w2[:rows, :B][:, keep]
    sel = sel[~np.isnan(sel)]
    got = TR.masked_mean(v2, 5, kd, skip_nan=True).item()
    if sel.size:
        check(got, sel, 'skip_nan with NaNs')
    else:
        assert math.isnan(got)
    assert math.isnan(TR.masked_mean(v2, 5, kd, skip_nan=False).item())
    # empty sets
    none = torch.zeros(B, dtype=torch.bool, device=DEV)
    assert math.isnan(TR.masked_mean(view, 5, none, skip_nan=True).item())
    assert math.isnan(TR.masked_mean(view, 5, none, skip_nan=False).item())
    assert math.isnan(TR.masked_mean(torch.full((T, B), NAN, device=DEV), 5, None, skip_nan=True).item())
    # skip_nan = 0: an inf in a kept column shows, a NaN in a column that is not kept does not
    if B > 1:
        k3 = np.ones(B, bool)
        k3[B - 1] = False
        for sign in (1.0, -1.0):
            w3 = wide.copy()
            w3[0, 0], w3[0, B - 1] = sign * INF, NAN
            got = TR.masked_mean(torch.from_numpy(w3).to(DEV)[:, :B], 5, torch.from_numpy(k3).to(DEV), skip_nan=False).item()
            assert got == sign * INF, got


def _special_inputs():
    k = np.arange(256, dtype=np.float32)
    base = (k / np.float32(255.0) - np.float32(0.5)).astype(np.float32)
    return np.concatenate([base, np.nextafter(base, np.float32(INF)), np.nextafter(base, np.float32(-INF)),
                           np.array([INF, -INF, 0.5, -0.5, 0.0, -0.0], np.float32)])


@pytest.mark.parametrize('HW', [7, 64])
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('TB', [(1, 1), (2, 3)])
def test_export_image_u8(hip, TB, C, HW):
    from pydreamer_amd import train as TR
    T, B = TB
    rs = np.random.RandomState(T * 100 + C * 10 + HW)
    x = rs.uniform(-0.7, 0.7, (T, B, C, HW, HW)).astype(np.float32)
    sp = _special_inputs()
    flat = x.reshape(-1)
    start = (17 * C + HW + T) % len(sp)      # small tensors hold a different window of the special values each
    m = min(flat.size, len(sp))
    flat[:m] = np.roll(sp, -start)[:m]
    if HW == 64:
        assert flat.size >= len(sp)          # ... and the large ones hold all of them
    xd = torch.from_numpy(x).to(DEV)
    for take_b in sorted({1, B, 999}):
        got = TR.export_image_u8(xd, take_b).cpu().numpy()
        v = x[:, :take_b] if take_b < B else x
        ref = ((v.transpose(0, 1, 3, 4, 2) + 0.5) * 255.0).clip(0, 255).astype('uint8').swapaxes(0, 1)
        assert got.dtype == np.uint8 and got.shape == ref.shape == (min(take_b, B), T, HW, HW, C)
        assert np.array_equal(got, ref), int((got != ref).sum())
    xn = xd.clone()
    xn.view(-1)[::5] = NAN      # NaN gives 0; the other elements as before
    got = TR.export_image_u8(xn, 999).permute(1, 0, 4, 2, 3).cpu().numpy()
    nan = np.isnan(xn.cpu().numpy())
    ref = ((x + 0.5) * 255.0).clip(0, 255).astype('uint8')
    assert (got[nan] == 0).all() and np.array_equal(got[~nan], ref[~nan])


def test_host_checks_launch_nothing(hip):
    from pydreamer_amd import train as TR
    E = hip.DreamerHipError
    f = torch.zeros(300, device=DEV)
    d = torch.zeros(300, dtype=torch.float64, device=DEV)
    c = torch.zeros(300, dtype=torch.int64, device=DEV)
    r = torch.zeros(300, dtype=torch.uint8, device=DEV)
    st = hip.stream()
    P = hip.ptr
    for args in ((4, None, P(r), P(d), P(d), P(c)), (4, P(f), None, P(d), P(d), P(c)), (4, P(f), P(r), None, P(d), P(c)),
                 (4, P(f), P(r), P(d), None, P(c)), (4, P(f), P(r), P(d), P(d), None)):
        with pytest.raises(E, match='code -5'):
            hip.call('dm_metric_accum', *args, st)
    for n in (0, 257):
        with pytest.raises(E, match='code -1'):
            hip.call('dm_metric_accum', n, P(f), P(r), P(d), P(d), P(c), st)
    with pytest.raises(E, match='code -5'):
        hip.call('dm_batch_stats', 4, None, P(r), None, P(f), st)
    with pytest.raises(E, match='code -5'):
        hip.call('dm_batch_stats', 4, P(f), P(r), None, None, st)
    with pytest.raises(E, match='code -1'):
        hip.call('dm_batch_stats', 0, P(f), P(r), None, P(f), st)
    with pytest.raises(E, match='code -5'):
        hip.call('dm_masked_mean', 2, 2, None, 2, 5, None, 1, P(f), st)
    with pytest.raises(E, match='code -1'):
        hip.call('dm_masked_mean', 2, 4, P(f), 3, 5, None, 1, P(f), st)      # ldx < B
    with pytest.raises(E, match='code -5'):
        hip.call('dm_export_image_u8', 1, 1, 1, 3, 4, 4, None, P(r), st)
    with pytest.raises(E, match='code -1'):
        hip.call('dm_export_image_u8', 1, 1, 1, 2, 4, 4, P(f), P(r), st)      # C = 2
    with pytest.raises(E, match='code -1'):
        hip.call('dm_export_image_u8', 1, 1, 1, 3, 4, 5, P(f), P(r), st)      # H != W
    with pytest.raises(ValueError):
        TR.rules_tensor([0, 1, 5], DEV)
    with pytest.raises(ValueError):
        TR.MetricAccumulator({'a': (0, 7)}, DEV)
    with pytest.raises(ValueError):
        TR.MetricAccumulator({'a': (256, 1)}, DEV)
    torch.cuda.synchronize()
    assert float(f.abs().sum()) == 0 and float(d.abs().sum()) == 0 and int(c.sum()) == 0


def test_accumulator_object(hip):
    """MetricAccumulator over the kernels: names, the two-slot name, omitted names, and the refill."""
    from pydreamer_amd import train as TR
    acc = TR.MetricAccumulator({'a': (0, 1), 'g': (2, 2), 'r': [(4, 3), (7, 4)], 'never': (5, 1)}, DEV)
    steps = [[1.0, 9.0, 2.0, 9.0, 0.5, NAN, 9.0, 3.0], [NAN, 9.0, INF, 9.0, 0.25, NAN, 9.0, -1.0], [0.1, 9.0, 4.0, 9.0, 0.125, NAN, 9.0, 2.0]]
    for s in steps:
        acc.add(torch.tensor(s, device=DEV))
    out = acc.read_and_reset()
    assert out == {'a': (1.0 + float(np.float32(0.1))) / 2, 'g': 3.0, 'g_max': 4.0, 'r': (0.5 + 0.25 + 0.125) / 3, 'r_max': 3.0}
    assert acc.read_and_reset() == {}
    acc.add(torch.tensor(steps[0], device=DEV))
    assert acc.read_and_reset() == {'a': 1.0, 'g': 2.0, 'g_max': 2.0, 'r': 0.5, 'r_max': 3.0}
