"""-m gpu: the row kernels of the gradient step at every dispatch branch, each against a plain fp64 restatement of the same
operation: the categorical sampler family (six kernels behind dm_sample_onehot), the straight-through softmax backward (four
instantiations), the actor-critic tail (dm_gae_losses, dm_actor_loss, dm_critic_loss, dm_multi_sum modes 1 and 2) and the
optimizer kernels (dm_multi_tensor_norm_clip, dm_scale_inplace, dm_adamw_step, dm_axpby).

Shapes are the smallest that reach a branch; the bars are those of the tests of the same kernels in test_gpu_primitives.py.
Every output buffer is filled with NaN (floats) or a marker (indices) before the call, and padding columns of strided outputs
must keep it.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DM_E_SHAPE, DM_E_WORKSPACE = -1, -2
SENT = 0x7FC0DEAD                     # a NaN with a payload no arithmetic produces
NAN = float('nan')


def _close(a, b, rtol, atol, what=''):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    err = (a - b).abs()
    bad = ~(err <= atol + rtol * b.abs())
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e}, ' \
                          f'max ref {float(b.abs().max()):.3e}'


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------- sampler
# (rows, groups, C) -> the kernel dm_sample_onehot_launch picks: C <= 8 wave<8>, <= 16 wave<16>, <= 32 wave<32>, <= 64 wave<64>,
# above that the generic one-thread-per-group kernel; C = 32 with 16-byte aligned rows: lane32.
SAMPLER_SHAPES = [(37, 3, 3), (37, 5, 8), (37, 3, 9), (37, 3, 16), (37, 2, 17), (129, 3, 32), (37, 2, 33), (37, 2, 64), (37, 2, 65),
                  (37, 1, 100)]
MARGIN = 1e-4


def _rule64(logits, u):
    """The inverse-CDF rule in fp64: idx = #{k : cdf_k <= u cdf_last} clamped to C - 1, and each draw's distance to a CDF edge."""
    p = torch.softmax(logits.double(), -1)
    cdf = torch.cumsum(p, -1)
    target = u.double().unsqueeze(-1) * cdf[..., -1:]
    idx = (cdf <= target).sum(-1).clamp(max=logits.shape[-1] - 1)
    return idx, (cdf - target).abs().min(-1).values


def _oracle_sample(logits, u):
    """The same rule on CPU fp32 (test_gpu_primitives.py's restatement)."""
    p = torch.softmax(logits.float().cpu(), -1)
    cdf = torch.cumsum(p, -1)
    target = u.float().cpu().unsqueeze(-1) * cdf[..., -1:]
    idx = (cdf <= target).sum(-1).clamp(max=logits.shape[-1] - 1)
    return idx, (cdf - target).abs().min(-1).values


_SAMPLER = {}


def _sampler_case(rows, groups, C):
    """Logits 2 randn and uniforms on the CPU; a draw closer than 1e-4 (fp64) to a CDF edge gets the midpoint of its group's
    widest bin instead, so NO draw is excluded: fp32 rounding of the rule is bounded by about C * 6e-8 <= 1e-5 at these C.
    Asserted here, before any launch: every margin >= 1e-4, and the CPU fp32 restatement gives the fp64 index everywhere."""
    key = (rows, groups, C)
    if key not in _SAMPLER:
        g = _gen(1000 * C + groups)
        logits = 2.0 * torch.randn(rows, groups, C, generator=g)
        u = torch.rand(rows, groups, generator=g)
        _, margin = _rule64(logits, u)
        near = margin < MARGIN
        p = torch.softmax(logits.double(), -1)
        cdf = torch.cumsum(p, -1)
        k = p.argmax(-1, keepdim=True)
        mid = ((cdf.gather(-1, k) - 0.5 * p.gather(-1, k)) / cdf[..., -1:]).squeeze(-1)
        u = torch.where(near, mid.float(), u)
        idx, margin = _rule64(logits, u)
        assert float(margin.min()) >= MARGIN, (key, float(margin.min()))
        idx32, _ = _oracle_sample(logits, u)
        assert torch.equal(idx32, idx), key
        _SAMPLER[key] = (logits, u, idx)
    return _SAMPLER[key]


def _run_sampler(hip, logits, u, forced=None, lpad=0, opad=0, offset=0):
    """dm_sample_onehot on (rows, groups, C) CPU logits: rows of groups*C + lpad floats (NaN padding) starting `offset` floats
    into a 16-byte aligned buffer; onehot rows of groups*C + opad floats.  Returns (idx, onehot incl. padding) on the CPU."""
    rows, groups, C = logits.shape
    W = groups * C
    buf = torch.full((offset + rows * (W + lpad),), NAN, device=DEV)
    lg = buf[offset:].view(rows, W + lpad)
    lg[:, :W] = logits.reshape(rows, W).to(DEV)
    onehot = _sentinel(rows, W + opad)
    idx = torch.full((rows, groups), -77, dtype=torch.int32, device=DEV)
    du = u.to(DEV).contiguous() if u is not None else None
    dforced = forced.int().to(DEV).contiguous() if forced is not None else None
    hip.call('dm_sample_onehot', rows, groups, C, ctypes.c_void_p(lg.data_ptr()), W + lpad, hip.fptr(du), hip.ptr(dforced),
             hip.fptr(onehot), W + opad, hip.ptr(idx), hip.stream())
    torch.cuda.synchronize()
    return idx.cpu().long(), onehot.cpu()


def _check_onehot(onehot, idx, C, opad):
    rows, groups = idx.shape
    W = groups * C
    assert torch.equal(onehot[:, :W].reshape(rows, groups, C), F.one_hot(idx, C).float()), 'onehot is not one_hot(idx)'
    assert bool((_bits(onehot[:, W:]) == SENT).all()), 'onehot padding columns were written'


@pytest.mark.parametrize('lpad,opad', [(0, 0), (4, 8), (1, 8)])
@pytest.mark.parametrize('rows,groups,C', SAMPLER_SHAPES)
def test_sample_onehot_every_kernel_exact(hip, rows, groups, C, lpad, opad):
    """GPU indices equal the fp64 indices EXACTLY (no draw excluded, see _sampler_case), onehot = one_hot(idx), the forced-index
    call reproduces them.  C 3, 8: wave<8>; 9, 16: wave<16>; 17: wave<32>; 33, 64: wave<64>; 65, 100: the generic kernel; 32: lane32
    with ldl = groups*C and + 4, wave<32> with ldl = groups*C + 1 (rows lose their 16-byte alignment).  Strides: NaN in the
    logit padding (never read), the sentinel kept in the one-hot padding (ldo = groups*C + 8)."""
    logits, u, ref = _sampler_case(rows, groups, C)
    idx, onehot = _run_sampler(hip, logits, u, lpad=lpad, opad=opad)
    assert torch.equal(idx, ref), f'{int((idx != ref).sum())} of {ref.numel()} indices differ from the fp64 rule'
    _check_onehot(onehot, idx, C, opad)
    idx_f, onehot_f = _run_sampler(hip, logits, None, forced=ref, lpad=lpad, opad=opad)
    assert torch.equal(idx_f, ref)
    _check_onehot(onehot_f, ref, C, opad)


def test_sample_onehot_c32_lane32_and_wave32_agree(hip):
    """The same C = 32 logits 16-byte aligned (lane32) and from a view one float into the buffer (wave<32>): identical indices,
    as csrc/elementwise.hip and the header promise for every kernel of the family."""
    logits, u, ref = _sampler_case(129, 3, 32)
    a, _ = _run_sampler(hip, logits, u)
    b, _ = _run_sampler(hip, logits, u, offset=1)
    assert torch.equal(a, b) and torch.equal(a, ref)
    # and on draws that are NOT kept away from the CDF edges: the two kernels must agree there too
    g = _gen(5)
    logits = 2.0 * torch.randn(2000, 4, 32, generator=g)
    u = torch.rand(2000, 4, generator=g)
    a, _ = _run_sampler(hip, logits, u)
    b, _ = _run_sampler(hip, logits, u, offset=1)
    assert torch.equal(a, b)


@pytest.mark.parametrize('rows,groups,C', SAMPLER_SHAPES)
def test_sample_onehot_edges_every_kernel(hip, rows, groups, C):
    """Per C: u = 0 on random logits (index 0) and on a delta at the LAST class (C - 1, the first class with mass); u just below 1
    and u = 1 on uniform logits (C - 1; with u = 1 every cdf_k <= the target, the count is C and only the clamp idx <= C - 1 makes
    the index a class of the group: without it the one-hot row would be all zero - C = 65 and 100 take it in the generic kernel); a delta
    distribution with u = 0.5.  The expected indices are the fp64 rule's."""
    g = _gen(C)
    j = 5 % C
    logits = torch.zeros(5, groups, C)
    logits[0] = 2.0 * torch.randn(groups, C, generator=g)
    logits[2, :, j] = 2000.0
    logits[3, :, C - 1] = 2000.0
    u = torch.tensor([0.0, 1.0 - 2.0 ** -24, 0.5, 0.0, 1.0]).unsqueeze(1).repeat(1, groups)
    want = torch.tensor([0, C - 1, j, C - 1, C - 1]).unsqueeze(1).repeat(1, groups)
    assert torch.equal(_rule64(logits, u)[0], want)
    for lpad in (0, 1):
        idx, onehot = _run_sampler(hip, logits, u, lpad=lpad, opad=8)
        assert torch.equal(idx, want), (lpad, idx.tolist())
        _check_onehot(onehot, idx, C, 8)


# ------------------------------------------------------------------------------------------- straight-through backward
def _st_case(rows, groups, C, saturated):
    g = _gen(77 * C + groups)
    logits = torch.randn(rows, groups * C, generator=g)
    if saturated:
        logits = logits * (60.0 / float(logits.abs().max()))
    dz = torch.randn(rows, groups * C, generator=g)
    base = torch.randn(rows, groups * C, generator=g)
    x = logits.double().requires_grad_(True)
    p = torch.softmax(x.reshape(rows, groups, C), -1)
    (p * dz.double().reshape(rows, groups, C)).sum().backward()
    return logits, dz, base, x.grad


def _padded(t, pad, fill=NAN):
    out = torch.full((t.shape[0], t.shape[1] + pad), fill, device=DEV)
    out[:, :t.shape[1]] = t.to(DEV)
    return out


@pytest.mark.parametrize('saturated', [False, True], ids=['unit', 'pm60'])
@pytest.mark.parametrize('accum', [0, 1])
@pytest.mark.parametrize('rows,groups,C', [s for s in SAMPLER_SHAPES if s[2] <= 64])
def test_st_softmax_bwd_every_instantiation(hip, rows, groups, C, accum, saturated):
    """dlogits (+)= p (dz - sum p dz) against fp64 autograd at test_st_softmax_bwd's bars (1e-4, 1e-6): C 3, 8 -> <8>; 9, 16 -> <16>;
    17, 32 -> <32>; 33, 64 -> <64>; overwrite and accumulate; ldl = W + 4, lddz = W + 1, lddl = W + 8 with NaN in the input padding
    and the sentinel kept in the output padding; logits scaled to +-60 (saturated softmax): finite and within the same bar."""
    logits, dz, base, ref = _st_case(rows, groups, C, saturated)
    W = groups * C
    lg, dzp = _padded(logits, 4), _padded(dz, 1)
    out = _sentinel(rows, W + 8)
    if accum:
        out[:, :W] = base.to(DEV)
    hip.call('dm_st_softmax_bwd', rows, groups, C, hip.fptr(lg), W + 4, hip.fptr(dzp), W + 1, hip.fptr(out), W + 8, accum, hip.stream())
    want = ref + base.double() if accum else ref
    assert bool(torch.isfinite(out[:, :W]).all())
    print(f'st bwd C={C} accum={accum} saturated={saturated}: max err {float((out[:, :W].double().cpu() - want).abs().max()):.3e}')
    _close(out[:, :W], want, 1e-4, 1e-6, f'st bwd C={C} accum={accum}')
    assert bool((_bits(out[:, W:]) == SENT).all()), 'dlogits padding columns were written'


def test_st_softmax_bwd_refuses_c65(hip):
    x = torch.zeros(4, 130, device=DEV)
    out = _sentinel(4, 130)
    rc = hip.lib().dm_st_softmax_bwd(4, 2, 65, hip.fptr(x), 130, hip.fptr(x), 130, hip.fptr(out), 130, 0, hip.stream())
    assert rc == DM_E_SHAPE
    torch.cuda.synchronize()
    assert bool((_bits(out) == SENT).all())


# ------------------------------------------------------------------------------------------- actor-critic tail
def _gae_ref(H, gamma, lam, reward, terminal, value_t):
    """a2c.py:81-108 in fp64 (test_gae_and_ac_losses' restatement)"""
    r, tm, vt = reward.double(), terminal.double(), value_t.double()
    advantage = -vt[:-1] + r[1:] + gamma * (1 - tm[1:]) * vt[1:]
    acc, out = None, []
    for a_, t_ in zip(reversed(advantage.unbind()), reversed(tm[1:].unbind())):
        acc = a_ if acc is None else a_ + lam * gamma * (1 - t_) * acc
        out.append(acc)
    out.reverse()
    agae = torch.stack(out)
    weight = (1 - tm[:-1]).log().cumsum(0).exp()
    return advantage, agae, agae + vt[:-1], weight


@pytest.mark.parametrize('term', ['inside', 'zero', 'one'])
@pytest.mark.parametrize('H,M', [(1, 1), (1, 257), (15, 300), (3, 256)])
def test_gae_losses_shapes_and_terminals(hip, H, M, term):
    """H = 1 (only the t == H - 1 branch), a ragged last block (257, 300 columns), one block exactly (256); gamma 0.99 and 1,
    lambda 0, 0.95 and 1; terminal strictly inside (0, 1), exactly 0, and exactly 1.0 at one step per column (what an fp32 sigmoid
    gives above about 17): the reality weight is 0 from that step on and stays 0, nothing is NaN, advantage and target stay
    finite.  fp64 restatement and bars of test_gae_and_ac_losses."""
    J = H + 1
    g = _gen(100 * H + M)
    reward = torch.randn(J, M, generator=g)
    value_t = torch.randn(J, M, generator=g)
    if term == 'inside':
        terminal = torch.sigmoid(torch.randn(J, M, generator=g) - 3)
    elif term == 'zero':
        terminal = torch.zeros(J, M)
    else:
        terminal = torch.sigmoid(torch.randn(J, M, generator=g) - 3)
        at = torch.arange(M) % J
        terminal[at, torch.arange(M)] = 1.0
    d_reward, d_terminal, d_value_t = reward.to(DEV), terminal.to(DEV), value_t.to(DEV)
    for gamma in (0.99, 1.0):
        for lam in (0.0, 0.95, 1.0):
            outs = [torch.full((H, M), NAN, device=DEV) for _ in range(4)]
            hip.call('dm_gae_losses', H, M, gamma, lam, hip.fptr(d_reward), hip.fptr(d_terminal), hip.fptr(d_value_t),
                     *[hip.fptr(o) for o in outs], hip.stream())
            adv, agae, vtgt, wgt = outs
            for o in outs:
                assert bool(torch.isfinite(o).all()), (gamma, lam)
            r_adv, r_agae, r_vtgt, r_w = _gae_ref(H, gamma, lam, reward, terminal, value_t)
            what = f'gamma {gamma} lambda {lam}'
            _close(adv, r_adv, 1e-5, 1e-5, 'advantage ' + what)
            _close(agae, r_agae, 1e-5, 2e-5, 'advantage_gae ' + what)
            _close(vtgt, r_vtgt, 1e-5, 2e-5, 'value_target ' + what)
            _close(wgt, r_w, 1e-5, 1e-6, 'reality weight ' + what)
            if term == 'zero':
                assert bool((wgt == 1.0).all())
            if term == 'one':
                dead = torch.arange(H).unsqueeze(1) >= at.unsqueeze(0)           # steps from the saturated one on
                assert bool((wgt.cpu()[dead] == 0.0).all()) and bool((wgt.cpu()[~dead] > 0.0).all())


def _actor_case(rows, A, saturated):
    g = _gen(31 * A + rows)
    logits = torch.randn(rows, A, generator=g)
    if saturated:
        logits = logits + 80.0 * (2.0 * torch.randint(0, 2, (rows, A), generator=g).float() - 1.0)
        logits[0] = -80.0                       # one row entirely at the bottom, one at the top: uniform policies
        logits[-1] = 80.0
    act = torch.randint(0, A, (rows,), generator=g)
    act[-1] = A - 1
    if rows > 1:
        act[0] = 0
    adv = torch.randn(rows, generator=g)
    wgt = torch.rand(rows, generator=g)
    return logits, act, adv, wgt


def _actor_ref(logits, act, adv, wgt, ent_w, dtype):
    """a2c.py:119-130 restated with torch.distributions in `dtype`: (loss rows, entropy rows, d mean(loss) / d logits)"""
    import torch.distributions as D
    lg = logits.detach().clone().to(dtype).requires_grad_(True)
    dist = D.OneHotCategorical(logits=lg)
    la = (-dist.log_prob(F.one_hot(act, logits.shape[1]).to(dtype)) * adv.to(dtype) - ent_w * dist.entropy()) * wgt.to(dtype)
    la.mean().backward()
    return la.detach(), dist.entropy().detach(), lg.grad


# Logits +-80: where the fp32 CPU restatement (_actor_ref in float32) itself misses the bars against fp64, measured on the CPU for
# exactly these inputs as (its max abs error, its worst error / bar).  Every other +-80 combination meets the bars (worst ratio
# 0.93 at A 2, 257 rows, loss; 0.67 at A 18 and 65) and keeps them.
PM80_RESTATEMENT_MISSES = {
    (2, 257, 'entropy'): (3.7e-6, 1.66),
    (2, 4500, 'loss'): (3.5e-5, 3.5),
    (2, 4500, 'entropy'): (3.9e-6, 2.6),
    (2, 4500, 'dlogits'): (1.9e-9, 4.1),
}


@pytest.mark.parametrize('saturated', [False, True], ids=['unit', 'pm80'])
@pytest.mark.parametrize('rows', [1, 257, 4500])
@pytest.mark.parametrize('A', [1, 2, 18, 65])
def test_actor_loss_shapes_and_optional_outputs(hip, A, rows, saturated):
    """A 1, 2, 18, 65 at 1, 257 (ragged block) and 4500 rows; action index 0 and A - 1; with loss, entropy and dlogits each NULL in
    turn the other outputs keep their bits.  fp64 restatement and bars of test_gae_and_ac_losses: loss and entropy (1e-5, 1e-6),
    dlogits (1e-4, 1e-10).

    Logits +-80 (+ randn): everything finite, and the same bars - except in the four (A, rows, output) combinations of
    PM80_RESTATEMENT_MISSES, all at A = 2, where the reference's own fp32 restatement (torch.distributions, log pi = x -
    logsumexp(x) with the logsumexp rounded at |x| = 80: half an ulp is 3.8e-6) misses them; those four allow the bar or 4x that
    restatement's max error for the same inputs (computed here, from the reference alone), whichever is larger."""
    ent_w = 1e-3
    logits, act, adv, wgt = _actor_case(rows, A, saturated)
    dl, da, dadv, dw = logits.to(DEV), act.int().to(DEV), adv.to(DEV), wgt.to(DEV)

    def run(loss=True, entropy=True, dlogits=True):
        o = [torch.full((rows,), NAN, device=DEV) if loss else None, torch.full((rows,), NAN, device=DEV) if entropy else None,
             torch.full((rows, A), NAN, device=DEV) if dlogits else None]
        hip.call('dm_actor_loss', rows, A, hip.fptr(dl), hip.ptr(da), hip.fptr(dadv), hip.fptr(dw), ent_w, 1.0 / rows, hip.fptr(o[0]),
                 hip.fptr(o[1]), hip.fptr(o[2]), hip.stream())
        return o
    full = run()
    ref64 = _actor_ref(logits, act, adv, wgt, ent_w, torch.float64)
    ref32 = _actor_ref(logits, act, adv, wgt, ent_w, torch.float32)
    for name, o, r64, r32, (rtol, atol) in zip(('loss', 'entropy', 'dlogits'), full, ref64, ref32, ((1e-5, 1e-6), (1e-5, 1e-6), (1e-4, 1e-10))):
        assert bool(torch.isfinite(o).all()), name
        err = (o.double().cpu() - r64).abs()
        e32 = float((r32.double() - r64).abs().max())
        tol = atol + rtol * r64.abs()
        print(f'actor A={A} rows={rows} saturated={saturated} {name}: max err {float(err.max()):.3e}, worst err / bar '
              f'{float((err / tol).max()):.2f}, fp32 restatement {e32:.3e}')
        if saturated and (A, rows, name) in PM80_RESTATEMENT_MISSES:
            tol = tol.clamp(min=4 * e32)
        bad = ~(err <= tol)
        assert not bad.any(), f'{name}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e}, fp32 restatement {e32:.3e}'
    for skip in range(3):
        part = run(*[i != skip for i in range(3)])
        for i in range(3):
            assert part[i] is None if i == skip else _same_bits(part[i], full[i]), (skip, i)


@pytest.mark.parametrize('rows', [1, 257, 4500])
def test_critic_loss_optional_outputs(hip, rows):
    """One row, a ragged block and several blocks; with `loss` NULL and with `dvalue` NULL the other output keeps its bits.  fp64
    restatement and bars of test_gae_and_ac_losses."""
    g = _gen(rows)
    value, vtgt, wgt = torch.randn(rows, generator=g), torch.randn(rows, generator=g), torch.rand(rows, generator=g)
    dv, dt, dw = value.to(DEV), vtgt.to(DEV), wgt.to(DEV)

    def run(loss=True, dvalue=True):
        o = [torch.full((rows,), NAN, device=DEV) if loss else None, torch.full((rows,), NAN, device=DEV) if dvalue else None]
        hip.call('dm_critic_loss', rows, hip.fptr(dv), hip.fptr(dt), hip.fptr(dw), 1.0 / rows, hip.fptr(o[0]), hip.fptr(o[1]), hip.stream())
        return o
    full = run()
    v = value.double().requires_grad_(True)
    lc = 0.5 * (vtgt.double() - v) ** 2 * wgt.double()
    lc.mean().backward()
    _close(full[0], lc, 1e-5, 1e-6, 'critic loss')
    _close(full[1], v.grad, 1e-5, 1e-10, 'critic dvalue')
    only_d, only_l = run(loss=False), run(dvalue=False)
    assert only_d[0] is None and _same_bits(only_d[1], full[1])
    assert only_l[1] is None and _same_bits(only_l[0], full[0])


def test_multi_sum_modes_mixed(hip):
    """32 items in one launch, modes 0 (scale sum x), 1 (scale sum (x - c)^2) and 2 (its square root) mixed, n 1, 255 and 37 500,
    plus n = 0 items with a NULL pointer (allowed: 0 in every mode).  fp64 reference, test_multi_sum's bars (1e-5, 1e-6)."""
    sizes = [1, 255, 37500, 0]
    items = (hip.dm_reduce_item * 32)()
    keep, ref = [], []
    for i in range(32):
        n, mode = sizes[i % 4], (i // 4) % 3
        x = (torch.randn(n, generator=_gen(i)) * (1 + i % 5) + 0.3 * i).to(DEV) if n else None
        c = torch.full((1,), float(x.mean()) if n > 1 else 0.25, device=DEV)
        scale = 1.0 / max(n - (1 if mode else 0), 1)
        keep += [x, c]
        items[i].x = x.data_ptr() if n else None
        items[i].n = n
        items[i].scale = scale
        items[i].mode = mode
        items[i].center = c.data_ptr() if mode else None
        xd = x.double().cpu() if n else torch.zeros(0, dtype=torch.float64)
        s = xd.sum() if mode == 0 else ((xd - float(c)) ** 2).sum()
        s = s * float(torch.tensor(scale, dtype=torch.float32))
        ref.append(s.sqrt() if mode == 2 else s)
    out = torch.full((32,), NAN, device=DEV)
    hip.call('dm_multi_sum', 32, items, hip.fptr(out), hip.stream())
    assert bool(torch.isfinite(out).all())
    assert all(float(out[i]) == 0.0 for i in range(32) if sizes[i % 4] == 0)
    _close(out, torch.stack(ref), 1e-5, 1e-6, 'multi_sum modes 0 / 1 / 2')


# ------------------------------------------------------------------------------------------- optimizer
def _grad(n, seed, scale):
    g = torch.randn(n, generator=_gen(seed))
    return (g + 0.5 * torch.sign(g)) * scale           # |g| >= 0.5 scale: which steps clip does not depend on the draw, even at n = 1


@pytest.mark.parametrize('step0', [1, 1000])
@pytest.mark.parametrize('weight_decay', [0.0, 0.1])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4097, 5_000_003])
def test_norm_clip_adamw_sizes(hip, n, weight_decay, step0):
    """Three AdamW steps with clipping against torch.optim.AdamW + clip_grad_norm_ at test_norm_clip_adamw's bars: n below one
    float4 (1, 3), exactly one (4), with a tail (5, 1023, 4097) and 5 000 003 - past the block caps of all three kernels (1024
    x 4096, 2048 x 1024 and 4096 x 1024 elements), so their grid-stride loops run, with a non-zero n & 3 tail; weight decay 0 and
    0.1; step counts 1..3 and 1000..1002 (moments carried in); the middle step clips, the others do not."""
    max_norm = 0.5 * n ** 0.5
    p0 = torch.randn(n, generator=_gen(1))
    m0 = torch.zeros(n) if step0 == 1 else 0.05 * torch.randn(n, generator=_gen(2))
    v0 = torch.zeros(n) if step0 == 1 else 0.01 * torch.rand(n, generator=_gen(3))
    ref_p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref_p], lr=3e-4, eps=1e-5, weight_decay=weight_decay)
    if step0 > 1:
        opt.state[ref_p] = dict(step=torch.tensor(float(step0 - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    clipped = []
    m64, v64 = m0.double(), v0.double()
    for k in range(3):
        step = step0 + k
        gcpu = _grad(n, 10 + k, 3.0 if k == 1 else 0.05)
        g64 = gcpu.double() * min(1.0, max_norm / (float(gcpu.double().norm()) + 1e-6))
        m64, v64 = m64 + (g64 - m64) * (1 - 0.9), v64 * 0.999 + (1 - 0.999) * g64 * g64
        ref_p.grad = gcpu.clone()
        total = torch.nn.utils.clip_grad_norm_([ref_p], max_norm)
        opt.step()
        g = gcpu.to(DEV)
        norm = torch.full((2,), NAN, device=DEV)
        hip.call('dm_multi_tensor_norm_clip', hip.fptr(g), n, max_norm, hip.fptr(norm), hip.ptr(ws), ws.numel(), hip.stream())
        hip.call('dm_scale_inplace', hip.fptr(g), n, ctypes.c_void_p(norm.data_ptr() + 4), hip.stream())
        hip.call('dm_adamw_step', hip.fptr(p), hip.fptr(g), hip.fptr(m), hip.fptr(v), n, 3e-4, 0.9, 0.999, 1e-5, weight_decay, step,
                 None, hip.stream())
        clipped.append(float(norm[1]) < 1.0)
        _close(norm[0], gcpu.double().norm(), 2e-6, 0, 'grad norm vs fp64')
        _close(norm[0], total, 1e-4, 0, 'grad norm vs torch fp32')
        _close(norm[1], torch.clamp(max_norm / (gcpu.double().norm() + 1e-6), max=1.0), 1e-5, 0, 'clip coefficient')
        _close(g, ref_p.grad, 1e-4, 1e-9, 'clipped grad')
        _close(p, ref_p.detach(), 2e-6, 2e-7, f'adamw step {step}')
    assert clipped == [False, True, False]
    # the moments against their fp64 restatement (torch's own carry the rounding of its fp32 norm), norm-wise: three fp32
    # roundings per step for exp_avg.  exp_avg_sq also carries the ABI's float beta2: 1 - beta2 is formed from 0.999f, half an ulp
    # of which (2^-25) is 3.0e-5 of 0.001
    em, ev = _rel_l2(m, m64), _rel_l2(v, v64)
    print(f'adamw n={n} step0={step0}: exp_avg {em:.3e} exp_avg_sq {ev:.3e}')
    assert em < 1e-6 and ev < 3.0e-5 + 1e-6, (em, ev)


@pytest.mark.parametrize('n', [5, 4097, 5_000_003])
def test_adamw_clip_coef_pointer_is_scale_then_step(hip, n):
    """dm_adamw_step with the coefficient read from device memory gives the BITS of dm_scale_inplace followed by the NULL form
    (parameters and both moments), and leaves the gradient alone."""
    p0, g0 = torch.randn(n, generator=_gen(1)).to(DEV), torch.randn(n, generator=_gen(2)).to(DEV)
    m0, v0 = (0.05 * torch.randn(n, generator=_gen(3))).to(DEV), (0.01 * torch.rand(n, generator=_gen(4))).to(DEV)
    coef = torch.tensor([0.37], device=DEV)
    args = (3e-4, 0.9, 0.999, 1e-5, 0.01, 7)
    pa, ga, ma, va = p0.clone(), g0.clone(), m0.clone(), v0.clone()
    hip.call('dm_scale_inplace', hip.fptr(ga), n, hip.fptr(coef), hip.stream())
    assert torch.equal(ga, g0 * 0.37)
    hip.call('dm_adamw_step', hip.fptr(pa), hip.fptr(ga), hip.fptr(ma), hip.fptr(va), n, *args, None, hip.stream())
    pb, gb, mb, vb = p0.clone(), g0.clone(), m0.clone(), v0.clone()
    hip.call('dm_adamw_step', hip.fptr(pb), hip.fptr(gb), hip.fptr(mb), hip.fptr(vb), n, *args, hip.fptr(coef), hip.stream())
    assert torch.equal(gb, g0)
    for name, a, b in (('param', pa, pb), ('exp_avg', ma, mb), ('exp_avg_sq', va, vb)):
        assert _same_bits(a, b), f'{name}: {int((_bits(a) != _bits(b)).sum())} of {n} elements differ'
    assert not torch.equal(pa, p0)


@pytest.mark.parametrize('n', [3, 4097])
def test_zero_gradient_gives_norm_zero_and_coefficient_one(hip, n):
    """An all-zero gradient: norm 0, coefficient 1 (max_norm / 1e-6 clamped), and a step with that coefficient read from device
    memory moves the parameters as torch does (weight decay alone, moments stay 0)."""
    p0 = torch.randn(n, generator=_gen(1))
    ref_p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref_p], lr=3e-4, eps=1e-5, weight_decay=0.01)
    ref_p.grad = torch.zeros(n)
    torch.nn.utils.clip_grad_norm_([ref_p], 100.0)
    opt.step()
    p, g, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    norm = torch.full((2,), NAN, device=DEV)
    ws = torch.empty(1 << 12, dtype=torch.uint8, device=DEV)
    hip.call('dm_multi_tensor_norm_clip', hip.fptr(g), n, 100.0, hip.fptr(norm), hip.ptr(ws), ws.numel(), hip.stream())
    assert norm.tolist() == [0.0, 1.0]
    hip.call('dm_adamw_step', hip.fptr(p), hip.fptr(g), hip.fptr(m), hip.fptr(v), n, 3e-4, 0.9, 0.999, 1e-5, 0.01, 1,
             ctypes.c_void_p(norm.data_ptr() + 4), hip.stream())
    assert bool(torch.isfinite(p).all()) and bool((m == 0).all()) and bool((v == 0).all())
    _close(p, ref_p.detach(), 2e-6, 2e-7, 'adamw on a zero gradient')


def test_norm_clip_refusals(hip):
    """A gradient pointer 4 bytes off 16-byte alignment: DM_E_SHAPE; a workspace below one float per block: DM_E_WORKSPACE.
    Both before any launch: the norm buffer keeps its sentinel."""
    n = 3 * 4096 + 1                                   # 4 blocks: 16 bytes of workspace
    g = torch.zeros(n + 1, device=DEV)
    norm = _sentinel(2)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    lib = hip.lib()
    assert lib.dm_multi_tensor_norm_clip(ctypes.c_void_p(g.data_ptr() + 4), n, 1.0, hip.fptr(norm), hip.ptr(ws), 64, hip.stream()) == DM_E_SHAPE
    assert lib.dm_multi_tensor_norm_clip(hip.fptr(g), n, 1.0, hip.fptr(norm), hip.ptr(ws), 15, hip.stream()) == DM_E_WORKSPACE
    assert lib.dm_multi_tensor_norm_clip(hip.fptr(g), n, 1.0, hip.fptr(norm), None, 64, hip.stream()) == DM_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((_bits(norm) == SENT).all())
    assert lib.dm_multi_tensor_norm_clip(hip.fptr(g), n, 1.0, hip.fptr(norm), hip.ptr(ws), 16, hip.stream()) == 0
    assert norm.tolist() == [0.0, 1.0]


@pytest.mark.parametrize('n', [1, 1000, 2_100_001])
def test_axpby_b_zero_ignores_y(hip, n):
    """y = a x + b y with b = 0 and NaN in y leaves no NaN (the kernel does not multiply y by 0); 2 100 001 is past the block
    cap (2048 x 1024 elements): the grid-stride loop runs."""
    x = torch.randn(n, generator=_gen(n)).to(DEV)
    y = torch.full((n,), NAN, device=DEV)
    hip.call('dm_axpby', n, 2.5, hip.fptr(x), 0.0, hip.fptr(y), hip.stream())
    assert torch.equal(y, 2.5 * x)
    y0 = torch.randn(n, generator=_gen(n + 1)).to(DEV)
    y = y0.clone()
    hip.call('dm_axpby', n, 2.5, hip.fptr(x), -0.5, hip.fptr(y), hip.stream())
    _close(y, 2.5 * x.double() - 0.5 * y0.double(), 1e-6, 1e-6, 'axpby')
