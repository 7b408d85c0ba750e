"""-m gpu: dm_gru_sequence_fwd / _bwd (csrc/gru_seq.hip) through the C-ABI against an fp64 restatement of torch.nn.GRU.

Reference: the GRU written out in torch (gate order r, z, n; h_0 = h0 * !reset0), run in float64 with autograd on the same fp32
inputs.  Loss: sum(H * P) with a random projection P that is zero at some steps, so dH = P.

Bar, per output tensor (H, dX, dW_ih, dW_hh, db_ih, db_hh): max-norm error <= 4 x the max-norm error of the SAME restatement run
in plain torch fp32 on the CPU against the fp64 one (computed here, per case), with a floor of 2^-23 * max|ref|.  Why 4: two fp32
summation orders on the CPU (plain, and K in reversed chunks of 16) differ from each other by a factor 0.58 .. 1.36 in that error
over five shapes up to T 48, D 1024 (errors 1e-7 .. 6e-7 of max|ref|); the MFMA's k-ordered chain with its 8-way split is a
third order.  Each tensor prints a `[tol]` line with err / bar.

Exact demands (bits): a row with reset0 set equals the same call with that row of h0 zeroed; acts == NULL gives the same H;
a second forward + backward into the SAME buffers (which then hold the first call's results, not NaN) gives the same bits in
every output - the overwrite convention of include/dreamer_hip.h; the guard words behind and between the rows of every output
are untouched.  Every case names the schedule the call must report (CASES).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (T, B, In, D, dm_gru_sequence_fuse_enable mode, the schedule the call must report).  Mode 1 is the default dispatch: the one-launch
# step for B <= 64 up to D = 144, the composed pair above - D 132 / 140 / 144 are the widths at which every wave of
# the kernel's 8-way K split has work and the second accumulator of waves 0 (and 1) is live (9 chunks of 16).  Mode 2 dispatches
# the one-launch step at every width: the issue's wide cases run on BOTH schedules.  Mode 0: the pair at a narrow width.
CASES = [(1, 1, 33, 4, 1, 1), (2, 3, 38, 20, 1, 1), (5, 3, 38, 64, 1, 1), (4, 33, 50, 72, 1, 1),
         (3, 16, 35, 132, 1, 1), (3, 17, 35, 140, 1, 1), (3, 64, 50, 144, 1, 1),
         (3, 16, 35, 200, 1, 0), (3, 17, 35, 200, 1, 0), (3, 64, 50, 600, 1, 0), (3, 65, 50, 64, 1, 0), (6, 50, 50, 1024, 1, 0),
         (3, 16, 35, 200, 2, 1), (3, 17, 35, 200, 2, 1), (3, 64, 50, 600, 2, 1), (6, 50, 50, 1024, 2, 1), (3, 65, 50, 64, 2, 0),
         (5, 3, 38, 64, 0, 0)]
PAT = 0x7FC5A5A5          # guard word (a NaN with a payload: an accidental float write cannot reproduce it)
GUARD = 256


def gru_restated(x, h0, reset0, w_ih, w_hh, b_ih, b_hh, P):
    """torch.nn.GRU (one layer, time-major) written out; returns H (T, B, D) and the gradients of sum(H * P)."""
    T = x.shape[0]
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, w_ih, w_hh, b_ih, b_hh)]
    x_, wi, wh, bi, bh = leaves
    h = h0 * (~reset0).to(h0.dtype)[:, None]
    gi = x_ @ wi.T + bi
    hs = []
    for t in range(T):
        gh = h @ wh.T + bh
        ir, iz, inn = gi[t].chunk(3, -1)
        hr, hz, hn = gh.chunk(3, -1)
        r = torch.sigmoid(ir + hr)
        z = torch.sigmoid(iz + hz)
        n = torch.tanh(inn + r * hn)
        h = (1 - z) * n + z * h
        hs.append(h)
    H = torch.stack(hs)
    (H * P).sum().backward()
    return [H.detach()] + [t.grad for t in leaves]


class Guarded:
    """rows x n floats with leading dimension ld inside a buffer of guard words; the payload starts as NaN."""

    def __init__(self, rows, n, ld, dev):
        self.rows, self.n, self.ld = rows, n, ld
        self.raw = torch.full((rows * ld + GUARD,), PAT, dtype=torch.int32, device=dev)
        self.f = self.raw.view(torch.float32)
        self.mask = torch.zeros(rows * ld + GUARD, dtype=torch.bool, device=dev)
        self.mask[:rows * ld].view(rows, ld)[:, :n] = True
        self.f[self.mask] = float('nan')

    def ptr(self):
        return ctypes.c_void_p(self.f.data_ptr())

    def value(self):
        return self.f[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.n].clone()

    def guards_intact(self):
        return bool((self.raw[~self.mask] == PAT).all())


def _inputs(T, B, In, D, seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / D ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k
    x = torch.randn(T, B, In, generator=g)
    h0 = torch.randn(B, D, generator=g) * 0.5
    reset0 = torch.zeros(B, dtype=torch.bool)
    reset0[::2] = True                              # some rows set, others left (B = 1: the one row is set)
    if B > 1:
        reset0[0] = False
        reset0[1] = True
    P = torch.randn(T, B, D, generator=g)
    if T > 1:
        P[torch.arange(T) % 2 == 1] = 0             # the loss is zero at some steps
    return x, h0, reset0, u(3 * D, In), u(3 * D, D), u(3 * D), u(3 * D), P


@pytest.mark.parametrize('T,B,In,D,mode,schedule', CASES)
def test_gru_sequence_against_fp64(hip, T, B, In, D, mode, schedule):
    assert hip.lib().dm_gru_sequence_fuse_enable(-1) == 1, 'the default dispatch'
    hip.lib().dm_gru_sequence_fuse_enable(mode)
    try:
        _case(hip, T, B, In, D, mode, schedule)
    finally:
        hip.lib().dm_gru_sequence_fuse_enable(1)


def _case(hip, T, B, In, D, mode, schedule):
    dev = torch.device('cuda')
    x, h0, reset0, w_ih, w_hh, b_ih, b_hh, P = _inputs(T, B, In, D, 100 + T + B + D)
    cpu = (x, h0, reset0, w_ih, w_hh, b_ih, b_hh, P)
    ref64 = gru_restated(*[t.double() if t.dtype == torch.float32 else t for t in cpu])
    ref32 = gru_restated(*cpu)

    N = T * B
    ldx, ldh, lddh, lddx = In + 1, D + 4, D + 8, In + 3
    xd = torch.zeros(N, ldx, device=dev)
    xd[:, :In] = x.reshape(N, In).to(dev)
    dHd = torch.full((N, lddh), float('nan'), device=dev)
    dHd[:, :D] = P.reshape(N, D).to(dev)
    h0d, r0d = h0.to(dev), reset0.to(torch.uint8).to(dev)
    W = [t.to(dev).contiguous() for t in (w_ih, w_hh, b_ih, b_hh)]
    params = hip.gru_struct(*W)
    acts = torch.full((hip.lib().dm_gru_sequence_acts_floats(T, B, In, D),), float('nan'), device=dev)
    wsb = hip.lib().dm_gru_sequence_ws_bytes(T, B, In, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    H = Guarded(N, D, ldh, dev)
    dX = Guarded(N, In, lddx, dev)
    G = [Guarded(3 * D, In, In, dev), Guarded(3 * D, D, D, dev), Guarded(1, 3 * D, 3 * D, dev), Guarded(1, 3 * D, 3 * D, dev)]
    grads = hip.dm_gru_grads()
    grads.w_ih, grads.w_hh, grads.b_ih, grads.b_hh = [g.f.data_ptr() for g in G]

    def fwd(out, h0_, r0_, acts_):
        hip.call('dm_gru_sequence_fwd', T, B, In, D, hip.fptr(xd), ldx, hip.fptr(h0_), hip.ptr(r0_), ctypes.byref(params),
                 hip.fptr(acts_), out.ptr(), ldh, hip.ptr(ws), wsb, hip.stream())

    def bwd():
        hip.call('dm_gru_sequence_bwd', T, B, In, D, hip.fptr(xd), ldx, ctypes.byref(params), hip.fptr(acts), H.ptr(), ldh,
                 hip.fptr(dHd), lddh, ctypes.byref(grads), dX.ptr(), lddx, hip.ptr(ws), wsb, hip.stream())

    outs = [H, dX] + G
    names = ['H', 'dX', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh']
    fwd(H, h0d, r0d, acts)
    sched = int(hip.lib().dm_gru_sequence_last_schedule())
    assert sched == schedule, f'T {T} B {B} D {D} mode {mode}: schedule {sched}, expected {schedule}'
    bwd()
    torch.cuda.synchronize()
    first = [o.value() for o in outs]
    for nm, o in zip(names, outs):
        assert o.guards_intact(), f'{nm}: guard words changed'

    worst = 0.0
    for nm, got, r64, r32 in zip(names, first, ref64, ref32):
        r64 = r64.reshape(got.shape)
        err = float((got.cpu().double() - r64).abs().max())
        bar = max(4.0 * float((r32.reshape(got.shape).double() - r64).abs().max()), 2.0 ** -23 * float(r64.abs().max()))
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float('inf'))      # (an all-zero reference: dW_hh from h_0 = 0 at T = 1)
        print(f'[tol] gru_sequence T{T} B{B} In{In} D{D} schedule {schedule} {nm}: err {err:.3e} bar {bar:.3e} ratio {ratio:.3f}')
        worst = max(worst, ratio)
        assert torch.isfinite(got).all(), f'{nm}: not every element was written'
        assert err <= bar, f'{nm}: err {err:.3e} > bar {bar:.3e}'
    print(f'[tol] gru_sequence T{T} B{B} In{In} D{D} schedule {schedule} worst ratio {worst:.3f}')

    # a second forward + backward into the same buffers: overwritten, bit-identical
    fwd(H, h0d, r0d, acts)
    bwd()
    torch.cuda.synchronize()
    for nm, o, a in zip(names, outs, first):
        assert torch.equal(o.value().view(torch.int32), a.view(torch.int32)), f'{nm}: second call differs'
        assert o.guards_intact(), f'{nm}: guard words changed on the second call'

    # acts == NULL: the same H
    H2 = Guarded(N, D, ldh, dev)
    fwd(H2, h0d, r0d, None)
    torch.cuda.synchronize()
    assert torch.equal(H2.value().view(torch.int32), first[0].view(torch.int32)) and H2.guards_intact()

    # reset0 rows == those rows of h0 zeroed, no reset0
    h0z = h0d.clone()
    h0z[reset0.to(dev)] = 0
    H3 = Guarded(N, D, ldh, dev)
    fwd(H3, h0z, None, None)
    torch.cuda.synchronize()
    assert torch.equal(H3.value().view(torch.int32), first[0].view(torch.int32)) and H3.guards_intact()
