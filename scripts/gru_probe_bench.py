"""Timings of the GRU probe baseline -> profiles/gru_probe_bench.txt.

    python scripts/gru_probe_bench.py                 # both parts
    python scripts/gru_probe_bench.py --composed-only # part 2's composed pair alone: uses only dm_gemm_f32 and dm_gru_gates_fwd,
                                                      # so it also runs on a build that has no dm_gru_sequence_ entry points

Part 1: WorldModelProbe step time (forward + backward + grad_clip + optimizer) at `defaults` + `miniworld` with
probe_model='map+goals', goals_size=3, B 32, T 48 - with the library's own dispatch (what a trainer gets) and with
dm_gru_sequence_fuse_enable(2), the one-launch step forced at this width.

Part 2: per-step time of the recurrent forward step at D in {600, 1024, 2048}, B in {32, 50}, three columns:
  composed pair   - 192 x [dm_gemm_f32(h W_hh^T + b_hh), dm_gru_gates_fwd] from this script;
  library default - dm_gru_sequence_fwd (acts = NULL) as the library dispatches it (the schedule it reports is printed);
  one-launch step - the same call under dm_gru_sequence_fuse_enable(2), which dispatches gru_step_kernel at every width.
Both sequence columns are  [(t(T=200) - gi(T=200)) - (t(T=8) - gi(T=8))] / 192:  the call timed at two lengths minus its batched
input product GI = X W_ih^T + b_ih timed alone through the same entry at the same lengths (it grows with T too), i.e. the cost of
one recurrent step; the input product's own share per step is printed at the end of the line.
Every timed region is enqueued behind a ~10 ms matmul, so the host's launch loop runs ahead of the GPU and HIP events see device
time only.  Three repeats each, (min, median, max) in microseconds per step.
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydreamer_amd import hip as H                # noqa: E402

DEV = 'cuda'
STEPS = 192
DM_SPLITK_BYTES = 64 * 1024 * 1024      # the split-K scratch the sequence call hands its products (csrc/common.h DM_SPLITK_FLOATS)


def _behind_busy_gpu(fn, busy):
    """Device milliseconds of fn(), enqueued while the GPU is still busy with a large matmul."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.mm(busy, busy)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _stats(xs):
    xs = sorted(xs)
    return f'{xs[0]:8.2f} {xs[len(xs) // 2]:8.2f} {xs[-1]:8.2f}'


def step_pair(D, B, busy, composed_only):
    In = 32 + 3
    g = torch.Generator().manual_seed(D + B)
    k = D ** -0.5
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * k).to(DEV)
    w_ih, w_hh, b_ih, b_hh = u(3 * D, In), u(3 * D, D), u(3 * D), u(3 * D)
    h0 = torch.randn(B, D, generator=g).to(DEV)
    out = {}
    # composed: the pair the parent commit has
    ws = torch.empty(64 * 1024 * 1024 + 4096, dtype=torch.uint8, device=DEV)
    gi = torch.randn(B, 3 * D, generator=g).to(DEV)
    gh = torch.empty(B, 3 * D, device=DEV)
    hs = [h0.clone(), torch.empty(B, D, device=DEV)]
    st = H.stream()

    def composed():
        for t in range(STEPS):
            a, b = hs[t & 1], hs[1 - (t & 1)]
            H.call('dm_gemm_f32', 0, 0, B, 3 * D, D, H.fptr(a), D, H.fptr(w_hh), D, H.fptr(gh), 3 * D, H.fptr(b_hh), None, 0, 0,
                   H.ptr(ws), ws.numel(), st)
            H.call('dm_gru_gates_fwd', B, D, H.fptr(gi), H.fptr(gh), H.fptr(a), D, H.fptr(b), D, st)

    composed()
    out['composed'] = [1e3 * _behind_busy_gpu(composed, busy) / STEPS for _ in range(3)]
    if composed_only:
        return out
    lib = H.lib()
    params = H.gru_struct(w_ih, w_hh, b_ih, b_hh)
    T1, T0 = STEPS + 8, 8
    x = torch.randn(T1 * B, In, generator=g).to(DEV)
    Hs = torch.empty(T1 * B, D, device=DEV)
    wsb = int(lib.dm_gru_sequence_ws_bytes(T1, B, In, D))
    ws2 = torch.empty(wsb, dtype=torch.uint8, device=DEV)

    def fused(T):
        H.call('dm_gru_sequence_fwd', T, B, In, D, H.fptr(x), In, H.fptr(h0), None, ctypes.byref(params), None, H.fptr(Hs), D,
               H.ptr(ws2), wsb, st)

    gi_all = torch.empty(T1 * B, 3 * D, device=DEV)

    def input_product(T):      # the call's batched GI = X W_ih^T + b_ih, the same product through the same entry
        H.call('dm_gemm_f32', 0, 0, T * B, 3 * D, In, H.fptr(x), In, H.fptr(w_ih), In, H.fptr(gi_all), 3 * D, H.fptr(b_ih), None, 0, 0,
               H.ptr(ws2), DM_SPLITK_BYTES, st)

    input_product(T1)
    gis = []
    for mode, key in ((1, 'default'), (2, 'forced')):
        lib.dm_gru_sequence_fuse_enable(mode)
        try:
            fused(T1)
            out['schedule_' + key] = int(lib.dm_gru_sequence_last_schedule())
            reps = []
            for _ in range(3):
                t1 = _behind_busy_gpu(lambda: fused(T1), busy)
                t0 = _behind_busy_gpu(lambda: fused(T0), busy)
                g1 = _behind_busy_gpu(lambda: input_product(T1), busy)
                g0 = _behind_busy_gpu(lambda: input_product(T0), busy)
                reps.append(1e3 * ((t1 - g1) - (t0 - g0)) / STEPS)
                gis.append(1e3 * (g1 - g0) / STEPS)
            out[key] = reps
        finally:
            lib.dm_gru_sequence_fuse_enable(1)
    out['gi'] = gis
    return out


def model_step(mode, steps=10, warmup=3):
    H.lib().dm_gru_sequence_fuse_enable(mode)
    from pydreamer_amd import config
    from pydreamer_amd.models import WorldModelProbe
    conf = config.load_config('defaults', 'miniworld', model='gru_probe', probe_gradients=True, probe_model='map+goals', goals_size=3,
                              batch_size=32, batch_length=48)
    torch.manual_seed(0)
    model = WorldModelProbe(conf).to(DEV)
    opts = model.init_optimizers(conf.adam_lr, eps=conf.adam_eps)
    T, B, A, G, S, C = conf.batch_length, conf.batch_size, conf.action_dim, conf.goals_size, conf.map_size, conf.map_channels
    g = torch.Generator().manual_seed(1)
    obs = dict(image=torch.randint(0, 256, (T, B, 64, 64, 3), generator=g, dtype=torch.uint8),
               action_next=torch.nn.functional.one_hot(torch.randint(0, A, (T, B), generator=g), A).float(),
               reward=torch.randn(T, B, generator=g), terminal=torch.zeros(T, B), reset=torch.zeros(T, B, dtype=torch.bool),
               map=torch.randint(0, C, (T, B, S, S), generator=g), map_coord=torch.randn(T, B, 4, generator=g),
               map_seen_mask=torch.randint(0, 2, (T, B, S, S), generator=g),
               goal_direction=torch.randn(T, B, 2, generator=g), goals_direction=torch.randn(T, B, 2 * G, generator=g),
               goals_visage=torch.randint(0, 300, (T, B, G), generator=g).float())
    obs = {k: v.to(DEV) for k, v in obs.items()}
    state = model.init_state(B)
    times = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        losses, state, _, _, _ = model.training_step(obs, state)
        for o in opts:
            o.zero_grad()
        losses[0].backward()
        model.grad_clip(conf.grad_clip)
        for o in opts:
            o.step()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    sched = int(H.lib().dm_gru_sequence_last_schedule())
    H.lib().dm_gru_sequence_fuse_enable(1)
    n = sum(p.numel() for p in model.parameters())
    print(f'WorldModelProbe gru_probe, defaults + miniworld, map+goals, goals_size 3, B {B}, T {T}, deter {conf.deter_dim}, {n} parameters, '
          f'dm_gru_sequence_fuse_enable({mode}) -> schedule {sched}')
    print(f'  step (forward + backward + clip + AdamW), ms over {steps} steps: min med max = {_stats(times)}   loss {float(losses[0].detach()):.5f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--composed-only', action='store_true')
    args = ap.parse_args()
    H.call('dm_device_check')
    if not args.composed_only:
        model_step(1)
        model_step(2)
    busy = torch.randn(8192, 8192, device=DEV)
    print(f'recurrent forward step, us per step over {STEPS} steps, three repeats: min med max')
    for D in (600, 1024, 2048):
        for B in (32, 50):
            r = step_pair(D, B, busy, args.composed_only)
            line = f'  D {D:5d} B {B:3d}  composed pair {_stats(r["composed"])}'
            if 'default' in r:
                line += (f'   library default {_stats(r["default"])} (schedule {r["schedule_default"]})   one-launch step {_stats(r["forced"])} '
                         f'(schedule {r["schedule_forced"]})   input product {_stats(r["gi"])}')
            print(line)


if __name__ == '__main__':
    main()
