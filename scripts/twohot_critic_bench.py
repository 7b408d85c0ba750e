"""Cost of the two-hot critic and the percentile return normalisation -> profiles/twohot_critic_bench.txt.

    python scripts/twohot_critic_bench.py [--out FILE] [--steps 20] [--warmup 8] [--reps 3] [--kernel-calls 50]

1  The three kernels of csrc/twohot.hip alone at the Atari-literal step's shape (B 50, T 50, H 15: 40 000 imagined rows, 37 500
   loss rows), device events around `--kernel-calls` back-to-back calls, each against the torch composition it replaces on the same
   inputs: dm_twohot_decode 40 000 x 255 against softmax . bins + expm1; dm_twohot_loss against log_softmax + gather (+ the
   two-hot weights and the softmax-minus-target gradient); dm_return_norm (n 37 500) against torch.quantile + EMA + divide.
2  The whole Atari-literal training step (bench.py's loop: training_step, zero_grad, four backward passes, clip, AdamW) with the
   defaults, critic_dist='twohot' at 255 and at 32 bins, and return_norm='percentile': each variant in a fresh child process of
   its own (one model per process, one process at a time), `--rounds` alternating rounds, in each a warm-up and `--reps` blocks
   of `--steps` steps between device synchronisations; per variant (min, median, max) over all its blocks of the host
   milliseconds per step.  The same step on the parent commit is bench.py's own figure, taken in the same GPU visit and appended
   to the profile by hand.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import GlobalNoise, make_ring                  # noqa: E402
from pydreamer_amd import config, hip as H                # noqa: E402
from pydreamer_amd.models import Dreamer                  # noqa: E402

DEV = 'cuda'


def events_ms(fn, calls):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def symlog(x):
    return torch.sign(x) * torch.log1p(x.abs())


def kernels(calls, lines):
    rows_total, rows, K = 40000, 37500, 255
    g = torch.Generator(device=DEV).manual_seed(0)
    logits = torch.randn(rows_total, K, device=DEV, generator=g) * 3
    bins = torch.linspace(-20.0, 20.0, K, device=DEV)
    target, weight = torch.randn(rows, device=DEV, generator=g) * 100, torch.rand(rows, device=DEV, generator=g)
    value, loss, dlogits = torch.empty(rows_total, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows_total, K, device=DEV)
    decode = lambda: H.call('dm_twohot_decode', rows_total, K, H.fptr(logits), K, H.fptr(bins), H.fptr(value), H.stream())
    t_decode = lambda: torch.sign(m := (torch.softmax(logits, -1) * bins).sum(-1)) * torch.expm1(m.abs())
    a, b = events_ms(decode, calls), events_ms(t_decode, calls)
    err = float(((value - t_decode()).abs() / (1 + value.abs())).max())
    lines.append(f'dm_twohot_decode {rows_total} x {K}: {1e3 * a:.1f} us, torch softmax . bins + expm1 {1e3 * b:.1f} us (x {b / a:.1f}; '
                 f'max difference relative to 1 + |v| {err:.1e})')
    print(lines[-1], flush=True)
    lossk = lambda: H.call('dm_twohot_loss', rows, rows_total, K, H.fptr(logits), K, H.fptr(bins), H.fptr(target), H.fptr(weight),
                           1.0 / rows, H.fptr(loss), H.fptr(dlogits), None, H.stream())

    def t_loss():
        x = symlog(target).clamp(bins[0], bins[-1])
        k = ((bins[None, :] <= x[:, None]).sum(-1) - 1).clamp(0, K - 2)
        w_hi = (x - bins[k]) / (bins[k + 1] - bins[k])
        lsm = torch.log_softmax(logits[:rows], -1)
        out = -weight * ((1 - w_hi) * lsm.gather(-1, k[:, None])[:, 0] + w_hi * lsm.gather(-1, (k + 1)[:, None])[:, 0])
        d = torch.zeros(rows_total, K, device=DEV)
        d[:rows] = lsm.exp()
        d[:rows].scatter_add_(-1, k[:, None], -(1 - w_hi)[:, None]).scatter_add_(-1, (k + 1)[:, None], -w_hi[:, None])
        d[:rows] *= (weight / rows)[:, None]
        return out, d
    a, b = events_ms(lossk, calls), events_ms(t_loss, calls)
    tl, td = t_loss()
    lines.append(f'dm_twohot_loss {rows} of {rows_total} rows x {K} (loss + dlogits): {1e3 * a:.1f} us, torch log_softmax + gather + '
                 f'scatter {1e3 * b:.1f} us (x {b / a:.1f}; max differences: loss {float((loss - tl).abs().max()):.1e}, dlogits '
                 f'{float((dlogits - td).abs().max()):.1e})')
    print(lines[-1], flush=True)
    x, adv0 = torch.randn(rows, device=DEV, generator=g) * 5, torch.randn(rows, device=DEV, generator=g)
    state, out, adv = torch.zeros(2, device=DEV), torch.empty(5, device=DEV), adv0.clone()
    norm = lambda: H.call('dm_return_norm', rows, H.fptr(x), 0.05, 0.95, 0.99, 1.0, 1, H.fptr(state), H.fptr(out), H.fptr(adv), rows,
                          H.stream())
    q, tstate = torch.tensor([0.05, 0.95], device=DEV), torch.zeros(2, device=DEV)

    def t_norm():
        p = torch.quantile(x, q)
        tstate.mul_(0.99).add_(0.01 * p)
        return adv0 / torch.clamp(tstate[1] - tstate[0], min=1.0)
    a, b = events_ms(norm, calls), events_ms(t_norm, calls)
    state.zero_()
    norm()
    pq = torch.quantile(x, q)
    lines.append(f'dm_return_norm n {rows} (two percentiles, EMA, {rows} divisions; 2 launches): {1e3 * a:.1f} us, torch.quantile + EMA + '
                 f'divide {1e3 * b:.1f} us (x {b / a:.1f}; percentiles differ by {float((out[:2] - pq).abs().max()):.1e})')
    print(lines[-1], flush=True)


def trainer(**switches):
    conf = config.atari_literal(**switches)
    torch.manual_seed(0)
    model = Dreamer(conf).to(DEV)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    B = conf.batch_size
    ring, noise = make_ring(conf, B, 0, B, 4, torch.device(DEV), 1234), GlobalNoise(conf, B, 0, B, torch.device(DEV), 777)
    state = {'s': model.init_state(B), 'i': 0}

    def step():
        losses, state['s'], _, _, _ = model.training_step(ring[state['i'] % len(ring)], state['s'], noise=noise.draw())
        state['i'] += 1
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in opts:
            opt.step()
    return step


def block(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


VARIANTS = dict(defaults={}, twohot_255=dict(critic_dist='twohot', critic_bins=255), twohot_32=dict(critic_dist='twohot', critic_bins=32),
                percentile=dict(return_norm='percentile'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'twohot_critic_bench.txt'))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--kernel-calls', type=int, default=50)
    ap.add_argument('--variant', default='', help='(internal) time this one variant in this process and print its block times')
    args = ap.parse_args()
    if args.variant:
        step = trainer(**VARIANTS[args.variant])
        block(step, args.warmup)
        print('BLOCKS ' + json.dumps([block(step, args.steps) for _ in range(args.reps)]), flush=True)
        return
    # One model per process: with all four models in one process the variants built second and fourth (twohot_255 and
    # percentile, the latter one 44 us call away from the defaults) measured +19 ms (supposed: a model's side streams take hardware queues when they are created and a second model's share them, so
    # its backward passes no longer overlap).  The variants run in fresh child processes, one at a time, alternating.
    times = {k: [] for k in VARIANTS}
    for _ in range(args.rounds):
        for k in VARIANTS:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--variant', k, '--steps', str(args.steps), '--warmup',
                                  str(args.warmup), '--reps', str(args.reps)], check=True, capture_output=True, text=True, timeout=300).stdout
            times[k] += json.loads(next(l for l in out.splitlines() if l.startswith('BLOCKS '))[7:])
    H.call('dm_device_check')
    lines = [f'two-hot critic and percentile return normalisation, {torch.cuda.get_device_name(0)}',
             f'kernels alone at the Atari-literal step\'s shape, device events, {args.kernel_calls} calls each:']
    kernels(args.kernel_calls, lines)
    lines.append(f'Atari-literal training step (B 50, T 50, H 15, fp32), host milliseconds per step; one process per variant, '
                 f'{args.rounds} alternating rounds of {args.reps} blocks of {args.steps} steps after {args.warmup} warm-up steps: min median max')
    base = sorted(times['defaults'])[len(times['defaults']) // 2]
    for k, v in times.items():
        med = sorted(v)[len(v) // 2]
        lines.append(f'  {k:<11} {min(v):8.3f} {med:8.3f} {max(v):8.3f}   {med - base:+7.3f} ms against the defaults')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
