"""Cost of free bits and the symlog two-hot reward head -> profiles/wm_v3_losses_bench.txt.

    python scripts/wm_v3_losses_bench.py [--out FILE] [--steps 20] [--warmup 8] [--reps 3] [--kernel-calls 50]

1  The three new entries alone at the Atari-literal step's shapes (B 50, T 50, H 15), device events around `--kernel-calls`
   back-to-back calls, each against the torch-device composition of the same results on the same inputs: dm_kl_free_fwd and
   dm_kl_free_bwd on 2 500 rows x 32 groups x 32 classes (beside dm_kl_balance_fwd / _bwd, the same kernels without the gate)
   against log_softmax / sums / clamp / where; dm_twohot_head_loss on 2 500 x 255 head rows (loss, gradient and mean) against
   log_softmax + gather + scatter, and its mean-only form on 40 000 x 255 rows against softmax . bins + expm1.
2  The whole Atari-literal training step (bench.py's loop: training_step, zero_grad, four backward passes, clip, AdamW) with the
   defaults, kl_free=1, reward_dist='twohot' at 255 and at 32 bins, and both switches on: each variant in a fresh child process
   of its own (one model per process, one process at a time), `--rounds` alternating rounds, in each a warm-up and `--reps` blocks
   of `--steps` steps between device synchronisations; per variant (min, median, max) over all its blocks of the host
   milliseconds per step.
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


def kl_kernels(calls, lines):
    rows, S, C, free, sp, sq = 2500, 32, 32, 1.0, 0.2 / 2500, 0.8 / 2500
    g = torch.Generator(device=DEV).manual_seed(0)
    post = torch.randn(rows, S * C, device=DEV, generator=g) * 0.18     # row KLs around the gate: both kinds of row
    prior = torch.randn(rows, S * C, device=DEV, generator=g) * 0.18
    kl, clip, closed, ep, eq = (torch.empty(rows, device=DEV) for _ in range(5))
    dpost, dprior = torch.empty_like(post), torch.empty_like(prior)
    fwd = lambda: H.call('dm_kl_free_fwd', rows, S, C, H.fptr(post), H.fptr(prior), free, H.fptr(kl), H.fptr(clip), H.fptr(closed),
                         H.fptr(ep), H.fptr(eq), H.stream())
    fwd0 = lambda: H.call('dm_kl_balance_fwd', rows, S, C, H.fptr(post), H.fptr(prior), H.fptr(kl), H.fptr(ep), H.fptr(eq), H.stream())
    bwd = lambda: H.call('dm_kl_free_bwd', rows, S, C, H.fptr(post), H.fptr(prior), H.fptr(closed), sp, sq, H.fptr(dpost),
                         H.fptr(dprior), H.stream())
    bwd0 = lambda: H.call('dm_kl_balance_bwd', rows, S, C, H.fptr(post), H.fptr(prior), sp, sq, H.fptr(dpost), H.fptr(dprior), H.stream())

    def t_fwd():
        lp, lq = torch.log_softmax(post.view(rows, S, C), -1), torch.log_softmax(prior.view(rows, S, C), -1)
        p, q = lp.exp(), lq.exp()
        k = (p * (lp - lq)).sum((1, 2))
        return k, torch.clamp(k, min=free), (k <= free).float(), -(p * lp).sum((1, 2)), -(q * lq).sum((1, 2))

    def t_bwd():
        lp, lq = torch.log_softmax(post.view(rows, S, C), -1), torch.log_softmax(prior.view(rows, S, C), -1)
        p, q = lp.exp(), lq.exp()
        kg = (p * (lp - lq)).sum(-1, keepdim=True)
        shut = (closed != 0).view(rows, 1, 1)
        return (torch.where(shut, 0.0, sp * p * ((lp - lq) - kg)).view(rows, -1), torch.where(shut, 0.0, sq * (q - p)).view(rows, -1))
    a, a0, b = events_ms(fwd, calls), events_ms(fwd0, calls), events_ms(t_fwd, calls)
    fwd()
    tk = t_fwd()
    lines.append(f'dm_kl_free_fwd {rows} x {S} x {C}: {1e3 * a:.1f} us (dm_kl_balance_fwd {1e3 * a0:.1f} us), torch log_softmax + sums + '
                 f'clamp {1e3 * b:.1f} us (x {b / a:.1f}; closed {float(closed.mean()):.2f} of the rows, max differences: kl '
                 f'{float((kl - tk[0]).abs().max()):.1e}, kl_clip {float((clip - tk[1]).abs().max()):.1e})')
    print(lines[-1], flush=True)
    a, a0, b = events_ms(bwd, calls), events_ms(bwd0, calls), events_ms(t_bwd, calls)
    bwd()
    td = t_bwd()
    lines.append(f'dm_kl_free_bwd {rows} x {S} x {C}: {1e3 * a:.1f} us (dm_kl_balance_bwd {1e3 * a0:.1f} us), torch log_softmax + where '
                 f'{1e3 * b:.1f} us (x {b / a:.1f}; max differences: dpost {float((dpost - td[0]).abs().max()):.1e}, dprior '
                 f'{float((dprior - td[1]).abs().max()):.1e})')
    print(lines[-1], flush=True)


def head_kernels(calls, lines):
    K = 255
    g = torch.Generator(device=DEV).manual_seed(1)
    bins = torch.linspace(-20.0, 20.0, K, device=DEV)
    for rows in (2500, 40000):
        logits = torch.randn(rows, K, device=DEV, generator=g) * 3
        target = torch.randn(rows, device=DEV, generator=g) * 100
        loss, mean, dlogits = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, K, device=DEV)
        full = lambda: H.call('dm_twohot_head_loss', rows, 1, K, H.fptr(logits), K, H.fptr(bins), H.fptr(target), 1.0 / rows, H.fptr(loss),
                              H.fptr(dlogits), H.fptr(mean), H.stream())
        only = lambda: H.call('dm_twohot_head_loss', rows, 1, K, H.fptr(logits), K, H.fptr(bins), None, 0.0, None, None, H.fptr(mean),
                              H.stream())

        def t_full():
            x = symlog(target).clamp(bins[0], bins[-1])
            k = ((bins[None, :] <= x[:, None]).sum(-1) - 1).clamp(0, K - 2)
            w_hi = (x - bins[k]) / (bins[k + 1] - bins[k])
            lsm = torch.log_softmax(logits, -1)
            out = -((1 - w_hi) * lsm.gather(-1, k[:, None])[:, 0] + w_hi * lsm.gather(-1, (k + 1)[:, None])[:, 0])
            d = lsm.exp()
            d.scatter_add_(-1, k[:, None], -(1 - w_hi)[:, None]).scatter_add_(-1, (k + 1)[:, None], -w_hi[:, None])
            m = (lsm.exp() * bins).sum(-1)
            return out, d / rows, torch.sign(m) * torch.expm1(m.abs())
        t_only = lambda: torch.sign(m := (torch.softmax(logits, -1) * bins).sum(-1)) * torch.expm1(m.abs())
        a, b = events_ms(full, calls), events_ms(t_full, calls)
        full()
        tl, td, tm = t_full()
        lines.append(f'dm_twohot_head_loss {rows} x {K} (loss + dlogits + mean): {1e3 * a:.1f} us, torch log_softmax + gather + scatter '
                     f'{1e3 * b:.1f} us (x {b / a:.1f}; max differences: loss {float((loss - tl).abs().max()):.1e}, dlogits '
                     f'{float((dlogits - td).abs().max()):.1e}, mean relative to 1 + |m| {float(((mean - tm).abs() / (1 + tm.abs())).max()):.1e})')
        print(lines[-1], flush=True)
        a, b = events_ms(only, calls), events_ms(t_only, calls)
        lines.append(f'dm_twohot_head_loss {rows} x {K} (mean only): {1e3 * a:.1f} us, torch softmax . bins + expm1 {1e3 * b:.1f} us (x {b / a:.1f})')
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


VARIANTS = dict(defaults={}, kl_free_1=dict(kl_free=1.0), twohot_255=dict(reward_dist='twohot', reward_twohot_bins=255),
                twohot_32=dict(reward_dist='twohot', reward_twohot_bins=32),
                both=dict(kl_free=1.0, reward_dist='twohot', reward_twohot_bins=255))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wm_v3_losses_bench.txt'))
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
    # one model per process, one process at a time, alternating (scripts/twohot_critic_bench.py has the reason)
    times = {k: [] for k in VARIANTS}
    for _ in range(args.rounds):
        for k in VARIANTS:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--variant', k, '--steps', str(args.steps), '--warmup',
                                  str(args.warmup), '--reps', str(args.reps)], check=True, capture_output=True, text=True, timeout=300).stdout
            times[k] += json.loads(next(l for l in out.splitlines() if l.startswith('BLOCKS '))[7:])
    H.call('dm_device_check')
    lines = [f'free bits and the symlog two-hot reward head, {torch.cuda.get_device_name(0)}',
             f'the new entries alone at the Atari-literal step\'s shapes, device events, {args.kernel_calls} calls each:']
    kl_kernels(args.kernel_calls, lines)
    head_kernels(args.kernel_calls, lines)
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
