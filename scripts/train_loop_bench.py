"""Host milliseconds per gradient step under three logging routes -> profiles/train_loop_bench.txt.

    python scripts/train_loop_bench.py [--out FILE] [--steps 100] [--reps 5] [--pipeline]

The Atari-literal model (config.atari_literal(): B 50, T 50, H 15, deter 600, 32 x 32 latents, fp32) on ONE fixed device batch; a
step is training_step -> zero_grad -> 4 x backward -> grad_clip -> 4 x AdamW, bench.py's loop.  Routes:
  (a) none       no logging at all: bench.py's loop
  (b) host       packed_metrics_host() every step - one device-to-host wait per step: the documented trainer route, the baseline
  (c) accum      join_optimizers() + MetricAccumulator.add(metric_buffer) + add_batch_stats(obs) behind the optimizer step, ONE
                 read_and_reset() per block: what train.run does
  (d) deferred   as (c), but step n's buffer is folded after training_step() of step n + 1 has returned, where the caller's stream
                 has already waited for the pipelined actor / critic optimizers, so no join is needed (the last buffer of a block is
                 folded with a join before the read)
After a warm-up of every route the blocks alternate a, b, c, d, a, ...; the host clock runs around each block, with a device
synchronize at its end.  Per route: min / median / max over the blocks of the milliseconds per step.  --pipeline switches
Dreamer.pipeline_ac_optimizer on (bench.py's --pipeline), where the gradient norms of the actor and critic are written on the
actor-critic stream."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydreamer_amd import config, hip as H                                  # noqa: E402
from pydreamer_amd.models import Dreamer                                    # noqa: E402
from pydreamer_amd.train import MetricAccumulator, default_slots            # noqa: E402

DEV = 'cuda'


def make_batch(conf, seed=0):
    g = torch.Generator().manual_seed(seed)
    T, B, A = conf.batch_length, conf.batch_size, conf.action_dim
    u8 = torch.randint(0, 256, (T, B, conf.image_size, conf.image_size, conf.image_channels), generator=g, dtype=torch.uint8)
    reset = torch.rand(T, B, generator=g) < 1.0 / 200
    reset[0, 0] = True
    obs = dict(image=u8.float().div_(255.0).sub_(0.5).permute(0, 1, 4, 2, 3).contiguous(),
               action=torch.nn.functional.one_hot(torch.randint(0, A, (T, B), generator=g), A).float(),
               reward=torch.tanh(torch.randn(T, B, generator=g)), terminal=(torch.rand(T, B, generator=g) < 0.005).float(), reset=reset)
    return {k: v.to(DEV) for k, v in obs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_loop_bench.txt'))
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--pipeline', action='store_true')
    args = ap.parse_args()
    H.call('dm_device_check')
    conf = config.atari_literal()
    torch.manual_seed(0)
    model = Dreamer(conf).to(DEV)
    model.pipeline_ac_optimizer = bool(args.pipeline)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    obs = make_batch(conf)
    acc = MetricAccumulator(default_slots(model), DEV)
    st = {'s': model.init_state(conf.batch_size), 'prev': None, 'last': None}

    def step(route):
        losses, st['s'], _, _, _ = model.training_step(obs, st['s'])
        if route == 'd' and st['prev'] is not None:      # the stream has waited for the previous step's optimizers by now
            acc.add(st['prev'])
            acc.add_batch_stats(obs)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in opts:
            opt.step()
        if route == 'b':
            st['last'] = model.packed_metrics_host()
        elif route == 'c':
            model.join_optimizers()
            acc.add(model.metric_buffer)
            acc.add_batch_stats(obs)
        elif route == 'd':
            st['prev'] = model.metric_buffer

    def block(route, steps):
        st['prev'] = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(route)
        if route == 'd':
            model.join_optimizers()
            acc.add(st['prev'])
            acc.add_batch_stats(obs)
        if route in ('c', 'd'):
            st['last'] = acc.read_and_reset()
            model.check_device_status()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    routes = dict(a='none', b='host', c='accum', d='deferred')
    times = {k: [] for k in routes}
    for k in routes:
        block(k, args.warmup)
    for _ in range(args.reps):
        for k in routes:
            times[k].append(block(k, args.steps))
            print(f'  ({k}) {routes[k]:9s} {times[k][-1]:8.3f} ms / step', flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    lines = [f'trainer loop logging routes, Atari-literal fp32 (B {conf.batch_size}, T {conf.batch_length}), one fixed device batch, '
             f'{torch.cuda.get_device_name(0)}, pipeline_ac_optimizer = {bool(args.pipeline)}',
             f'host milliseconds per gradient step, {args.reps} alternating blocks of {args.steps} steps per route: min median max']
    for k, name in routes.items():
        v = times[k]
        lines.append(f'  ({k}) {name:9s} {min(v):8.3f} {med[k]:8.3f} {max(v):8.3f}')
    shown = med['c'] < min(times['b'])
    lines.append(f'(c) median {med["c"]:.3f} vs (b) minimum {min(times["b"]):.3f}: ' +
                 ('(c) is faster than (b) in every block pairing' if shown else 'the ranges overlap: no gain is shown'))
    lines.append(f'(c) median - (a) median = {med["c"] - med["a"]:+.3f} ms; (d) median - (c) median = {med["d"] - med["c"]:+.3f} ms')
    lines.append(f'logged by the last (c)/(d) block: loss_model {st["last"].get("loss_model", float("nan")):.6g}, '
                 f'data_reset {st["last"].get("data_reset", float("nan")):.6g}')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a' if args.pipeline else 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
