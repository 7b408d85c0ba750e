"""Time per environment step of the acting path -> profiles/act_bench.txt.

    python scripts/act_bench.py [--out FILE] [--steps 200] [--reps 5]

Two routes from a preprocessed device observation to the action and the three logged scalars ON THE HOST, in the same process, on
the model of `defaults` + `atari` (deter 1024, 32 x 32 latents, 18 actions) at B = 1, 16 and 256 environments:
  (a) act        Dreamer.act, then one torch.cat(action, stats).cpu()                       - what NetworkPolicy.__call__ does
  (b) inference  Dreamer.inference, then the reference generator's torch ops on the distribution object (generator.py:321-328):
                 sample(), log_prob(action).exp().mean().item(), entropy().mean().item(), policy_value.item(), action.cpu()
Both end in a device-to-host wait, so the host clock around a block of steps measures whole steps (launches, kernels and waits).
Each route carries its recurrent state from step to step.  After a warm-up of both routes the blocks alternate a, b, a, b, ...;
per route the (min, median, max) over the blocks of the microseconds per step, and the ratio of the medians b / a.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydreamer_amd import config, hip as H                # noqa: E402
from pydreamer_amd.models import Dreamer                  # noqa: E402

DEV = 'cuda'
KEYS = ('policy_value', 'action_prob', 'policy_entropy')


def route_act(model, obs, state):
    action, state, metrics = model.act(obs, state)
    host = torch.cat([action.reshape(-1)] + [metrics[k].reshape(1) for k in KEYS]).cpu()
    return host, state


def route_inference(model, obs, state):
    with torch.no_grad():
        dist, state, metrics = model.inference(obs, state)
        action = dist.sample()
    out = {k: v.item() for k, v in metrics.items()}
    out.update(action_prob=dist.log_prob(action).exp().mean().item(), policy_entropy=dist.entropy().mean().item())
    return (action.cpu(), out), state


def block(route, model, obs, state, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        _, state = route(model, obs, state)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / steps, state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'act_bench.txt'))
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    H.call('dm_device_check')
    conf = config.load_config('defaults', 'atari')
    torch.manual_seed(0)
    model = Dreamer(conf).to(DEV)
    A = conf.action_dim
    lines = [f'acting path, defaults + atari (deter {conf.deter_dim}, latents {conf.stoch_dim} x {conf.stoch_discrete}, {A} actions), '
             f'{torch.cuda.get_device_name(0)}',
             f'host microseconds per environment step, {args.reps} alternating blocks of {args.steps} steps per route: min median max',
             '(a) Dreamer.act + one device-to-host copy   (b) Dreamer.inference + the generator\'s torch ops and .item() reads']
    for B in (1, 16, 256):
        g = torch.Generator().manual_seed(B)
        obs = dict(image=torch.randint(0, 256, (1, B, 64, 64, conf.image_channels), generator=g, dtype=torch.uint8),
                   action=torch.nn.functional.one_hot(torch.randint(0, A, (1, B), generator=g), A).float(),
                   reset=torch.zeros(1, B, dtype=torch.bool))
        obs = {k: v.to(DEV) for k, v in obs.items()}
        routes = dict(a=route_act, b=route_inference)
        states = {k: model.init_state(B) for k in routes}
        times = {k: [] for k in routes}
        for k, fn in routes.items():      # warm-up: code objects, allocator, this batch size's workspaces
            _, states[k] = block(fn, model, obs, states[k], 20)
        for _ in range(args.reps):
            for k, fn in routes.items():
                t, states[k] = block(fn, model, obs, states[k], args.steps)
                times[k].append(t)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        fmt = lambda v: f'{min(v):9.1f} {sorted(v)[len(v) // 2]:9.1f} {max(v):9.1f}'
        lines.append(f'  B {B:4d}   (a) {fmt(times["a"])}   (b) {fmt(times["b"])}   b / a = {med["b"] / med["a"]:.3f}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[:3]))


if __name__ == '__main__':
    main()
