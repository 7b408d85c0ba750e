"""Time per environment step of planning against the actor -> profiles/plan_bench.txt.

    python scripts/plan_bench.py [--out FILE] [--plan-steps 4] [--act-steps 100] [--reps 3] [--kernel-calls 50]

On the model of `defaults` + `atari` (deter 1024, 32 x 32 latents, 18 actions) with PlaNet's planner sizes (horizon 12, 1000
candidates, 100 elites, 10 iterations, the critic closing the return), at B = 1 and 8 environments, in one process:
  (a) plan   CEMPlanner.act, then one torch.cat(action, stats).cpu()   - what PlannerPolicy.__call__ does
  (b) act    Dreamer.act, then the same copy                           - what NetworkPolicy.__call__ does
Both end in a device-to-host wait, so the host clock around a block of steps measures whole steps.  After a warm-up of both the
blocks alternate a, b, a, b, ...; per route (min, median, max) over the blocks of the milliseconds per step.
Before that, with device events around `--kernel-calls` back-to-back calls: dm_cem_draw and dm_cem_update alone at one
environment's shape, which is what the planner launches (their share of the planning step = B x iters x (draw + update) / the
step's median; the rest is the chain and the heads), and dm_cem_update against the torch composition of the same update (returns,
topk, gather, one_hot, mean) on the same inputs.
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
from pydreamer_amd.planner import CEMPlanner              # noqa: E402

DEV = 'cuda'
KEYS = ('policy_value', 'action_prob', 'policy_entropy')


def route(fn):
    def step(obs, state):
        action, state, metrics = fn(obs, state)
        return torch.cat([action.reshape(-1)] + [metrics[k].reshape(1) for k in KEYS]).cpu(), state
    return step


def block(step, obs, state, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        _, state = step(obs, state)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, state


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


def torch_update(B, J, K, Hp, A, gamma, reward, terminal, value, act_idx, prop, floor):
    """The composition dm_cem_update replaces (kind 0, alpha = 0): the same quantities from torch ops."""
    w = torch.ones_like(reward[0])
    ret = torch.zeros_like(reward[0])
    for t in range(Hp):
        ret = ret + (gamma ** t) * w * reward[t]
        w = w * (1 - terminal[t])
    ret = ret + (gamma ** Hp) * w * value
    key = torch.where(torch.isfinite(ret), ret, torch.full_like(ret, torch.finfo(torch.float32).min)).view(B, J)
    top, elite = torch.topk(key, K, dim=1)
    idx = torch.gather(act_idx.view(Hp, B, J).long(), 2, elite.unsqueeze(0).expand(Hp, B, K))
    freq = torch.nn.functional.one_hot(idx, A).float().mean(2).transpose(0, 1)
    out = (1 - floor) * freq + floor / A
    p0 = out[:, 0]
    stats = torch.stack((top[:, 0], top.mean(1), -(p0 * p0.clamp_min(1e-30).log()).sum(1),
                         torch.gather(p0, 1, idx[0, :, :1]).squeeze(1)), 1)
    return out, ret, elite, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plan_bench.txt'))
    ap.add_argument('--plan-steps', type=int, default=4)
    ap.add_argument('--act-steps', type=int, default=100)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--kernel-calls', type=int, default=50)
    args = ap.parse_args()
    H.call('dm_device_check')
    conf = config.load_config('defaults', 'atari')
    torch.manual_seed(0)
    model = Dreamer(conf).to(DEV)
    planner = CEMPlanner(model)
    A, Hp, J, K, iters = conf.action_dim, planner.horizon, planner.candidates, planner.elites, planner.iters
    lines = [f'planning against acting, defaults + atari (deter {conf.deter_dim}, latents {conf.stoch_dim} x {conf.stoch_discrete}, {A} '
             f'actions), horizon {Hp}, {J} candidates, {K} elites, {iters} iterations, value {planner.use_value}, '
             f'{torch.cuda.get_device_name(0)}',
             f'host milliseconds per environment step, {args.reps} alternating blocks of {args.plan_steps} (plan) / {args.act_steps} '
             f'(act) steps: min median max',
             '(a) CEMPlanner.act + one device-to-host copy   (b) Dreamer.act + the same copy']
    # the two kernels alone at one environment's shape - what the planner launches - and the torch composition of the update
    B = 1
    M = B * J
    prop = torch.full((B, Hp, A), 1.0 / A, device=DEV)
    u = torch.rand(Hp, M, device=DEV)
    actions, act_idx = torch.empty(Hp, M, A, device=DEV), torch.empty(Hp, M, dtype=torch.int32, device=DEV)
    reward, terminal, value = torch.randn(Hp, M, device=DEV), torch.rand(Hp, M, device=DEV) * 0.1, torch.randn(M, device=DEV)
    pout, ret = torch.empty_like(prop), torch.empty(M, device=DEV)
    elite, first, stats = torch.empty(B, K, dtype=torch.int32, device=DEV), torch.empty(B, A, device=DEV), torch.empty(B, 4, device=DEV)
    gamma = float(model.ac.gamma)
    draw = lambda: H.call('dm_cem_draw', 0, B, J, Hp, A, H.fptr(prop), H.fptr(u), H.fptr(actions), H.ptr(act_idx), H.stream())
    update = lambda: H.call('dm_cem_update', 0, B, J, K, Hp, A, gamma, H.fptr(reward), H.fptr(terminal), H.fptr(value),
                            H.fptr(actions), H.ptr(act_idx), H.fptr(prop), 0.0, planner.floor, H.fptr(pout), H.fptr(ret),
                            H.ptr(elite), H.fptr(first), H.fptr(stats), H.stream())
    composed = lambda: torch_update(B, J, K, Hp, A, gamma, reward, terminal, value, act_idx, prop, planner.floor)
    t_draw, t_upd, t_torch = (events_ms(f, args.kernel_calls) for f in (draw, update, composed))
    out_t, _, elite_t, _ = composed()
    same = bool((elite_t.sort(1).values == elite.long().sort(1).values).all()) and float((out_t - pout).abs().max()) < 1e-6
    lines.append(f'one environment ({J} candidates), device events, {args.kernel_calls} calls: dm_cem_draw {1e3 * t_draw:.1f} us, dm_cem_update '
                 f'{1e3 * t_upd:.1f} us, torch composition of the update {1e3 * t_torch:.1f} us (x {t_torch / t_upd:.1f}; same elites and '
                 f'proposal: {same})')
    print(lines[-1], flush=True)
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        obs = dict(image=torch.randint(0, 256, (1, B, 64, 64, conf.image_channels), generator=g, dtype=torch.uint8),
                   action=torch.nn.functional.one_hot(torch.randint(0, A, (1, B), generator=g), A).float(),
                   reset=torch.zeros(1, B, dtype=torch.bool))
        obs = {k: v.to(DEV) for k, v in obs.items()}
        routes = dict(a=(route(planner.act), args.plan_steps), b=(route(model.act), args.act_steps))
        states = {k: model.init_state(B) for k in routes}
        times = {k: [] for k in routes}
        for k, (fn, _) in routes.items():      # warm-up: code objects, allocator, this batch size's workspaces
            _, states[k] = block(fn, obs, states[k], 2)
        for _ in range(args.reps):
            for k, (fn, steps) in routes.items():
                t, states[k] = block(fn, obs, states[k], steps)
                times[k].append(t)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        fmt = lambda v: f'{min(v):9.3f} {sorted(v)[len(v) // 2]:9.3f} {max(v):9.3f}'
        lines.append(f'  B {B:2d}   (a) {fmt(times["a"])}   (b) {fmt(times["b"])}   '
                     f'a / b = {med["a"] / med["b"]:.1f}')
        print(lines[-1], flush=True)
        share = B * iters * (t_draw + t_upd) / med['a']
        lines.append(f'       {B} x {iters} x (draw + update) = {B * iters * (t_draw + t_upd):.3f} ms = {100 * share:.2f} % of the planning step; '
                     f'the rest is {B} x {iters * Hp} chain steps, the heads and the posterior step')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
