"""Timing record of the dense categorical image path -> profiles/minigrid_bench.txt.

    python scripts/minigrid_bench.py --parent ../parent-checkout [--this-first] [--out profiles/minigrid_bench.txt] [--append]
                                     [--baseline]

Two things (three with --baseline), on one GPU of one box:

1. The flagship benchmark, which the dense path must not move (it touches no call of the convolution path):
   `bench.py --gpus 1 --steps 20 --warmup 5` twice in --parent, a BUILT checkout of the parent commit (e.g. `git worktree add`
   + build()), and once in this tree.  The new value has to lie within the spread of the parent's two runs; the script records
   the three values and says whether it does.  Without --parent only this tree is measured.
2. The time of one trainer iteration at `defaults + minigrid` as the section stands (T=48, B=32, deter 2048, 32x32 latents, the
   map probe on an 11x11 map): training_step + zero_grad + 4 x backward + grad_clip + 4 x AdamW on synthetic class images, the
   batch resident in HBM.  There is no earlier number to hold it against: a record, not a bar.
3. --baseline: one trainer iteration of WorldModelProbe at the same section with model=gru_probe, probe_gradients=True,
   probe_model=map (DenseEncoder -> Linear(256, 32) -> GRU(39, 2048) -> map probe): training_step + zero_grad + backward + grad_clip
   + AdamW, the image as the uint8 class map (T,B,7,7) the feeds hand over.  A record as well.

Every benchmark run is a fresh child process with its own time limit; the first failure ends the script.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BENCH = ['bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5']


def run_bench(tree, limit):
    p = subprocess.run([sys.executable] + BENCH, cwd=tree, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f'bench.py failed in {tree} with exit status {p.returncode}')
    line = next(l for l in reversed(p.stdout.splitlines()) if l.startswith('{'))
    rec = json.loads(line)
    return float(rec['value']), float(rec.get('ms_per_step') or 1000.0 / rec['value'])


def minigrid_step_ms(steps, warmup):
    import torch
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    conf = config.load_config('defaults', 'minigrid')
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = Dreamer(conf).to(dev)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    T, B, A = conf.batch_length, conf.batch_size, conf.action_dim
    g = torch.Generator(device=dev).manual_seed(1)
    ri = lambda hi, *shape: torch.randint(0, hi, shape, device=dev, generator=g)
    one_hot = torch.nn.functional.one_hot
    obs = dict(image=one_hot(ri(conf.image_channels, T, B, conf.image_size, conf.image_size), conf.image_channels)
               .permute(0, 1, 4, 2, 3).float().contiguous(),                                    # replay.preprocess_batch(image_categorical=C)
               action=one_hot(ri(A, T, B), A).float(), reward=torch.tanh(torch.randn(T, B, device=dev, generator=g)),
               terminal=(torch.rand(T, B, device=dev, generator=g) < 0.01).float(), reset=torch.zeros(T, B, dtype=torch.bool, device=dev),
               map=ri(conf.map_channels, T, B, conf.map_size, conf.map_size), map_coord=torch.randn(T, B, 4, device=dev, generator=g))
    state = model.init_state(B)

    def step(state):
        losses, state, _, _, _ = model.training_step(obs, state)
        for o in opts:
            o.zero_grad()
        for l in losses:
            l.backward()
        model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for o in opts:
            o.step()
        return state
    for _ in range(warmup):
        state = step(state)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        state = step(state)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1000.0 / steps
    model.check_device_status()
    n = sum(p.numel() for p in model.parameters())
    return ms, f'T={T} B={B} rows={T * B} deter={conf.deter_dim} parameters={n} steps={steps} warmup={warmup}'


def baseline_step_ms(steps, warmup):
    import torch
    from pydreamer_amd import config
    from pydreamer_amd.models import WorldModelProbe
    conf = config.load_config('defaults', 'minigrid', model='gru_probe', probe_gradients=True, probe_model='map')
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = WorldModelProbe(conf).to(dev)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    T, B, A = conf.batch_length, conf.batch_size, conf.action_dim
    g = torch.Generator(device=dev).manual_seed(1)
    ri = lambda hi, *shape: torch.randint(0, hi, shape, device=dev, generator=g)
    obs = dict(image=ri(conf.image_channels, T, B, conf.image_size, conf.image_size).to(torch.uint8),      # ReplayFeed / DeviceReplay(image_categorical=C)
               action_next=torch.nn.functional.one_hot(ri(A, T, B), A).float(), reward=torch.tanh(torch.randn(T, B, device=dev, generator=g)),
               terminal=(torch.rand(T, B, device=dev, generator=g) < 0.01).float(), reset=torch.zeros(T, B, dtype=torch.bool, device=dev),
               map=ri(conf.map_channels, T, B, conf.map_size, conf.map_size).to(torch.uint8),
               map_coord=torch.randn(T, B, 4, device=dev, generator=g))
    state = model.init_state(B)

    def step(state):
        losses, state, _, _, _ = model.training_step(obs, state)
        for o in opts:
            o.zero_grad()
        for l in losses:
            l.backward()
        model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for o in opts:
            o.step()
        return state
    for _ in range(warmup):
        state = step(state)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        state = step(state)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1000.0 / steps
    n = sum(p.numel() for p in model.parameters())
    return ms, f'T={T} B={B} rows={T * B} deter={conf.deter_dim} parameters={n} steps={steps} warmup={warmup}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='', help='a built checkout of the parent commit; its bench.py runs twice')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'minigrid_bench.txt'))
    ap.add_argument('--this-first', action='store_true', help='run this tree before the parent (does the position in the series matter?)')
    ap.add_argument('--append', action='store_true', help='add this series to --out instead of replacing it')
    ap.add_argument('--baseline', action='store_true', help='also time one iteration of the gru_probe baseline on the section')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--limit', type=int, default=300, help='time limit of one bench.py run, seconds')
    args = ap.parse_args()
    lines = ['# scripts/minigrid_bench.py', '# ' + ' '.join(BENCH) + ' : grad-steps/s (ms per step)']

    def note(*new):          # printed as soon as it exists: a series takes minutes
        lines.extend(new)
        print('\n'.join(new), flush=True)
    parent = []
    if args.this_first:
        v, ms = run_bench(ROOT, args.limit)
        note(f'this commit : {v:.4f} ({ms:.3f} ms)')
    if args.parent:
        for i in range(2):
            pv, pms = run_bench(args.parent, args.limit)
            parent.append(pv)
            note(f'parent run {i + 1}: {pv:.4f} ({pms:.3f} ms)')
    if not args.this_first:
        v, ms = run_bench(ROOT, args.limit)
        note(f'this commit : {v:.4f} ({ms:.3f} ms)')
    if parent:
        lo, hi = min(parent), max(parent)
        note(f'within the spread of the parent\'s two runs [{lo:.4f}, {hi:.4f}]: {"yes" if lo <= v <= hi else "NO"}')
    ms, what = minigrid_step_ms(args.steps, args.warmup)
    note('# defaults + minigrid: training_step + zero_grad + 4 x backward + grad_clip + 4 x AdamW', f'# {what}',
         f'minigrid iteration: {ms:.3f} ms ({1000.0 / ms:.2f} grad-steps/s)')
    if args.baseline:
        ms, what = baseline_step_ms(args.steps, args.warmup)
        note('# defaults + minigrid, model=gru_probe, probe_model=map: training_step + zero_grad + backward + grad_clip + AdamW',
             f'# {what}', f'gru_probe iteration: {ms:.3f} ms ({1000.0 / ms:.2f} grad-steps/s)')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a' if args.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
