"""Step time at Atari-literal (B = 50, T = 50, 64 x 64 x 3 frames) under the three ways a batch can reach the step, in ONE process:

  resident : the step on batches already in device memory (a ring of four);
  ring     : fed by DeviceRing(ReplayFeed(SequentialReplay)) - episode files -> pinned slot -> 30.9 MB over PCIe per step;
  device   : fed by DeviceReplay - episodes resident in HBM, one gather launch per batch;

and the gather launch alone, by device events, next to a device-to-device copy_ of the same byte count.

    python scripts/replay_feed_bench.py [--steps 30] [--warmup 10] [--regions 3] [--files 24] [--rows 1000]

The repository is synthetic and written to a temporary directory: --files episode files of --rows rows, stored UNCOMPRESSED
(the ring leg reads a file on every visit; zlib would make that leg measure the decompressor).  Both feeds run the trainer's
order: next() in front of training_step(), prefetch() right after it returned.  What is timed per leg: --regions regions of
--steps steps (training_step + four backward passes + grad_clip + AdamW), each between a synchronise and a synchronise, host
clock; the legs ALTERNATE region by region, so drift of the box hits all three alike.  One JSON line: ms per step of every
region, median and spread (max - min) per leg; the gather and the copy as microseconds per launch, three regions of 200.
No GPU, no number: the script refuses to run without one."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_repository(path, files, rows, action_dim, seed=0):
    from pydreamer_amd.replay import LocalEpisodeRepository
    rs = np.random.RandomState(seed)
    for ep in range(files):
        d = dict(image=rs.randint(0, 256, (rows, 64, 64, 3), dtype=np.uint8), action=rs.randint(0, action_dim, rows),
                 reward=rs.randn(rows).astype(np.float32), terminal=np.zeros(rows, bool), reset=np.zeros(rows, bool))
        d['terminal'][-1] = True
        name = LocalEpisodeRepository.build_episode_name(ep, ep, float(d['reward'].sum()), rows - 1)
        np.savez(os.path.join(path, name), **d)
    return LocalEpisodeRepository(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--files', type=int, default=24)
    ap.add_argument('--rows', type=int, default=1000)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from pydreamer_amd import config, hip
    from pydreamer_amd import replay as R
    from pydreamer_amd.models import Dreamer
    if not torch.cuda.is_available():
        raise SystemExit('replay_feed_bench: no GPU - a step time is measured on the MI355X or not at all')
    hip.call('dm_device_check')
    dev = torch.device('cuda:0')
    conf = config.atari_literal()
    T, B, A = conf.batch_length, conf.batch_size, conf.action_dim
    torch.manual_seed(0)
    model = Dreamer(conf).to(dev)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    state = model.init_state(B)

    def step(obs, after=None):
        nonlocal state
        losses, state, metrics, _, _ = model.training_step(obs, state)
        if after is not None:
            after()
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in opts:
            opt.step()
        return metrics

    with tempfile.TemporaryDirectory() as tmp:
        repo = write_repository(tmp, args.files, args.rows, A)
        replay = lambda: R.SequentialReplay(repo, T, B, allow_mid_reset=True, seed=7)
        ring = R.DeviceRing(R.ReplayFeed(replay(), A, clip_rewards='tanh'), dev, depth=4)
        dr = R.DeviceReplay(replay(), A, dev, depth=4, clip_rewards='tanh')
        res = R.DeviceReplay(replay(), A, dev, depth=4, clip_rewards='tanh')
        resident = [{k: v.clone() for k, v in res.next().items()} for _ in range(4)]
        res.close()
        del res
        count = [0]

        def resident_step():
            count[0] += 1
            return step(resident[count[0] % 4])
        legs = {'resident': resident_step, 'ring': lambda: step(ring.next(), ring.prefetch), 'device': lambda: step(dr.next(), dr.prefetch)}
        for run in legs.values():
            for _ in range(args.warmup):
                run()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(args.regions):
            for k, run in legs.items():
                run()                                          # the first step behind another leg is not that leg's steady state
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    metrics = run()
                torch.cuda.synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
        loss_model = float(metrics['loss_model'])
        assert loss_model == loss_model, 'loss_model is NaN'

        # the gather launch alone against a device-to-device copy of the same bytes
        stream = torch.cuda.current_stream(dev)
        nbytes = T * B * sum(dr.row_bytes.values())
        a, b = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        slot = (dr.next_dev - 1) % dr.depth
        reps = 200

        def events_us(fn):
            out = []
            for _ in range(args.regions):
                for _ in range(10):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                out.append(1e3 * e0.elapsed_time(e1) / reps)
            return out
        gather_us = events_us(lambda: dr._launch(slot, stream))
        copy_us = events_us(lambda: b.copy_(a))
        cached = dict(files=len(dr._cache), bytes=dr.cached_bytes)
        ring.close()
        dr.close()

    def leg(v):
        return dict(ms_per_step_regions=[round(x, 4) for x in v], median=round(sorted(v)[len(v) // 2], 4), spread=round(max(v) - min(v), 4))
    line = dict(shape=dict(B=B, T=T, action_dim=A), repository=dict(files=args.files, rows=args.rows, compressed=False),
                steps_per_region=args.steps, warmup=args.warmup, legs={k: leg(v) for k, v in ms.items()},
                batch_bytes=nbytes, resident_episodes=cached,
                gather_us_per_launch=dict(regions=[round(x, 3) for x in gather_us], median=round(sorted(gather_us)[len(gather_us) // 2], 3)),
                d2d_copy_us_same_bytes=dict(regions=[round(x, 3) for x in copy_us], median=round(sorted(copy_us)[len(copy_us) // 2], 3)),
                gather_read_plus_write_TBps=round(2 * nbytes / (sorted(gather_us)[len(gather_us) // 2] * 1e-6) / 1e12, 3),
                loss_model=loss_model)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
