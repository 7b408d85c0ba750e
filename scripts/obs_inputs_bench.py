"""Step time with and without reward_input (encoders.py:52-59) at the `miniworld` shape - B=32, T=48, cnn_depth=32,
action_dim=3, everything else `defaults` - and with vecobs_size 0 / 27 at the `minecraft` shape - B=32, T=48, cnn_depth=48,
action_dim=29.

    python scripts/obs_inputs_bench.py --reward-input 0
    python scripts/obs_inputs_bench.py --reward-input 1
    python scripts/obs_inputs_bench.py --shape minecraft --vecobs-size 27
    python scripts/obs_inputs_bench.py --reward-input 0 --root <another checkout of this repository>

What is timed: Dreamer.training_step + the four backward passes + grad_clip + the AdamW steps (train.py:165-198), uint8 frames
on the device, after --warmup steps; --regions timed regions of --steps steps each, every region between two device events
that are waited for.  One JSON line: ms per step of every region, their median and their spread (max - min).  --root imports
the package from another checkout, so that the commit before a change is measured by the same script in the same visit
(the shape is spelled out here instead of taken from the `miniworld` section for that reason).

For --reward-input 1 the line also carries the time of one HBM pass over the layer-1 output gradient G (N * 961 * d * 4 bytes
at 6.0 TB/s, a swept 1.2 GB table on the MI355X): the fold adds one (N, d) table and no pass over G or the frames, so the
difference to the run without the key is expected to stay below the spread plus that time.  For --vecobs-size > 0 it carries
the forward + backward time of the two vecobs MLPs and of the reward head at the same T * B rows, each timed alone.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

HBM_STREAM_BYTES_PER_S = 6.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reward-input', type=int, default=0)
    ap.add_argument('--vecobs-size', type=int, default=0)
    ap.add_argument('--shape', choices=('miniworld', 'minecraft'), default='miniworld')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from pydreamer_amd import config, hip
    from pydreamer_amd.models import Dreamer
    if not torch.cuda.is_available():
        raise SystemExit('obs_inputs_bench: no GPU - a step time is measured on the MI355X or not at all')
    hip.call('dm_device_check')
    dev = torch.device('cuda:0')
    kw = dict(action_dim=3, cnn_depth=32) if args.shape == 'miniworld' else dict(action_dim=29)
    if args.reward_input:
        kw['reward_input'] = True
    if args.vecobs_size:
        kw['vecobs_size'] = args.vecobs_size
    conf = config.load_config('defaults', **kw)
    T, B, A = conf.batch_length, conf.batch_size, conf.action_dim
    torch.manual_seed(0)
    model = Dreamer(conf).to(dev)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    gen = torch.Generator().manual_seed(1234)
    ring = []
    for _ in range(4):
        ring.append(dict(image=torch.randint(0, 256, (T, B, 64, 64, 3), generator=gen, dtype=torch.uint8).to(dev),
                         action=F.one_hot(torch.randint(0, A, (T, B), generator=gen), A).float().to(dev),
                         reward=torch.tanh(torch.randn(T, B, generator=gen)).to(dev),
                         terminal=(torch.rand(T, B, generator=gen) < 0.01).float().to(dev),
                         reset=(torch.rand(T, B, generator=gen) < 0.005).to(dev)))
        if args.vecobs_size:
            ring[-1]['vecobs'] = torch.randn(T, B, args.vecobs_size, generator=gen).to(dev)
    state = model.init_state(B)

    def step(i):
        nonlocal state
        losses, state, metrics, _, _ = model.training_step(ring[i % len(ring)], state)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in opts:
            opt.step()
        return metrics

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    region_ms, n = [], args.warmup
    for _ in range(args.regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            metrics = step(n + i)
        e1.record()
        e1.synchronize()
        n += args.steps
        region_ms.append(e0.elapsed_time(e1) / args.steps)
    loss_model = float(metrics['loss_model'])
    assert loss_model == loss_model, 'loss_model is NaN'
    line = dict(shape=dict(B=B, T=T, cnn_depth=conf.cnn_depth, action_dim=A, deter_dim=conf.deter_dim), reward_input=bool(args.reward_input),
                vecobs_size=args.vecobs_size,
                root=os.path.basename(os.path.abspath(args.root)), steps_per_region=args.steps, warmup=args.warmup,
                ms_per_step_regions=[round(x, 4) for x in region_ms], ms_per_step_median=round(sorted(region_ms)[len(region_ms) // 2], 4),
                spread_ms=round(max(region_ms) - min(region_ms), 4), loss_model=loss_model)
    if args.reward_input:
        line['one_hbm_pass_over_G_ms'] = round(1e3 * T * B * 961 * conf.cnn_depth * 4 / HBM_STREAM_BYTES_PER_S, 4)
    if args.vecobs_size:
        rows, F_ = T * B, model.wm.features_dim
        ws = model.wm.workspace(model.wm.shape(T, B, 1), dev)

        def mlp_ms(mlp, x):
            def once():
                out, acts = mlp.fwd(x, x.shape[1], rows, ws)
                mlp.bwd(x, x.shape[1], rows, acts, torch.ones_like(out), ws)
            for _ in range(5):
                once()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                once()
            e1.record()
            e1.synchronize()
            return round(e0.elapsed_time(e1) / 50, 4)
        feat = torch.randn(rows, F_, device=dev)
        line['mlp_fwd_bwd_ms_at_TB_rows'] = dict(
            encoder_vecobs=mlp_ms(model.wm.encoder.encoder_vecobs, torch.randn(rows, args.vecobs_size, device=dev)),
            decoder_vecobs=mlp_ms(model.wm.decoder.vecobs.model, feat), reward_head=mlp_ms(model.wm.decoder.reward.model, feat))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
