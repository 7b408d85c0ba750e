"""Step time of the image-less world model at the `vectorenv` section's native shape - B=32, T=48, vecobs_size=4,
action_dim=2, deter_dim=2048, hidden_dim=1000, imag_horizon=15, everything as load_config('defaults', 'vectorenv') gives it -
in fp32 and with --amp.

    python scripts/vectorenv_bench.py
    python scripts/vectorenv_bench.py --amp

The method of scripts/obs_inputs_bench.py: Dreamer.training_step + the four backward passes + grad_clip + the AdamW steps
(train.py:165-198) on batches that live on the device and hold no image, after --warmup steps; --regions timed regions of --steps
steps each, every region between two device events that are waited for.  One JSON line: ms per step of every region, their
median and their spread (max - min), and the forward + backward time of the two vecobs MLPs and of the reward head at the same
T * B rows, each timed alone.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--amp', action='store_true')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--regions', type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pydreamer_amd import config, hip
    from pydreamer_amd.models import Dreamer
    if not torch.cuda.is_available():
        raise SystemExit('vectorenv_bench: no GPU - a step time is measured on the MI355X or not at all')
    hip.call('dm_device_check')
    dev = torch.device('cuda:0')
    conf = config.load_config('defaults', 'vectorenv', amp=bool(args.amp))
    T, B, A, V = conf.batch_length, conf.batch_size, conf.action_dim, conf.vecobs_size
    torch.manual_seed(0)
    model = Dreamer(conf).to(dev)
    assert model.wm.imageless
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    gen = torch.Generator().manual_seed(1234)
    ring = [dict(action=F.one_hot(torch.randint(0, A, (T, B), generator=gen), A).float().to(dev),
                 reward=torch.tanh(torch.randn(T, B, generator=gen)).to(dev),
                 terminal=(torch.rand(T, B, generator=gen) < 0.01).float().to(dev),
                 reset=(torch.rand(T, B, generator=gen) < 0.005).to(dev),
                 vecobs=torch.randn(T, B, V, generator=gen).to(dev)) for _ in range(4)]
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
    line = dict(shape=dict(B=B, T=T, vecobs_size=V, action_dim=A, deter_dim=conf.deter_dim, hidden_dim=conf.hidden_dim,
                           imag_horizon=conf.imag_horizon), amp=bool(args.amp),
                parameters=sum(p.numel() for p in model.parameters()), steps_per_region=args.steps, warmup=args.warmup,
                ms_per_step_regions=[round(x, 4) for x in region_ms], ms_per_step_median=round(sorted(region_ms)[len(region_ms) // 2], 4),
                spread_ms=round(max(region_ms) - min(region_ms), 4), loss_model=loss_model,
                schedule=dict(fwd=hip.last_schedule(0), rollout=hip.last_schedule(2)),
                mlp_fwd_bwd_ms_at_TB_rows=dict(encoder_vecobs=mlp_ms(model.wm.encoder.encoder_vecobs, torch.randn(rows, V, device=dev)),
                                               decoder_vecobs=mlp_ms(model.wm.decoder.vecobs.model, feat),
                                               reward_head=mlp_ms(model.wm.decoder.reward.model, feat)))
    print(json.dumps(line))


if __name__ == '__main__':
    main()
