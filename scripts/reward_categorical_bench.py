"""The categorical reward decoder (reward_decoder_categorical) at the Atari-literal shape - B=50, T=50, H=15,
deter 600, fp32.

    python scripts/reward_categorical_bench.py kernel
    python scripts/reward_categorical_bench.py step --categorical 1
    python scripts/reward_categorical_bench.py step --categorical 0
    python scripts/reward_categorical_bench.py step --categorical 0 --root <a checkout of the parent commit>

kernel  dm_head_loss_catsup alone at rows = 2 500 (the full form: loss, dlogits, mean, bin) and rows = 40 000 (the mean-only
        form of the dream) for K in {4, 32}, against the same results composed from torch device ops - log_softmax, gather,
        softmax, the one-hot subtraction and scaling, softmax @ support, the squared-distance argmin.  Each timed between two
        device events over --iters calls after a warm-up; the outputs of the two are compared first.  The line also carries
        the bytes a call must move (logits in, outputs out) and the time that takes at 6.0 TB/s.
step    Dreamer.training_step + the four backward passes + grad_clip + the AdamW steps (train.py:165-198), as
        scripts/obs_inputs_bench.py times it: --regions regions of --steps steps between device events after --warmup steps;
        ms per step of every region, the median and the spread.  --categorical 1 sets reward_decoder_categorical=[-10, 0, 1, 10];
        --root imports the package from another checkout, so that the parent commit is measured by the same script in the
        same visit.
One JSON line per run.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

HBM_STREAM_BYTES_PER_S = 6.0e12


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters      # microseconds per call


def kernel_mode(args, hip, dev):
    out = []
    for rows, full in ((2500, True), (40000, False)):
        for K in (4, 32):
            g = torch.Generator().manual_seed(rows + K)
            x = (torch.randn(rows, K, generator=g) * 3).to(dev)
            sup = torch.sort(torch.randn(K, generator=g) * 3).values.to(dev)
            t = (torch.randn(rows, generator=g) * 3).to(dev)
            scale = 1.0 / rows
            loss, mean = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
            dl, b = torch.empty(rows, K, device=dev), torch.empty(rows, dtype=torch.int32, device=dev)

            def ours():
                if full:
                    hip.call('dm_head_loss_catsup', rows, 1, K, hip.fptr(x), K, hip.fptr(sup), hip.fptr(t), scale, hip.fptr(loss),
                             hip.fptr(dl), hip.fptr(mean), hip.ptr(b), hip.stream())
                else:
                    hip.call('dm_head_loss_catsup', rows, 1, K, hip.fptr(x), K, hip.fptr(sup), None, 0.0, None, None, hip.fptr(mean),
                             None, hip.stream())

            def composed():
                if not full:
                    return None, None, torch.softmax(x, -1) @ sup, None
                bb = torch.square(t[:, None] - sup).argmin(-1)
                lp = F.log_softmax(x, -1)
                p = lp.exp()
                return -lp.gather(-1, bb[:, None])[:, 0], scale * (p - F.one_hot(bb, K)), p @ sup, bb
            ours()
            r_loss, r_dl, r_mean, r_b = composed()
            torch.cuda.synchronize()
            err = dict(mean=float((mean - r_mean).abs().max()))
            if full:
                err.update(loss=float((loss - r_loss).abs().max()), dlogits=float((dl - r_dl).abs().max()),
                           bins_equal=bool(torch.equal(b.long(), r_b)))
            nbytes = 4 * (rows * K + rows) + (4 * (rows * K + 3 * rows) if full else 0)
            out.append(dict(rows=rows, K=K, form='full' if full else 'mean-only', kernel_us=round(timed(ours, args.iters), 3),
                            torch_composition_us=round(timed(composed, args.iters), 3), bytes=nbytes,
                            hbm_bound_us=round(1e6 * nbytes / HBM_STREAM_BYTES_PER_S, 4), max_abs_diff=err))
    print(json.dumps(dict(mode='kernel', iters=args.iters, cases=out)))


def step_mode(args, config, Dreamer, dev):
    kw = dict(reward_decoder_categorical=[-10, 0, 1, 10]) if args.categorical else {}
    conf = config.atari_literal(**kw)
    T, B, A = conf.batch_length, conf.batch_size, conf.action_dim
    torch.manual_seed(0)
    model = Dreamer(conf).to(dev)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    gen = torch.Generator().manual_seed(1234)
    ring = []
    for _ in range(4):      # sparse, heavy-tailed rewards under the section's tanh clip
        raw = torch.tensor([-10.0, 0.0, 1.0, 10.0])[torch.multinomial(torch.tensor([0.02, 0.9, 0.06, 0.02]), T * B, True, generator=gen)]
        ring.append(dict(image=torch.randint(0, 256, (T, B, 64, 64, 3), generator=gen, dtype=torch.uint8).to(dev),
                         action=F.one_hot(torch.randint(0, A, (T, B), generator=gen), A).float().to(dev),
                         reward=torch.tanh(raw).view(T, B).to(dev),
                         terminal=(torch.rand(T, B, generator=gen) < 0.01).float().to(dev),
                         reset=(torch.rand(T, B, generator=gen) < 0.005).to(dev)))
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
    loss_model, loss_reward = float(metrics['loss_model']), float(metrics['loss_reward'])
    assert loss_model == loss_model, 'loss_model is NaN'
    print(json.dumps(dict(mode='step', shape=dict(B=B, T=T, H=conf.imag_horizon, deter_dim=conf.deter_dim), categorical=bool(args.categorical),
                          root=os.path.basename(os.path.abspath(args.root)), steps_per_region=args.steps, warmup=args.warmup,
                          ms_per_step_regions=[round(v, 4) for v in region_ms],
                          ms_per_step_median=round(sorted(region_ms)[len(region_ms) // 2], 4),
                          spread_ms=round(max(region_ms) - min(region_ms), 4), loss_model=loss_model, loss_reward=loss_reward)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('kernel', 'step'))
    ap.add_argument('--categorical', type=int, default=1)
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from pydreamer_amd import config, hip
    from pydreamer_amd.models import Dreamer
    if not torch.cuda.is_available():
        raise SystemExit('reward_categorical_bench: no GPU - a time is measured on the MI355X or not at all')
    hip.call('dm_device_check')
    dev = torch.device('cuda:0')
    if args.mode == 'kernel':
        kernel_mode(args, hip, dev)
    else:
        step_mode(args, config, Dreamer, dev)


if __name__ == '__main__':
    main()
