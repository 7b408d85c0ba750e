"""Plan2Explore (expl_behavior='plan2explore') at the Atari-literal shape - B=50, T=50, H=15, deter 600, K=10, fp32.

    python scripts/explore_bench.py step --explore 0
    python scripts/explore_bench.py step --explore 1
    python scripts/explore_bench.py parts
    python scripts/explore_bench.py kernels

step     the trainer iteration as train.run orders it: Dreamer.training_step, (Plan2Explore.training_step,) the backward passes,
         grad_clip and the AdamW steps of the Dreamer (and of the exploration groups); --regions regions of --steps iterations
         between device events after --warmup; ms per iteration of every region, the median and the spread.
parts    the exploration step's pieces, each alone between device events over --iters calls on the buffers of one real step: the
         ensemble forward + loss + backward on (T-1) B = 2 450 rows, the second imagination rollout (with its reward, terminal and
         value heads), the K head forwards over the H M = 37 500 imagined rows (with the [feature | action] row copies),
         dm_disag_reward over them, the second actor-critic update (losses, both backward passes).
kernels  dm_disag_reward at (K, rows, D) = (10, 37 500, 1 024) and dm_ensemble_mse at (10, 2 450, 1 024) alone, with the bytes each
         must move (means in, rewards out; means and target in, loss and dmeans out) and the rate that is.
One JSON line per run.
"""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters      # microseconds per call


def build(explore, dev):
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    conf = config.atari_literal(expl_behavior='plan2explore' if explore else 'greedy')
    T, B, A = conf.batch_length, conf.batch_size, conf.action_dim
    torch.manual_seed(0)
    model = Dreamer(conf).to(dev)
    opts = list(model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps))
    p2e, eopts = None, []
    if explore:
        from pydreamer_amd.explore import Plan2Explore
        p2e = Plan2Explore(conf, model).to(dev)
        eopts = list(p2e.init_optimizers())
    gen = torch.Generator().manual_seed(1234)
    ring = []
    for _ in range(4):
        ring.append(dict(image=torch.randint(0, 256, (T, B, 64, 64, 3), generator=gen, dtype=torch.uint8).to(dev),
                         action=F.one_hot(torch.randint(0, A, (T, B), generator=gen), A).float().to(dev),
                         reward=torch.tanh(torch.randn(T, B, generator=gen)).to(dev),
                         terminal=(torch.rand(T, B, generator=gen) < 0.01).float().to(dev),
                         reset=(torch.rand(T, B, generator=gen) < 0.005).to(dev)))
    return conf, model, opts, p2e, eopts, ring


def iteration(conf, model, opts, p2e, eopts, obs, state):
    losses, state, metrics, _, _ = model.training_step(obs, state)
    elosses = ()
    if p2e is not None:
        elosses, emetrics = p2e.training_step()
        metrics = {**metrics, **emetrics}
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
    for opt in opts:
        opt.step()
    if p2e is not None:
        for opt in eopts:
            opt.zero_grad()
        for loss in elosses:
            loss.backward()
        p2e.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in eopts:
            opt.step()
    return state, metrics


def step_mode(args, dev):
    conf, model, opts, p2e, eopts, ring = build(args.explore, dev)
    state = model.init_state(conf.batch_size)
    n = 0
    for _ in range(args.warmup):
        state, metrics = iteration(conf, model, opts, p2e, eopts, ring[n % 4], state)
        n += 1
    torch.cuda.synchronize()
    region_ms = []
    for _ in range(args.regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            state, metrics = iteration(conf, model, opts, p2e, eopts, ring[n % 4], state)
            n += 1
        e1.record()
        e1.synchronize()
        region_ms.append(e0.elapsed_time(e1) / args.steps)
    out = dict(mode='step', explore=bool(args.explore), shape=dict(B=conf.batch_size, T=conf.batch_length, H=conf.imag_horizon,
                                                                   deter_dim=conf.deter_dim, K=conf.disag_models),
               steps_per_region=args.steps, warmup=args.warmup, ms_per_step_regions=[round(v, 4) for v in region_ms],
               ms_per_step_median=round(sorted(region_ms)[len(region_ms) // 2], 4), spread_ms=round(max(region_ms) - min(region_ms), 4),
               loss_model=float(metrics['loss_model']))
    if p2e is not None:
        out.update(loss_disag=float(metrics['loss_disag']), expl_reward=float(metrics['expl_reward']))
    assert out['loss_model'] == out['loss_model'], 'loss_model is NaN'
    print(json.dumps(out))


def parts_mode(args, dev):
    from pydreamer_amd import hip as H
    from pydreamer_amd.models import _ProbeLoss
    conf, model, opts, p2e, eopts, ring = build(1, dev)
    state = model.init_state(conf.batch_size)
    for i in range(3):
        state, _ = iteration(conf, model, opts, p2e, eopts, ring[i], state)
    model.training_step(ring[3], state)
    torch.cuda.synchronize()
    feat = p2e.step_features()
    pk = model.wm._last_pack
    T, B = pk['action'].shape[:2]
    N, K, Dt, F_ = (T - 1) * B, p2e.K, p2e.target_dim, p2e.features_dim
    Hh = conf.imag_horizon

    def ensemble():
        x, ldx = p2e._rows(feat, F_, pk['action'].view(T * B, -1)[B:], N)
        ws = p2e._workspace(N, dev)
        means, dmeans, loss = torch.empty(K, N, Dt, device=dev), torch.empty(K, N, Dt, device=dev), torch.empty(K, N, device=dev)
        packs = []
        for k, head in enumerate(p2e.heads):
            acts = torch.empty(head.acts_floats(N), device=dev)
            head.fwd(x, ldx, N, ws, acts=acts, window=(N, 0), out=means[k])
            packs.append(dict(mlp=head, x=x, ldx=ldx, rows=N, acts=acts, dout=dmeans[k], ws=ws))
        H.call('dm_ensemble_mse', K, N, Dt, H.fptr(means), N * Dt, Dt, ctypes.c_void_p(feat.data_ptr() + 4 * (B * F_ + p2e.deter_dim)), F_,
               H.ptr(pk['reset'].view(T * B)[B:]), 1.0 / N, H.fptr(loss), H.fptr(dmeans), H.stream())
        eopts[0].zero_grad()
        _ProbeLoss.apply(p2e.ensemble, dict(loss=loss.sum(), heads=packs), *p2e.ensemble.parameters()).backward()

    dpk = {}

    def rollout():
        dpk.clear()
        with torch.no_grad():
            return model._dream_from_features(feat, Hh, _pack=dpk, ac=p2e.ac)
    feats_d, actions_d, rewards_d, terminals_d = rollout()
    M = feats_d.shape[1]
    rows = Hh * M
    f2, a2 = feats_d.view(-1, F_)[:rows], actions_d.view(rows, -1)
    from pydreamer_amd.explore import _CHUNK_FLOATS
    chunk = max(1, min(rows, _CHUNK_FLOATS // (K * Dt)))
    means = torch.empty(K, chunk, Dt, device=dev)
    xbuf = torch.empty(chunk, p2e.in_dim, device=dev)
    out = torch.zeros(Hh + 1, M, device=dev)

    def heads():
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            p2e.predict(f2[r0:r0 + n], a2[r0:r0 + n], means=means, xbuf=xbuf)

    def disag():
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            H.call('dm_disag_reward', K, n, Dt, H.fptr(means), chunk * Dt, Dt, 1.0, H.fptr(out.view(-1)[M + r0:M + r0 + n]), H.stream())
    rewards = p2e.intrinsic_reward(feats_d, actions_d)

    def ac_update():
        (la, lc), _, _ = p2e.ac.training_step(feats_d, actions_d, rewards, terminals_d.mean, act_idx=dpk['act_idx'], ws=dpk['ws'],
                                              actor_acts=dpk['actor_acts'], actor_logits=dpk['actor_logits'], values=dpk['values'],
                                              _begun=True)
        eopts[1].zero_grad()
        eopts[2].zero_grad()
        la.backward()
        lc.backward()

    res = dict(mode='parts', iters=args.iters, rows_ensemble=N, rows_imagined=rows, K=K, D=Dt, chunk_rows=chunk,
               ensemble_fwd_loss_bwd_us=round(timed(ensemble, args.iters), 1), second_rollout_us=round(timed(rollout, args.iters), 1),
               head_forwards_us=round(timed(heads, args.iters), 1), disag_reward_us=round(timed(disag, args.iters), 1),
               second_ac_update_us=round(timed(ac_update, args.iters), 1))
    print(json.dumps(res))


def kernels_mode(args, dev):
    from pydreamer_amd import hip as H
    out = []
    K, D = 10, 1024
    rows = 37500
    means = torch.randn(K, rows, D, device=dev)
    reward = torch.empty(rows, device=dev)
    us = timed(lambda: H.call('dm_disag_reward', K, rows, D, H.fptr(means), rows * D, D, 1.0, H.fptr(reward), H.stream()), args.iters)
    nbytes = 4 * (K * rows * D + rows)
    out.append(dict(kernel='dm_disag_reward', K=K, rows=rows, D=D, us=round(us, 2), bytes=nbytes, GBps=round(nbytes / us / 1e3, 1)))
    rows = 2450
    means = torch.randn(K, rows, D, device=dev)
    feat = torch.randn(rows + 50, 600 + D, device=dev)
    skip = torch.rand(rows, device=dev) < 0.005
    loss, dmeans = torch.empty(K, rows, device=dev), torch.empty(K, rows, D, device=dev)
    target = ctypes.c_void_p(feat.data_ptr() + 4 * (50 * feat.shape[1] + 600))
    us = timed(lambda: H.call('dm_ensemble_mse', K, rows, D, H.fptr(means), rows * D, D, target, feat.shape[1], H.ptr(skip), 1.0 / rows,
                              H.fptr(loss), H.fptr(dmeans), H.stream()), args.iters)
    nbytes = 4 * (2 * K * rows * D + rows * D + K * rows) + rows
    out.append(dict(kernel='dm_ensemble_mse', K=K, rows=rows, D=D, us=round(us, 2), bytes=nbytes, GBps=round(nbytes / us / 1e3, 1)))
    print(json.dumps(dict(mode='kernels', iters=args.iters, cases=out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('step', 'parts', 'kernels'))
    ap.add_argument('--explore', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--regions', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('explore_bench.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    {'step': step_mode, 'parts': parts_mode, 'kernels': kernels_mode}[args.mode](args, dev)


if __name__ == '__main__':
    main()
