"""-m gpu: the two-hot critic and the percentile return normalisation inside the model, at the tiny shapes of the
oracle's tiny_conf (deter 64, stoch 8x8, T 5, B 3, H 4) with critic_bins in {7, 255}.

  * one Dreamer.training_step with critic_dist='twohot', without and with return_norm='percentile', against the float64
    restatement of tests/twohot_case.py run on the step's own dream (last_extras) and the same weights: loss_critic, loss_actor,
    value, value_target, the advantages and every actor / critic parameter gradient at the bars of test_gpu_training_step.py's
    actor-critic comparisons (losses 2e-5 relative or 2e-6, tensors 1e-4, gradients 2e-3 relative L2); ac.return_range follows
    the restated update, does not move under no_grad, and moves ONCE in a step that also runs the log dream (do_dream_tensors)
  * scale invariance: rewards r and 128 r give bit-equal actor gradient rows under the percentile scale, 128 x apart without it
  * Dreamer.act, Dreamer.inference and the planner's rollout value equal ActorCritic.value on the same features
  * a fresh two-hot critic values random features at |v| < 1e-5
  * twenty AdamW steps of ActorCritic.training_step on one fixed dream, both switches on, against the float64 restatement's
    trajectory; bound: 4 x the largest deviation of the same restatement in torch-fp32 on the CPU from its float64 run
  * save_checkpoint / load_checkpoint restores ac.return_range and the K-wide critic; the next step's losses are bit-equal
  * train.run on the tiny vectorenv loop logs train/policy_return_scale"""
import os
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dreamer_oracle as O
from pydreamer_amd import config
from tests import twohot_case as TC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _close(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})'


def _loss_close(a, b, what):
    a, b = float(a), float(b)
    print(f'{what}: {a:.9g} float64 {b:.9g}')
    assert abs(a - b) < 2e-5 * abs(b) or abs(a - b) < 2e-6, (what, a, b)


def _model(oconf, seed=0, **switches):
    """Dreamer on the oracle's closed-form parameters; a two-hot critic's K-wide output layers get their own closed-form values
    (a zero layer would leave nothing to compare), a tenth of the xavier range: with 7 bins over +-20 the full range decodes
    to values of +-1e5 (measured: loss_actor 1.4e5), where the fp32 cancellation inside the GAE sums - |v| 1e5, ulp 8e-3, against
    targets of order 10 - is the step's largest error (loss_critic off by 6e-5 relative) and hides what is compared here."""
    from pydreamer_amd.models import Dreamer
    model = Dreamer(config.load_config('defaults', 'atari', **{**vars(oconf), **switches}))
    params = O.make_params(oconf, seed=seed)
    if switches.get('critic_dist') == 'twohot':
        K, rs = switches['critic_bins'], np.random.RandomState(seed + 99)
        lim = 0.1 * np.sqrt(6.0 / (400 + K))
        for m in ('critic', 'critic_target'):
            params[f'ac.{m}.model.12.weight'] = torch.tensor(rs.uniform(-lim, lim, (K, 400)), dtype=torch.float32)
            params[f'ac.{m}.model.12.bias'] = torch.tensor(0.05 * rs.uniform(-1, 1, K), dtype=torch.float32)
    missing = model.load_state_dict(params, strict=False)
    assert set(missing.missing_keys) <= {'ac.return_range'} and not missing.unexpected_keys
    return model.to(DEV)


def _dream64(model, oconf):
    """The step's own dream in float64: features and actions from last_extras, reward and terminal means from the heads' weights."""
    xh = model.last_extras
    p = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    feats = xh['dream_features'].double().cpu()
    rewards = O.mlp(p, 'wm.decoder.reward.model.model', feats, oconf.reward_decoder_layers)
    terminals = torch.sigmoid(O.mlp(p, 'wm.decoder.terminal.model.model', feats, oconf.terminal_decoder_layers))
    return feats, xh['act_idx'].long().cpu(), rewards, terminals


def _step(model, opts, obs, state, noise, **kw):
    out = model.training_step(_to_dev(obs), state, noise=_to_dev(noise), **kw)
    for opt in opts:
        opt.zero_grad()
    for loss in out[0]:
        loss.backward()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('K', [7, 255])
@pytest.mark.parametrize('norm', ['none', 'percentile'])
def test_training_step_against_float64(hip, K, norm):
    oconf = O.tiny_conf()
    model = _model(oconf, critic_dist='twohot', critic_bins=K, return_norm=norm)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs, noise = O.preprocess(O.synthetic_batch(oconf), oconf), O.make_noise(oconf)
    state = model.init_state(oconf.batch_size)
    range0 = torch.tensor([-0.5, 1.0])
    if norm == 'percentile':
        model.ac.return_range.copy_(range0)
    losses, _, metrics, tensors, _ = _step(model, opts, obs, state, noise)
    ta = model.last_extras['ac_tensors']
    p = TC.ac_params(model.ac, torch.float64)
    (la, lc), t64, range64 = TC.ac_step(p, model.ac, *_dream64(model, oconf), return_range=range0.double())
    la.backward()
    lc.backward()
    _loss_close(losses[2], la, f'K={K} {norm} loss_actor')
    _loss_close(losses[3], lc, f'K={K} {norm} loss_critic')
    _loss_close(metrics['loss_critic'], lc, 'metric loss_critic')
    _loss_close(metrics['policy_value'], t64['value'][0].mean(), 'policy_value')
    _loss_close(metrics['policy_value_im'], t64['value'][:-1].mean(), 'policy_value_im')
    for k in ('value', 'value_target', 'value_advantage', 'value_advantage_gae', 'value_weight'):
        _close(ta[k], t64[k], 1e-4, 1e-4 * max(1.0, float(t64[k].abs().max())), f'tensor {k}')
    assert torch.equal(tensors['policy_value'].reshape(-1), ta['value'][0].reshape(-1))
    worst = ('', 0.0)
    for name, q in model.ac.named_parameters():
        if not q.requires_grad:
            continue
        e = _rel_l2(q.grad, p[f'ac.{name}'].grad)
        worst = max(worst, (name, e), key=lambda v: v[1])
    print(f'K={K} {norm}: worst gradient rel-L2 {worst[1]:.2e} at {worst[0]}')
    assert worst[1] < 2e-3, worst
    if norm == 'none':
        assert 'policy_return_scale' not in metrics and 'policy_return_scale' not in model.packed_metrics()[0]
        return
    # the running range: one restated update; logged; unchanged under no_grad; moved once by a step with the log dream
    got = model.ac.return_range.double().cpu()
    print(f'return_range {got.tolist()} float64 {range64.tolist()} scale {float(t64["scale"]):.6g}')
    assert torch.allclose(got, range64, rtol=1e-5, atol=1e-6)
    host = model.packed_metrics_host()
    assert host['policy_return_lo'] == float(model.ac.return_range[0]) and host['policy_return_hi'] == float(model.ac.return_range[1])
    assert abs(host['policy_return_scale'] - float(t64['scale'])) <= 1e-5 * float(t64['scale'])
    assert float(metrics['policy_return_scale']) == host['policy_return_scale']
    before = model.ac.return_range.clone()
    with torch.no_grad():
        model.training_step(_to_dev(obs), state, noise=_to_dev(noise), do_dream_tensors=True)
    assert torch.equal(model.ac.return_range, before), 'no update without gradients'
    _, _, _, _, dream_tensors = _step(model, opts, obs, state, noise, do_dream_tensors=True)
    assert 'value' in dream_tensors
    vt = model.last_extras['ac_tensors']['value_target'].double().cpu().flatten()
    q = torch.quantile(vt, torch.tensor(model.ac.return_norm_q, dtype=torch.float64))
    want = 0.99 * before.double().cpu() + (1 - 0.99) * q
    assert torch.allclose(model.ac.return_range.double().cpu(), want, rtol=1e-5, atol=1e-6), 'one update: the log dream does not move it'


def _fixed_dream(J, M, Fd, A, seed, reward_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(J, M, Fd, generator=g)
    act_idx = torch.randint(0, A, (J - 1, M), generator=g)
    rewards = torch.randn(J, M, generator=g) * 2 * reward_scale
    terminals = (torch.rand(J, M, generator=g) < 0.1).float() * 0.75
    return feats, act_idx, rewards, terminals


def _ws():
    return torch.empty(256 << 20, dtype=torch.uint8, device=DEV)


def test_percentile_scale_makes_the_actor_gradient_scale_invariant(hip):
    from pydreamer_amd.models import ActorCritic
    J, M, Fd, A = 5, 40, 48, 6
    rows = {}
    for norm in ('percentile', 'none'):
        for mult in (1.0, 128.0):
            torch.manual_seed(0)
            ac = ActorCritic(in_dim=Fd, out_actions=A, entropy_weight=0.0, return_norm=norm, return_norm_decay=0.0).to(DEV)
            with torch.no_grad():      # an mse critic that values every state at exactly 0
                ac.critic.model[12].weight.zero_()
                ac.critic.model[12].bias.zero_()
            feats, act_idx, rewards, terminals = _fixed_dream(J, M, Fd, A, seed=3)
            ac.training_step(feats.to(DEV), F.one_hot(act_idx, A).float().to(DEV), (rewards * mult).to(DEV), terminals.to(DEV), ws=_ws())
            torch.cuda.synchronize()
            rows[norm, mult] = ac._last_packs[0]['dout'].clone()
            if norm == 'percentile':
                lo, hi = ac.return_range.tolist()
                assert hi - lo >= mult, 'the range is above the limit, so the scale is the range'
    assert rows['percentile', 1.0].abs().max() > 0
    assert torch.equal(rows['percentile', 1.0], rows['percentile', 128.0]), 'every scaling is a power of two: the same bits'
    assert torch.equal(rows['none', 1.0] * 128, rows['none', 128.0]), 'the control: 128 x apart without the normalisation'
    assert not torch.equal(rows['none', 1.0], rows['none', 128.0])


@pytest.mark.parametrize('K', [7, 255])
def test_acting_and_planning_use_the_decoded_value(hip, K):
    from pydreamer_amd.planner import CEMPlanner
    oconf = O.tiny_conf()
    model = _model(oconf, critic_dist='twohot', critic_bins=K)
    obs = {k: v[:1] for k, v in _to_dev(O.preprocess(O.synthetic_batch(oconf), oconf)).items()}
    B, state = oconf.batch_size, model.init_state(oconf.batch_size)
    u_post = torch.rand(1, B, oconf.stoch_dim, device=DEV)
    with torch.no_grad():
        features, _ = model.wm.forward(obs, state, u_post)
        feat = features.reshape(B, -1).contiguous()
        want, _ = model.ac.value(feat, feat.shape[1], B, _ws(), sparse=False)
    assert want.shape == (B, 1)
    p = {f'ac.{k}': v.detach().double().cpu() for k, v in model.ac.state_dict().items()}
    v64 = TC.twohot_decode(O.mlp(p, 'ac.critic.model', feat.double().cpu(), 4), model.ac.bins.double().cpu())
    _close(want.view(B), v64, 1e-4, 1e-4, 'ActorCritic.value against float64')
    _, _, m = model.act(obs, state, noise=dict(u_post=u_post), return_rows=True)
    assert torch.equal(m['value'], want.view(B))
    assert abs(float(m['policy_value']) - float(want.mean())) <= 1e-5 * (1 + abs(float(want.mean())))
    with torch.no_grad():
        _, _, mi = model.inference(obs, state, noise=dict(u_post=u_post))
    assert torch.equal(mi['policy_value'], want.mean())
    planner = CEMPlanner(model, horizon=3, candidates=8, elites=2, iters=2)
    roll = planner.plan(feat, keep_rollout=True)['rollout']
    last = roll['features'][-1]
    for b in range(B):
        rows = last[b * 8:(b + 1) * 8].contiguous()
        v, _ = model.ac.value(rows, rows.shape[1], 8, _ws())
        assert torch.equal(roll['value'][b * 8:(b + 1) * 8], v.view(8)), b
    v64 = TC.twohot_decode(O.mlp(p, 'ac.critic.model', last.double().cpu(), 4), model.ac.bins.double().cpu())
    _close(roll['value'], v64, 1e-4, 1e-4, 'planner value against float64')


def test_a_fresh_twohot_critic_values_everything_at_zero(hip):
    from pydreamer_amd.models import ActorCritic
    for K in (7, 255, 256):
        torch.manual_seed(K)
        ac = ActorCritic(in_dim=96, out_actions=4, critic_dist='twohot', critic_bins=K).to(DEV)
        v, _ = ac.value(torch.randn(70, 96, device=DEV), 96, 70, _ws(), sparse=False)
        print(f'K={K}: fresh critic max |v| {float(v.abs().max()):.3e}')
        assert float(v.abs().max()) < 1e-5


def test_twenty_step_trajectory_against_float64(hip):
    from pydreamer_amd.models import ActorCritic
    from pydreamer_amd.optim import FusedAdamW
    J, M, Fd, A, K, steps, lr, eps = 5, 24, 48, 6, 31, 20, 1e-3, 1e-5
    torch.manual_seed(1)
    ac = ActorCritic(in_dim=Fd, out_actions=A, gamma=0.99, entropy_weight=1e-3, critic_dist='twohot', critic_bins=K,
                     return_norm='percentile').to(DEV)
    feats, act_idx, rewards, terminals = _fixed_dream(J, M, Fd, A, seed=5)
    start = {dt: TC.ac_params(ac, dt) for dt in (torch.float64, torch.float32)}

    def restated(dt):
        p = start[dt]
        groups = [[v for k, v in p.items() if k.startswith(f'ac.{m}.')] for m in ('actor', 'critic')]
        opts = [torch.optim.AdamW(g, lr=lr, eps=eps) for g in groups]
        rng, out = torch.zeros(2, dtype=dt), []
        for s in range(steps):
            if s == 0:      # the target network's refresh (a2c.py:76-79; target_interval 100)
                with torch.no_grad():
                    for k in p:
                        if k.startswith('ac.critic_target.'):
                            p[k].copy_(p[k.replace('critic_target', 'critic')])
            (la, lc), _, rng = TC.ac_step(p, ac, feats.to(dt), act_idx, rewards.to(dt), terminals.to(dt), return_range=rng)
            rng = rng.detach()
            for o in opts:
                o.zero_grad()
            la.backward()
            lc.backward()
            for o in opts:
                o.step()
            out.append((float(la), float(lc)))
        return np.array(out)

    ref, f32 = restated(torch.float64), restated(torch.float32)
    oa = FusedAdamW(list(ac.actor.parameters()), lr=lr, eps=eps)
    oc = FusedAdamW(list(ac.critic.parameters()), lr=lr, eps=eps)
    ac.actor._fused, ac.critic._fused = oa, oc
    dev = (feats.to(DEV), F.one_hot(act_idx, A).float().to(DEV), rewards.to(DEV), terminals.to(DEV))
    ws, got = _ws(), []
    for s in range(steps):
        (la, lc), _, _ = ac.training_step(*dev, ws=ws)
        for o in (oa, oc):
            o.zero_grad()
        la.backward()
        lc.backward()
        for o in (oa, oc):
            o.step()
        got.append((float(la), float(lc)))
    got = np.array(got)
    for c, name in enumerate(('loss_actor', 'loss_critic')):
        dev32, devgpu = np.abs(f32[:, c] - ref[:, c]).max(), np.abs(got[:, c] - ref[:, c]).max()
        print(f'{name}: first {ref[0, c]:.6g} last {ref[-1, c]:.6g}; fp32-CPU deviation {dev32:.3e}, GPU deviation {devgpu:.3e}')
    assert ref[-1, 1] < ref[0, 1], 'the critic learns the fixed targets'
    for c, name in enumerate(('loss_actor', 'loss_critic')):
        assert np.abs(got[:, c] - ref[:, c]).max() <= 4 * np.abs(f32[:, c] - ref[:, c]).max(), name


def test_checkpoint_round_trip(hip, tmp_path):
    from pydreamer_amd.train import load_checkpoint, save_checkpoint
    oconf = O.tiny_conf()
    sw = dict(critic_dist='twohot', critic_bins=7, return_norm='percentile')
    obs, noise = O.preprocess(O.synthetic_batch(oconf), oconf), O.make_noise(oconf)

    def trainer(seed):
        model = _model(oconf, seed=seed, **sw)
        return model, model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)

    model, opts = trainer(0)
    state = model.init_state(oconf.batch_size)
    for _ in range(2):
        _step(model, opts, obs, state, noise)
        model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        for opt in opts:
            opt.step()
    assert model.ac.return_range.abs().sum() > 0
    path = str(tmp_path / 'latest.pt')
    save_checkpoint(path, model, opts, 2)
    assert 'ac.return_range' in torch.load(path, map_location='cpu')['model_state_dict']
    fresh, fopts = trainer(1)
    assert load_checkpoint(path, fresh, fopts, map_location=DEV) == 2
    fresh.ac.train_steps = model.ac.train_steps      # (the step counter is the trainer's, not the checkpoint's)
    assert torch.equal(fresh.ac.return_range, model.ac.return_range)
    for k in ('ac.critic.model.12.weight', 'ac.critic_target.model.12.bias'):
        assert fresh.state_dict()[k].shape[0] == 7 and torch.equal(fresh.state_dict()[k], model.state_dict()[k])
    a = _step(model, opts, obs, state, noise)[0]
    b = _step(fresh, fopts, obs, state, noise)[0]
    for x, y in zip(a, b):
        assert torch.equal(x, y), (float(x), float(y))
    assert torch.equal(fresh.ac.return_range, model.ac.return_range)


def test_the_trainer_logs_the_return_scale(hip, tmp_path):
    from pydreamer_amd import replay as R
    from pydreamer_amd.train import run
    from tests.test_gpu_train_loop import LoopEnv, _loop_conf
    conf = Namespace(**{**vars(_loop_conf()), **dict(critic_dist='twohot', critic_bins=7, return_norm='percentile', eval_interval=1000)})
    data_dir = str(tmp_path / 'episodes')
    os.makedirs(data_dir)
    repo = R.LocalEpisodeRepository(data_dir)
    envs = [LoopEnv(b, lengths, conf.action_dim, conf.vecobs_size) for b, lengths in enumerate([[11, 12], [12, 10], [13, 11, 10]])]
    logged = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        steps = run(conf, repo, test_repository=repo, envs=envs, logdir=str(tmp_path / 'log'), logger=lambda m, s: logged.append((s, dict(m))),
                    env_steps_per_grad_step=3, seed=1, steps_per_npz=10)
    assert steps == 6
    train = [m for _, m in logged if 'train/steps' in m]
    assert len(train) == 2
    for m in train:
        assert m['train/policy_return_scale'] >= 1.0 and m['train/policy_return_hi'] >= m['train/policy_return_lo']
        assert np.isfinite(m['train/loss_critic']) and 'train/policy_return_scale_max' not in m
