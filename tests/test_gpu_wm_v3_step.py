"""-m gpu: free bits (kl_free) and the symlog two-hot reward head (reward_dist='twohot') inside the model, at the tiny
shapes of the oracle's tiny_conf (deter 64, stoch 8x8, T 5, B 3, H 4); the dense and the image-less cases at the sizes of the
tiny minigrid / vectorenv fixtures.  The float64 side is tests/wm_v3_case.py, fed the step's own posterior indices (forced_idx);
the bars are those tests/test_gpu_twohot_critic.py takes from tests/test_gpu_training_step.py: losses 2e-5 relative or 2e-6,
tensors 1e-4, every world-model gradient 2e-3 relative L2.

Free bits
  * kl_free below every row's KL: the four losses, every world-model gradient and every metric of the switch-off step are
    torch.equal; kl_free_frac == 0
  * kl_free above every row's KL: every world-model gradient torch.equal to a kl_weight = 0 step's; kl_free_frac == 1;
    loss_kl_clip = kl_free and loss_model = the kl_weight = 0 step's + kl_weight kl_free, to the loss bar
  * kl_free in the widest gap of the central third of the float64 row KLs (the gap condition asserted): loss_model, loss_kl,
    loss_kl_clip, the tensors and every world-model gradient against float64 - categorical latents, Gaussian latents,
    kl_balance = 0.5
  * the tail on the side stream (B = 16) bit-identical to the tail on the caller's stream; iwae_samples = 2 refused
The two-hot reward head
  * K in {7, 255} (and K = 7 under iwae_samples = 2) with the output layer filled with small closed-form values: loss_reward,
    reward_rec, loss_model and every world-model gradient (the head's, and through the features everything in front) against float64
  * do_image_pred gives logprob_reward, logprob_reward-1 / 1 and reward_pred; the dream's reward (and the log dream's reward_pred)
    torch.equal to the mean-only kernel on the dream's own logits, the planner's against float64 on its own features
    (Dreamer.inference reads no reward); a fresh head predicts |reward| < 1e-5; rewards x 128 keep loss_reward of order log K
  * one step with both switches on: convolution path with aux_critic, dense image path, image-less path, amp - finite, a gradient
    in every tensor of the head
  * checkpoint round trip: the next step's losses bit-equal; train.run logs train/kl_free_frac and train/loss_kl_clip"""
import ast
import math
import os
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import dreamer_oracle as O
from pydreamer_amd import config
from tests import twohot_case as TC
from tests import wm_v3_case as WC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
HEAD = 'wm.decoder.reward.model.model'


def _to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _close(a, b, what, rtol=1e-4, atol=1e-4):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    err = (a - b).abs()
    bad = err > atol * max(1.0, float(b.abs().max())) + rtol * b.abs()
    assert not bad.any() and not torch.isnan(err).any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e}'


def _loss_close(a, b, what):
    a, b = (float(x.detach()) if torch.is_tensor(x) else float(x) for x in (a, b))
    print(f'{what}: {a:.9g} reference {b:.9g}')
    assert abs(a - b) < 2e-5 * abs(b) or abs(a - b) < 2e-6, (what, a, b)


def _model(oconf, seed=0, **switches):
    """Dreamer on the oracle's closed-form parameters; a two-hot reward head's K-wide output layer gets its own closed-form values."""
    from pydreamer_amd.models import Dreamer
    model = Dreamer(config.load_config('defaults', 'atari', **{**vars(oconf), **switches}))
    params = O.make_params(oconf, seed=seed)
    if switches.get('reward_dist') == 'twohot':
        params[f'{HEAD}.12.weight'], params[f'{HEAD}.12.bias'] = WC.head_output_layer(switches.get('reward_twohot_bins', 255), seed)
    missing = model.load_state_dict(params, strict=False)
    assert not missing.missing_keys and not missing.unexpected_keys
    return model.to(DEV)


def _batch(oconf, reward_scale=1.0):
    obs = O.preprocess(O.synthetic_batch(oconf), oconf)
    obs['reward'] = obs['reward'] * reward_scale
    return obs, O.make_noise(oconf)


def _step(model, oconf, obs, noise, **kw):
    """One training_step with its four backward passes; returns (losses, metrics, tensors, dream_tensors, wm gradients)."""
    if not hasattr(model, '_opts'):
        model._opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    state = model.init_state(oconf.batch_size * kw.get('iwae_samples', oconf.iwae_samples))
    losses, _, metrics, tensors, dream_tensors = model.training_step(_to_dev(obs), state, noise=_to_dev(noise), **kw)
    for opt in model._opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().clone() for k, v in model.wm.named_parameters() if v.requires_grad and v.grad is not None}
    return losses, {k: v.clone() for k, v in metrics.items()}, tensors, dream_tensors, grads


def _float64(model, oconf, obs, noise, kl_free=0.0, I=1):
    """tests/wm_v3_case.wm_step on the model's weights and the step's own posterior indices; returns (loss, metrics, tensors, p)."""
    p = {k: v.detach().double().cpu().requires_grad_(k.startswith('wm.')) for k, v in model.state_dict().items()}
    obs64 = {k: (v.double() if v.is_floating_point() else v) for k, v in obs.items()}
    B, Z = oconf.batch_size * I, oconf.stoch_dim * (oconf.stoch_discrete or 1)
    state = (torch.zeros(B, oconf.deter_dim, dtype=torch.float64), torch.zeros(B, Z, dtype=torch.float64))
    head = model.wm.decoder.reward
    bins = head.bins.double().cpu() if hasattr(head, 'bins') else None
    if oconf.stoch_discrete:
        fidx, u_post = model.last_extras['post_idx'].long().cpu(), None
    else:
        fidx, u_post = None, noise['u_post'].double()
    loss, metrics, tensors = WC.wm_step(p, oconf, obs64, state, fidx, kl_free=kl_free, reward_bins=bins, u_post=u_post, iwae_samples=I)
    loss.backward()
    return loss, metrics, tensors, p


def _compare(model, got, ref, metric_keys, tensor_keys, tag):
    losses, metrics, tensors, _, grads = got
    loss64, m64, t64, p = ref
    _loss_close(losses[0], loss64, f'{tag} loss_model')
    for k in metric_keys:
        _loss_close(metrics[k], m64[k], f'{tag} {k}')
    for k in tensor_keys:
        _close(tensors[k], t64[k], f'{tag} tensor {k}')
    worst = ('', 0.0)
    for k, g in grads.items():
        worst = max(worst, (k, _rel_l2(g, p[f'wm.{k}'].grad)), key=lambda v: v[1])
    print(f'{tag}: worst world-model gradient rel-L2 {worst[1]:.2e} at {worst[0]} ({len(grads)} tensors)')
    assert len(grads) == sum(1 for k in p if k.startswith('wm.')) and worst[1] < 2e-3, worst


# ---------------------------------------------------------------------------------------------- free bits
@pytest.fixture(scope='module')
def off_step(hip):
    """The switch-off step every free-bits case starts from: its row KLs choose kl_free."""
    oconf = O.tiny_conf()
    obs, noise = _batch(oconf)
    model = _model(oconf)
    out = _step(model, oconf, obs, noise)
    return dict(oconf=oconf, obs=obs, noise=noise, out=out, kl=out[2]['loss_kl'].double().cpu(), names=model.packed_metrics()[0])


def test_free_bits_below_every_row(hip, off_step):
    oconf, obs, noise = off_step['oconf'], off_step['obs'], off_step['noise']
    free = 0.5 * float(off_step['kl'].min())
    assert free > 1e-3
    model = _model(oconf, kl_free=free)
    losses, metrics, tensors, _, grads = _step(model, oconf, obs, noise)
    l0, m0, t0, _, g0 = off_step['out']
    for a, b in zip(losses, l0):
        assert torch.equal(a, b), (float(a), float(b))
    assert set(metrics) == set(m0) | {'loss_kl_clip', 'kl_free_frac'}
    for k, v in m0.items():
        assert torch.equal(metrics[k], v), k
    assert float(metrics['kl_free_frac']) == 0.0 and torch.equal(metrics['loss_kl_clip'], metrics['loss_kl'])
    assert torch.equal(tensors['loss_kl_clip'], tensors['loss_kl']) and torch.equal(tensors['loss_kl'], t0['loss_kl'])
    assert grads.keys() == g0.keys()
    for k in g0:
        assert torch.equal(grads[k], g0[k]), k
    names, _, idx = model.packed_metrics()
    assert names == off_step['names'] + ['loss_kl_clip', 'kl_free_frac'] and idx[-2:] == [45, 46]
    host = model.packed_metrics_host()
    assert host['kl_free_frac'] == 0.0 and host['loss_kl_clip'] == float(metrics['loss_kl'])
    assert float(off_step['out'][1]['loss_kl']) > 0 and 'kl_free_frac' not in off_step['names']


def test_free_bits_above_every_row(hip, off_step):
    oconf, obs, noise = off_step['oconf'], off_step['obs'], off_step['noise']
    free = 2.0 * float(off_step['kl'].max())
    model = _model(oconf, kl_free=free)
    losses, metrics, tensors, _, grads = _step(model, oconf, obs, noise)
    zconf = O.tiny_conf(kl_weight=0.0)
    lz, mz, _, _, gz = _step(_model(zconf), zconf, obs, noise)
    assert float(metrics['kl_free_frac']) == 1.0
    _loss_close(metrics['loss_kl_clip'], free, 'loss_kl_clip against kl_free')
    assert bool((tensors['loss_kl_clip'] == torch.tensor(free, dtype=torch.float32)).all())
    assert torch.equal(metrics['loss_kl'], off_step['out'][1]['loss_kl']), 'loss_kl stays the exact KL'
    _loss_close(losses[0], float(lz[0].detach()) + oconf.kl_weight * free, 'loss_model against the kl_weight = 0 step + kl_weight kl_free')
    assert grads.keys() == gz.keys()
    for k in gz:
        assert torch.equal(grads[k], gz[k]), k
    assert any(not torch.equal(grads[k], off_step['out'][4][k]) for k in grads), 'the control: the switch-off gradients differ'


@pytest.mark.parametrize('extra', [dict(), dict(stoch_discrete=0, stoch_dim=16), dict(kl_balance=0.5)],
                         ids=['categorical', 'gaussian_latents', 'kl_balance_half'])
def test_free_bits_mid_against_float64(hip, extra):
    oconf = O.tiny_conf(**extra)
    obs, noise = _batch(oconf)
    probe = _model(oconf)
    _step(probe, oconf, obs, noise)
    kl64 = _float64(probe, oconf, obs, noise)[2]['loss_kl']
    free, gap = WC.mid_free(kl64.numpy())
    WC.assert_gap(free, gap)
    idx0 = probe.last_extras['post_idx'].clone()
    model = _model(oconf, kl_free=free)
    got = _step(model, oconf, obs, noise)
    assert torch.equal(model.last_extras['post_idx'], idx0)
    ref = _float64(model, oconf, obs, noise, kl_free=free)
    frac64 = float(ref[1]['kl_free_frac'])
    print(f'{extra}: kl_free {free:.6g} (gap {gap:.3e}), closed {frac64:.3f} of the rows')
    assert 0.0 < frac64 < 1.0 and abs(float(got[1]['kl_free_frac']) - frac64) < 1e-6
    assert torch.equal(got[2]['loss_kl_clip'] > got[2]['loss_kl'], (ref[2]['loss_kl'] < free).to(DEV))
    _compare(model, got, ref, ('loss_kl', 'loss_kl_clip', 'loss_image', 'loss_reward'), ('loss_kl', 'loss_kl_clip', 'loss_reward'),
             f'free bits {extra}')
    assert got[2]['loss_kl_clip'].shape == (oconf.batch_length, oconf.batch_size)


def test_free_bits_tail_on_the_side_stream_is_bit_identical(hip):
    oconf = O.tiny_conf(batch_size=16)
    obs, noise = _batch(oconf)
    probe = _model(oconf)
    free = float(_step(probe, oconf, obs, noise)[2]['loss_kl'].median())
    runs = []
    for tail in (True, False):
        model = _model(oconf, kl_free=free)
        model.wm_tail_on_side = tail
        out = _step(model, oconf, obs, noise)
        assert (model.wm._last_pack.get('tail') is not None) == tail
        assert 0.0 < float(out[1]['kl_free_frac']) < 1.0
        runs.append(out)
    a, b = runs
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    assert a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    for k in ('loss_kl', 'loss_kl_clip', 'loss_reward', 'loss_image', 'entropy_post'):
        assert torch.equal(a[2][k], b[2][k]), k
    assert all(torch.equal(a[4][k], b[4][k]) for k in a[4])


def test_free_bits_refuse_iwae(hip):
    oconf = O.tiny_conf()
    obs, noise = _batch(O.tiny_conf(iwae_samples=2))
    model = _model(oconf, kl_free=1.0)
    with pytest.raises(NotImplementedError, match='kl_free'):
        model.training_step(_to_dev(obs), model.init_state(oconf.batch_size * 2), noise=_to_dev(noise), iwae_samples=2)
    with pytest.raises(NotImplementedError, match='kl_free'):
        _model(O.tiny_conf(iwae_samples=2), kl_free=1.0)


# ---------------------------------------------------------------------------------------------- the two-hot reward head
@pytest.mark.parametrize('K,I', [(7, 1), (255, 1), (7, 2)])
def test_reward_head_against_float64(hip, K, I):
    oconf = O.tiny_conf(iwae_samples=I)
    obs, noise = _batch(oconf, reward_scale=3.0)
    model = _model(oconf, reward_dist='twohot', reward_twohot_bins=K)
    assert model.wm.decoder.reward.model.out_dim == K
    got = _step(model, oconf, obs, noise)
    ref = _float64(model, oconf, obs, noise, I=I)
    _compare(model, got, ref, ('loss_reward', 'loss_kl', 'loss_image', 'loss_terminal'), ('loss_reward', 'reward_rec', 'loss_kl'),
             f'two-hot K={K} I={I}')
    head = [k for k in got[4] if k.startswith('decoder.reward.')]
    assert len(head) == 18 and all(float(got[4][k].abs().max()) > 0 for k in head)
    assert got[4]['decoder.reward.model.model.12.weight'].shape == (K, 400)


def test_predict_dream_and_planner_read_the_decoded_mean(hip):
    from pydreamer_amd.planner import CEMPlanner
    K, oconf = 255, O.tiny_conf()
    obs, noise = _batch(oconf)
    model = _model(oconf, reward_dist='twohot', reward_twohot_bins=K)
    dec = model.wm.decoder
    p = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    decode64 = lambda feats: TC.twohot_decode(O.mlp(p, HEAD, feats.double().cpu(), oconf.reward_decoder_layers), dec.reward.bins.double().cpu())
    T, B = oconf.batch_length, oconf.batch_size
    with torch.no_grad():
        _, _, metrics, tensors, dream_tensors = model.training_step(_to_dev(obs), model.init_state(B), noise=_to_dev(noise),
                                                                    do_image_pred=True, do_dream_tensors=True)
    for k in ('logprob_reward', 'reward_pred', 'logprob_reward-1', 'logprob_reward1'):
        assert tensors[k].shape == (T, B), k
    for k in ('logprob_reward', 'logprob_reward-1', 'logprob_reward1'):
        assert k in metrics and math.isfinite(float(metrics[k])), k
    assert bool(torch.isfinite(tensors['reward_pred']).all()) and float(tensors['logprob_reward'].min()) > 0
    sign = torch.sign(_to_dev(obs)['reward'])
    assert torch.equal(torch.isnan(tensors['logprob_reward1']), sign != 1) and torch.equal(torch.isnan(tensors['logprob_reward-1']), sign != -1)
    # the dream: the mean-only kernel over all imagined rows
    xh = model.last_extras
    feats = xh['dream_features']
    _close(xh['dream_reward'].reshape(-1), decode64(feats).reshape(-1), 'dream reward against float64')
    # ... exactly: the head's mean-only launch on the dream's own logit rows (all (H + 1) T B of them, filled window by window)
    logits = xh['dream_reward_out']
    assert logits.shape == (feats.shape[0] * feats.shape[1], K)
    assert torch.equal(xh['dream_reward'].reshape(-1), dec.reward.loss(logits)[2]), 'dream reward = the mean-only kernel on its logits'
    _close(logits, O.mlp(p, HEAD, feats.double().cpu(), oconf.reward_decoder_layers).reshape(-1, K), 'dream logits against float64 (row order)')
    log_logits = xh['dream_log_reward_out']
    assert dream_tensors['reward_pred'].shape == (T, B) and log_logits.shape == (T * B, K)
    assert torch.equal(dream_tensors['reward_pred'].reshape(-1), dec.reward.loss(log_logits)[2]), 'the log dream reads the same decoded mean'
    # the planner's reward read (Dreamer.inference reads no reward: it returns the action distribution, the state and policy_value,
    # so there is nothing of this head to compare there)
    obs1 = {k: v[:1] for k, v in _to_dev(obs).items()}
    u_post = torch.rand(1, B, oconf.stoch_dim, device=DEV)
    with torch.no_grad():
        features, _ = model.wm.forward(obs1, model.init_state(B), u_post)
    roll = CEMPlanner(model, horizon=3, candidates=8, elites=2, iters=2).plan(features.reshape(B, -1).contiguous(), keep_rollout=True)['rollout']
    _close(roll['reward'].reshape(-1), decode64(roll['features']).reshape(-1), 'planner reward against float64')


def test_a_fresh_head_predicts_zero_and_large_rewards_stay_of_order_log_k(hip):
    from pydreamer_amd.models import Dreamer
    oconf = O.tiny_conf()
    obs, noise = _batch(oconf, reward_scale=128.0)
    ws = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    for K in (7, 255, 256):
        torch.manual_seed(K)
        model = Dreamer(config.load_config('defaults', 'atari', **{**vars(oconf), **dict(reward_dist='twohot', reward_twohot_bins=K)})).to(DEV)
        head, F_ = model.wm.decoder.reward, model.wm.features_dim
        x = torch.randn(70, F_, device=DEV)
        mean = head.loss(head.model.fwd(x, F_, 70, ws, save_acts=False)[0])[2]
        print(f'K={K}: fresh head max |reward| {float(mean.abs().max()):.3e}')
        assert float(mean.abs().max()) < 1e-5
    # unsquashed rewards: |r| up to 128
    normal = float(_step(_model(oconf), oconf, obs, noise)[1]['loss_reward'])
    for K in (7, 255):
        twohot = float(_step(_model(oconf, reward_dist='twohot', reward_twohot_bins=K), oconf, obs, noise)[1]['loss_reward'])
        print(f'rewards x 128: loss_reward Normal {normal:.6g}, two-hot K={K} {twohot:.6g} (log K {math.log(K):.4g})')
        assert math.isfinite(twohot) and 0 < twohot < 2 * math.log(K) and normal > 0.05 * 128 ** 2


def _head_gradients_ok(model, losses):
    assert all(math.isfinite(float(x)) for x in losses)
    head = {k: v for k, v in model.wm.decoder.reward.named_parameters()}
    assert len(head) == 18
    for k, v in head.items():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0, k


@pytest.mark.parametrize('extra', [dict(aux_critic=True), dict(amp=True)], ids=['conv_aux_critic', 'amp'])
def test_both_switches_on_the_convolution_path(hip, extra):
    oconf = O.tiny_conf(**extra)
    obs, noise = _batch(oconf)
    model = _model(oconf, reward_dist='twohot', reward_twohot_bins=31, kl_free=1.0)
    losses, metrics, _, _, _ = _step(model, oconf, obs, noise)
    _head_gradients_ok(model, losses)
    assert 0.0 <= float(metrics['kl_free_frac']) <= 1.0 and float(metrics['loss_kl_clip']) >= 1.0 - 1e-6


@pytest.mark.parametrize('section,fixture', [('minigrid', 'tiny_minigrid'), ('vectorenv', 'tiny_vectorenv')], ids=['dense_image', 'imageless'])
def test_both_switches_on_the_dense_and_the_imageless_path(hip, section, fixture):
    from pydreamer_amd.models import Dreamer
    g = np.load(os.path.join(GOLD, fixture + '.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    K = 31
    torch.manual_seed(5)
    model = Dreamer(config.load_config('defaults', section, **{**vars(oconf), **extra, **dict(reward_dist='twohot', reward_twohot_bins=K, kl_free=1.0)}))
    w, b = WC.head_output_layer(K)
    with torch.no_grad():
        model.wm.decoder.reward.model.model[12].weight.copy_(w)
        model.wm.decoder.reward.model.model[12].bias.copy_(b)
    model = model.to(DEV)
    assert model.wm.dense == (section == 'minigrid') and model.wm.imageless == (section == 'vectorenv')
    if section == 'minigrid':
        from tests.test_gpu_minigrid import _obs
        obs, noise = _obs(g, 's0_', oconf, model)
    else:
        from tests.test_gpu_vectorenv import _fixture_obs
        obs, noise = _fixture_obs(g, 's0_', oconf)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    losses, _, metrics, tensors, _ = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise)
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    torch.cuda.synchronize()
    _head_gradients_ok(model, losses)
    assert tensors['loss_kl_clip'].shape == tensors['loss_kl'].shape and bool((tensors['loss_kl_clip'] >= 1.0).all())
    assert 0.0 <= float(metrics['kl_free_frac']) <= 1.0


def test_checkpoint_round_trip(hip, tmp_path):
    from pydreamer_amd.train import load_checkpoint, save_checkpoint
    oconf = O.tiny_conf()
    sw = dict(reward_dist='twohot', reward_twohot_bins=7, kl_free=1.0)
    obs, noise = _batch(oconf)
    model, fresh = _model(oconf, seed=0, **sw), _model(oconf, seed=1, **sw)
    for _ in range(2):
        _step(model, oconf, obs, noise)
        model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        for opt in model._opts:
            opt.step()
    path = str(tmp_path / 'latest.pt')
    save_checkpoint(path, model, model._opts, 2)
    assert torch.load(path, map_location='cpu')['model_state_dict'][f'{HEAD}.12.weight'].shape == (7, 400)
    fresh._opts = fresh.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    assert load_checkpoint(path, fresh, fresh._opts, map_location=DEV) == 2
    fresh.ac.train_steps = model.ac.train_steps      # (the step counter is the trainer's, not the checkpoint's)
    for k in (f'{HEAD}.12.weight', f'{HEAD}.12.bias'):
        assert torch.equal(fresh.state_dict()[k], model.state_dict()[k])
    a, b = _step(model, oconf, obs, noise), _step(fresh, oconf, obs, noise)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y), (float(x), float(y))
    assert torch.equal(a[1]['kl_free_frac'], b[1]['kl_free_frac'])


def test_the_trainer_logs_the_free_bits_scalars(hip, tmp_path):
    from pydreamer_amd import replay as R
    from pydreamer_amd.train import run
    from tests.test_gpu_train_loop import LoopEnv, _loop_conf
    conf = Namespace(**{**vars(_loop_conf()), **dict(kl_free=0.5, reward_dist='twohot', reward_twohot_bins=7, eval_interval=1000)})
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
        assert 0.0 <= m['train/kl_free_frac'] <= 1.0 and m['train/loss_kl_clip'] >= max(0.5, m['train/loss_kl']) - 1e-5
        assert np.isfinite(m['train/loss_reward']) and np.isfinite(m['train/loss_model'])
