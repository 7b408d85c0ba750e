"""-m gpu: the categorical reward decoder (reward_decoder_categorical).

  * dm_head_loss_catsup against the fp64 restatement of tests/test_reward_categorical_cpu.py (which that file pins to the
    reference's fixtures): rows {1, 7, 63, 65, 2500} x K {2, 3, 5, 17, 32} x ld {K, K + 3} x I {1, 2} - partial waves, row groups
    that straddle a wave, K that is no power of two (padded lanes in a row group), more than one block.  Logits hold rows at +-80
    and rows of all-equal values; targets hold every support value, exact midpoints, values beyond both ends; the support holds
    a duplicate.  `bin` EQUALS the fp32 CPU argmin.  loss and dlogits at the tolerance tests/test_gpu_map_probe.py applies to
    dm_cat_image_loss (the same log-softmax arithmetic) with cells = 1:  loss  _EPS (K + 17) (1 + |max| + |lse - max| + |x_t|),
    dlogits  |scale| (K + 8) _EPS.  mean_out = sum_k p_k sup_k has no counterpart there; from the same per-probability bound
    (K + 8) _EPS:  _EPS ((K + 8) sum_k |sup_k| + 7 max_k |sup_k|) - every p_k within (K + 8) _EPS, then one product and at most
    five butterfly additions (K <= 32) of terms whose magnitudes sum to at most max |sup|, plus the final rounding.
    The mean-only call gives the bits of the full call's mean_out, two runs give the same bits, scale = 0 gives dlogits == 0, and
    a NaN guard band around loss and dlogits (and the padding columns of the logits) is untouched.
  * every fixture of scripts/gen_reward_categorical_golden.py through Dreamer at the bars of tests/test_gpu_vectorenv.py:
    training steps (losses, metrics, tensors, gradient norms, the companion file's full gradients, parameter checksums after the
    optimizer steps; `_support` unchanged and without optimizer state), the logging variants with logprob_reward{i}
    (equal_nan: the never-hit bucket) and without logprob_reward-1, dream_tensors['reward_pred'] on the image fixture, amp.
  * the Normal head through the changed code: tiny_vectorenv's first step still matches its fixture.
  * save_checkpoint -> load_checkpoint round-trips `_support` and the optimizer state; train.run for six steps with one evaluate.
"""
import ast
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_form_params as CFP                     # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402
from tests.test_gpu_map_probe import _EPS, _close, _nan          # noqa: E402
from tests.test_reward_categorical_cpu import SUPPORT_KEY, bins_fp32, fixture_conf, fixture_params, restate      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
GUARD = 3      # NaN rows in front of and behind every output


# ------------------------------------------------------------------------------------------------ the kernel
def _support(K, seed):
    s = torch.sort(torch.randn(K, generator=torch.Generator().manual_seed(seed)) * 3).values.float()
    if K >= 3:
        s[K // 2] = s[K // 2 - 1]      # a duplicate: the lower index wins
    return s


def _case(rows, I, K, pad, seed):
    g = torch.Generator().manual_seed(seed)
    sup = _support(K, seed)
    x = torch.randn(rows, K, generator=g) * 3
    for r, v in ((0, 80.0), (2, -80.0)):
        if r < rows:
            x[r] = v + torch.randn(K, generator=g)
    if rows > 1:
        x[1] = 0.75                     # all-equal logits
    if rows > 3:
        x[3] = -80.0
        x[3, K - 1] = 80.0              # one class takes everything
    n = rows // I
    mids = (sup[:-1] + sup[1:]) * 0.5
    menu = torch.cat([sup, mids, sup[:1] - 1.5, sup[-1:] + 1.5, torch.tensor([0.0])])
    t = torch.cat([menu, menu[torch.randint(0, len(menu), (max(n - len(menu), 0),), generator=g)]])[:n]
    t = t[torch.randperm(n, generator=g)].float().contiguous()
    buf = torch.full((rows, K + pad), float('nan'))
    buf[:, :K] = x
    return buf.to(DEV), x, sup, t


def _call(hip, rows, I, K, buf, ld, sup_d, t_d, scale, full=True, mean=True):
    loss, dl, b = _nan(rows + 2 * GUARD), _nan(rows + 2 * GUARD, K), torch.full((rows // I + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
    mu = _nan(rows + 2 * GUARD)
    at = lambda t, w=1: None if t is None else hip.ptr(t[GUARD:])
    hip.call('dm_head_loss_catsup', rows, I, K, hip.fptr(buf), ld, hip.fptr(sup_d), hip.fptr(t_d) if full else None, scale,
             at(loss) if full else None, at(dl) if full else None, at(mu) if mean else None, at(b) if full else None, hip.stream())
    return loss, dl, mu, b


@pytest.mark.parametrize('I', [1, 2])
@pytest.mark.parametrize('pad', [0, 3])
@pytest.mark.parametrize('K', [2, 3, 5, 17, 32])
@pytest.mark.parametrize('rows', [1, 7, 63, 65, 2500])
def test_head_loss_catsup_against_fp64(hip, rows, K, pad, I):
    rows = (rows + I - 1) // I * I
    buf, x, sup, t = _case(rows, I, K, pad, seed=100 * rows + 10 * K + I)
    sup_d, t_d, ld, scale = sup.to(DEV), t.to(DEV), K + pad, 0.37
    loss, dl, mu, b = _call(hip, rows, I, K, buf, ld, sup_d, t_d, scale)
    loss2, dl2, mu2, b2 = _call(hip, rows, I, K, buf, ld, sup_d, t_d, scale)
    _, _, mu_only, _ = _call(hip, rows, I, K, buf, ld, sup_d, None, 0.0, full=False)
    _, dl0, _, _ = _call(hip, rows, I, K, buf, ld, sup_d, t_d, 0.0)
    loss_nm, _, mu_nm, _ = _call(hip, rows, I, K, buf, ld, sup_d, t_d, scale, mean=False)
    torch.cuda.synchronize()
    body = lambda v: v[GUARD:-GUARD]
    # the bin: exactly the reference's fp32 arithmetic on the CPU, midpoints and the duplicate included
    want_b = bins_fp32(t, sup)
    assert torch.equal(body(b).cpu().long(), want_b), 'bin differs from torch.square(t - sup).argmin(-1) in fp32'
    if K >= 3 and rows // I > K:
        assert K // 2 not in set(want_b.tolist()), 'the duplicated support value: its lower index wins every tie'
    ref_loss, p, ref_mean, _ = restate(x, sup, t, I)
    xd = x.double()
    mx, lse = xd.max(-1).values, torch.logsumexp(xd, -1)
    xt = xd.gather(-1, want_b.repeat_interleave(I)[:, None])[:, 0]
    what = f'rows={rows} K={K} ld+{pad} I={I}'
    _close(body(loss), ref_loss, _EPS * (K + 17) * (1 + mx.abs() + (lse - mx).abs() + xt.abs()), 'loss ' + what)
    onehot = F.one_hot(want_b.repeat_interleave(I), K).double()
    _close(body(dl), scale * (p - onehot), abs(scale) * (K + 8) * _EPS, 'dlogits ' + what)
    sa = sup.double().abs()
    _close(body(mu), ref_mean, _EPS * ((K + 8) * float(sa.sum()) + 7 * float(sa.max())), 'mean_out ' + what)
    # same bits: run to run, mean-only against the full form, with and without the optional outputs
    assert torch.equal(body(loss), body(loss2)) and torch.equal(body(dl), body(dl2)) and torch.equal(body(b), body(b2))
    assert torch.equal(body(mu), body(mu2)) and torch.equal(body(mu), body(mu_only)), 'mean-only form differs from the full form'
    assert torch.equal(body(loss), body(loss_nm)) and torch.isnan(mu_nm).all()
    assert bool((body(dl0) == 0).all()), 'scale = 0 leaves a non-zero dlogits'
    # guard bands and the padding columns
    for v in (loss, dl, mu, mu_only, dl0):
        assert torch.isnan(v[:GUARD]).all() and torch.isnan(v[-GUARD:]).all(), 'a guard band was written'
    assert bool((b[:GUARD] == -7).all()) and bool((b[-GUARD:] == -7).all())
    assert pad == 0 or torch.isnan(buf[:, K:]).all()


# ------------------------------------------------------------------------------------------------ the model against the fixtures
def _fixture_model(g, **more):
    from pydreamer_amd.models import Dreamer
    oconf, conf = fixture_conf(g, **more)
    model = Dreamer(conf)
    assert list(model.state_dict().keys()) == list(CFP.shapes_of_fixture(g).keys())
    model.load_state_dict(fixture_params(g), strict=True)
    return oconf, conf, model.to(DEV)


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-12)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _close_rt(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e}'


def _vec_obs(g, pre, oconf):
    action = F.one_hot(torch.from_numpy(g[pre + 'in_action_idx']), oconf.action_dim).float()
    obs = dict(action=action, reward=torch.from_numpy(g[pre + 'in_reward']), terminal=torch.from_numpy(g[pre + 'in_terminal']),
               reset=torch.from_numpy(g[pre + 'in_reset']), vecobs=torch.from_numpy(g[pre + 'in_vecobs']))
    noise = {k: torch.from_numpy(g[pre + 'in_' + k]).to(DEV) for k in ('u_post', 'u_act', 'u_prior', 'u_pred') if pre + 'in_' + k in g.files}
    return {k: v.to(DEV) for k, v in obs.items()}, noise


def _step(model, opts, oconf, obs, state, noise):
    losses, state, metrics, tensors, dream_tensors = model.training_step(obs, state, noise=noise)
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
    grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
    for opt in opts:
        opt.step()
    return losses, state, metrics, tensors, dream_tensors, gm, grads


def _check_train_step(g, full, pre, s, oconf, out, model):
    """The bars of tests/test_gpu_vectorenv.py test_training_steps_match_the_reference."""
    losses, state, metrics, tensors, dream_tensors, gm, grads = out
    assert dream_tensors == {}
    assert set({**metrics, **gm}) == {k[len(pre + 'metric_'):] for k in g.files if k.startswith(pre + 'metric_')}
    assert set(tensors.keys()) == {k[len(pre + 'tensor_'):] for k in g.files if k.startswith(pre + 'tensor_')}
    xh = model.last_extras
    assert np.array_equal(xh['post_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_post']), (s, 'posterior indices')
    assert np.array_equal(xh['act_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_act']), (s, 'action indices')
    for i, l in enumerate(losses):
        ref = g[pre + 'losses'][i]
        print(f'step {s} loss {i}: {float(l.detach()):.8g} reference {ref:.8g}')
        assert _rel(l, ref) < 2e-5 or abs(float(l) - ref) < 2e-6, (s, i, float(l), ref)
    assert abs(float(losses[0]) - g[pre + 'losses'][0]) < 1e-3
    for k, v in {**metrics, **gm}.items():
        ref = float(g[pre + 'metric_' + k])
        assert _rel(v, ref) < 1e-4 or abs(float(v) - ref) < 5e-6, (s, k, float(v), ref)
    for k in g.files:
        if k.startswith(pre + 'tensor_'):
            ref = torch.from_numpy(g[k])
            _close_rt(tensors[k[len(pre + 'tensor_'):]], ref, 1e-4, 1e-4 * max(1.0, float(ref.abs().max())), f'step {s} {k}')
    _close_rt(state[0], torch.from_numpy(g[pre + 'out_state_h']), 0, 1e-5 if s == 0 else 1e-4, f'step {s} out_state h')
    assert torch.equal(state[1].cpu(), torch.from_numpy(g[pre + 'out_state_z'])), f'step {s} out_state z'
    names = [str(n) for n in g[pre + 'grad_names']]
    assert SUPPORT_KEY not in names, 'the reference leaves _support without a gradient'
    assert names == [n for n in grads if n in set(names)]
    for n in grads:      # `_support` may hold a .grad here - a slice of the optimizer's flat buffer - but then it is zero
        assert n in names or (n == SUPPORT_KEY and not bool(grads[n].any())), n
    for n, ref in zip(names, g[pre + 'grad_norms']):
        got = float(grads[n].double().norm())
        assert abs(got - ref) <= 2e-3 * ref + 1e-7, (s, n, got, ref)
    n_full = 0
    for k in full:
        if k.startswith(pre + 'grad_') and k not in (pre + 'grad_norms', pre + 'grad_names'):
            n = k[len(pre + 'grad_'):]
            n_full += 1
            e = _rel_l2(grads[n], torch.from_numpy(full[k]))
            print(f'step {s} full gradient {n}: relative L2 error {e:.3e}')
            assert e < 2e-3, (s, n, e)
    sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
    np.testing.assert_allclose(sums, g[pre + 'param_abs_sums'], rtol=2e-6)
    return n_full


@pytest.mark.parametrize('name,steps,I', [('tiny_reward_categorical', 2, 1), ('tiny_reward_categorical_iwae', 1, 2)])
def test_training_steps_match_the_reference(hip, name, steps, I):
    from pydreamer_amd.models import DenseCategoricalSupportDecoder
    g = np.load(os.path.join(GOLD, name + '.npz'))
    oconf, conf, model = _fixture_model(g)
    assert oconf.iwae_samples == I and float(g['min_edge_distance']) > 1e-5
    assert isinstance(model.wm.decoder.reward, DenseCategoricalSupportDecoder)
    full = dict(g)
    if os.path.exists(os.path.join(GOLD, name + '_grads.npz')):
        full.update(np.load(os.path.join(GOLD, name + '_grads.npz')))
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    state = model.init_state(oconf.batch_size * I)
    for s in range(steps):
        pre = f's{s}_'
        obs, noise = _vec_obs(g, pre, oconf)
        out = _step(model, opts, oconf, obs, state, noise)
        state = out[1]
        n_full = _check_train_step(g, full, pre, s, oconf, out, model)
        assert n_full >= (2 if name == 'tiny_reward_categorical' and s == 0 else 0)
        assert np.array_equal(model.wm.decoder.reward._support.detach().cpu().numpy(), g['support']), 'the optimizer moved _support'
    # the optimizer state keeps the reference's parameter numbering: _support has an index and no state entry
    sd = opts[0].state_dict()
    wm = model.param_groups()['wm']
    i_sup = [i for i, p in enumerate(wm) if p is model.wm.decoder.reward._support]
    assert len(i_sup) == 1 and len(wm) == int(g['wm_param_count']) and sd['param_groups'][0]['params'] == list(range(len(wm)))
    assert i_sup[0] not in sd['state'] and len(sd['state']) == len(wm) - 1
    opts[0].load_state_dict(sd)
    sd2 = opts[0].state_dict()
    assert list(sd2['state']) == list(sd['state'])
    for i in sd['state']:
        assert torch.equal(sd['state'][i]['exp_avg'], sd2['state'][i]['exp_avg']) and torch.equal(sd['state'][i]['exp_avg_sq'], sd2['state'][i]['exp_avg_sq'])


def _check_logging(g, losses, st, metrics, tensors, skip_tensors=()):
    """The bars of tests/test_gpu_vectorenv.py test_logging_variants_match_the_reference."""
    K = len(g['support'])
    want_t = {f[7:] for f in g.files if f.startswith('tensor_')}
    assert set(tensors.keys()) - set(skip_tensors) == want_t and set(metrics) == {f[7:] for f in g.files if f.startswith('metric_')}
    assert {k for k in want_t if k.startswith('logprob_reward')} == {'logprob_reward'} | {f'logprob_reward{i}' for i in range(K)}
    assert 'logprob_reward-1' not in tensors and 'logprob_reward-1' not in metrics
    np.testing.assert_allclose(st[0].cpu().numpy(), g['out_state_h'], rtol=0, atol=5e-6)
    for i, l in enumerate(losses):
        assert _rel(l, g['losses'][i]) < 2e-5 or abs(float(l) - g['losses'][i]) < 2e-6, (i, float(l), g['losses'][i])
    n_nan = 0
    for k in metrics:
        ref = float(g['metric_' + k])
        if np.isnan(ref):
            n_nan += 1
            assert torch.isnan(metrics[k]), k
        else:
            assert _rel(metrics[k], ref) < 1e-4 or abs(float(metrics[k]) - ref) < 5e-6, (k, float(metrics[k]), ref)
    assert n_nan >= 1, 'the never-hit bucket'
    for k in want_t:
        np.testing.assert_allclose(tensors[k].cpu().numpy(), g['tensor_' + k], rtol=1e-4, atol=2e-5, equal_nan=True, err_msg=k)


@pytest.mark.parametrize('name', ['tiny_reward_categorical_eval', 'tiny_reward_categorical_open_loop'])
def test_logging_variants_match_the_reference(hip, name):
    g = np.load(os.path.join(GOLD, name + '.npz'))
    open_loop = bool(g['open_loop'])
    oconf, conf, model = _fixture_model(g)
    obs, noise = _vec_obs(g, '', oconf)
    with torch.no_grad():
        losses, st, metrics, tensors, dt = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise, do_image_pred=True,
                                                               do_dream_tensors=True, do_open_loop=open_loop)
    assert dt == {}
    T, B, S = oconf.batch_length, oconf.batch_size, oconf.stoch_dim
    xh = model.last_extras
    assert np.array_equal(xh['post_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_post'])
    assert np.array_equal(xh['pred_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_pred'])
    _check_logging(g, losses, st, metrics, tensors)


def test_image_fixture_and_the_log_dream(hip):
    """Section `defaults` alone at the oracle's tiny sizes: the convolution path, so the log dream runs and
    dream_tensors['reward_pred'] comes from the mean-only call.  The frames are the oracle's synthetic batch of the recorded seed."""
    g = np.load(os.path.join(GOLD, 'tiny_reward_categorical_image_eval.npz'))
    oconf, conf, model = _fixture_model(g)
    raw = O.synthetic_batch(oconf, seed=int(g['batch_seed']), first=True)
    raw['reward'] = g['in_reward']
    obs = {k: v.to(DEV) for k, v in O.preprocess(raw, oconf).items()}
    noise = {k: v.to(DEV) for k, v in O.make_noise(oconf, seed=int(g['noise_seed'])).items() if k.startswith('u_')}
    with torch.no_grad():
        losses, st, metrics, tensors, dt = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise, do_image_pred=True,
                                                               do_dream_tensors=True)
    T, B, S = oconf.batch_length, oconf.batch_size, oconf.stoch_dim
    assert np.array_equal(model.last_extras['post_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_post'])
    assert np.array_equal(model.last_extras['pred_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_pred'])
    _check_logging(g, losses, st, metrics, tensors, skip_tensors=('image_rec', 'image_pred'))
    want_d = [f[6:] for f in g.files if f.startswith('dream_')]
    assert 'reward_pred' in want_d and set(dt.keys()) - {'image_pred'} == set(want_d)
    for k in want_d:
        np.testing.assert_allclose(dt[k].cpu().numpy(), g['dream_' + k], rtol=1e-4, atol=2e-5, err_msg=k)


def test_amp_against_the_reference_autocast(hip):
    """As tests/test_gpu_vectorenv.py test_amp_against_the_reference_autocast: posterior indices teacher-forced to the reference's,
    loss_model within 1e-3 relative of the reference's bf16 value AND of its fp32 value, the component metrics within 2e-2."""
    g = np.load(os.path.join(GOLD, 'tiny_reward_categorical_amp.npz'))
    assert np.array_equal(g['fp32_idx_post'], g['bf16_idx_post'])
    oconf, conf, model = _fixture_model(g, amp=True)
    obs, noise = _vec_obs(g, '', oconf)
    fidx = torch.from_numpy(g['bf16_idx_post'].astype(np.int64)).to(DEV)
    with torch.no_grad():
        losses, _, metrics, _, _ = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise, forced_idx=fidx)
    ref_bf16, ref_fp32 = float(g['bf16_losses'][0]), float(g['fp32_losses'][0])
    print('loss_model: build amp', float(losses[0]), 'reference autocast', ref_bf16, 'reference fp32', ref_fp32)
    assert abs(float(losses[0]) - ref_bf16) < 1e-3 * ref_bf16
    assert abs(float(losses[0]) - ref_fp32) < 1e-3 * ref_fp32
    for k in ('loss_vecobs', 'loss_reward', 'loss_terminal', 'entropy_post'):
        print(k, float(metrics[k]), float(g['bf16_metric_' + k]))
        assert _rel(metrics[k], float(g['bf16_metric_' + k])) < 2e-2, k


def test_normal_head_still_matches_its_fixture(hip):
    """reward_decoder_categorical unset: tiny_vectorenv's first step through the changed tail, backward and dream, at that
    fixture's own bars (losses, gradient norms, parameter checksums)."""
    from pydreamer_amd import config
    from pydreamer_amd.models import DenseNormalDecoder, Dreamer
    g = np.load(os.path.join(GOLD, 'tiny_vectorenv.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    model = Dreamer(config.load_config('defaults', 'vectorenv', **{**vars(oconf), **extra}))
    assert isinstance(model.wm.decoder.reward, DenseNormalDecoder) and model.wm.decoder.reward_bins == 0
    model.load_state_dict(CFP.make_params(CFP.shapes_of_fixture(g), seed=0), strict=True)
    model = model.to(DEV)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs, noise = _vec_obs(g, 's0_', oconf)
    losses, state, metrics, tensors, _, gm, grads = _step(model, opts, oconf, obs, model.init_state(oconf.batch_size), noise)
    for i, l in enumerate(losses):
        ref = g['s0_losses'][i]
        assert _rel(l, ref) < 2e-5 or abs(float(l) - ref) < 2e-6, (i, float(l), ref)
    assert set(tensors.keys()) == {k[len('s0_tensor_'):] for k in g.files if k.startswith('s0_tensor_')}
    for n, ref in zip([str(n) for n in g['s0_grad_names']], g['s0_grad_norms']):
        assert abs(float(grads[n].double().norm()) - ref) <= 2e-3 * ref + 1e-7, n
    sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
    np.testing.assert_allclose(sums, g['s0_param_abs_sums'], rtol=2e-6)


@pytest.mark.parametrize('combo', ['conv_aux_gauss_cont', 'dense_minigrid_probe'])
def test_other_paths_take_a_training_step(hip, combo):
    """The paths no fixture covers with this head: the convolution stack with the auxiliary critic, Gaussian latents and a
    continuous actor, and the dense categorical image path with reward_input and the map probe.  No reference here - none of
    these paths reads the reward head's width; what is checked is that a full step runs, every loss and metric is finite, the
    K-wide head receives a gradient in every tensor, and `_support` neither moves nor gets one."""
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    torch.manual_seed(0)
    if combo == 'conv_aux_gauss_cont':
        oconf = O.make_conf(**{**vars(O.tiny_conf()), 'aux_critic': True, 'stoch_discrete': 0, 'actor_dist': 'tanh_normal'})
        conf = config.load_config('defaults', 'atari', **vars(oconf), reward_decoder_categorical=[-1, 0, 1])
        model = Dreamer(conf).to(DEV)
        obs = {k: v.to(DEV) for k, v in O.preprocess(O.synthetic_batch(oconf), oconf).items()}
        noise = None
    else:
        from tests import test_gpu_minigrid as MG
        g = np.load(os.path.join(GOLD, 'tiny_minigrid.npz'))
        oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
        extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
        conf = config.load_config('defaults', 'minigrid', **{**vars(oconf), **extra, 'reward_decoder_categorical': [-1, 0, 1]})
        model = Dreamer(conf).to(DEV)
        assert model.wm.dense and conf.reward_input
        obs, noise = MG._obs(g, 's0_', oconf, model)
    K = 3
    sup0 = model.wm.decoder.reward._support.detach().clone()
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    losses, state, metrics, tensors, _, gm, grads = _step(model, opts, conf, obs, model.init_state(conf.batch_size), noise)
    vals = {k: float(v) for k, v in {**metrics, **gm}.items()}
    assert all(np.isfinite(float(l)) for l in losses) and all(np.isfinite(v) for v in vals.values()), vals
    assert 0 < vals['loss_reward'] < 10 and tuple(tensors['reward_rec'].shape) == (conf.batch_length, conf.batch_size)
    head = [n for n in grads if n.startswith('wm.decoder.reward.model.')]
    assert head and tuple(grads[head[-2]].shape) == (K, 400)
    for n in head:
        assert bool(torch.isfinite(grads[n]).all()) and float(grads[n].abs().sum()) > 0, n
    assert not bool(grads.get(SUPPORT_KEY, torch.zeros(1)).any())
    assert torch.equal(model.wm.decoder.reward._support.detach(), sup0)
    lo, hi = float(sup0.min()) - 1e-6, float(sup0.max()) + 1e-6      # (the probabilities sum to 1 up to rounding)
    assert bool(((tensors['reward_rec'] >= lo) & (tensors['reward_rec'] <= hi)).all()), 'a mean outside the support hull'


# ------------------------------------------------------------------------------------------------ checkpoint and trainer
def test_checkpoint_round_trips_support_and_optimizer_state(hip, tmp_path):
    from pydreamer_amd.models import Dreamer
    from pydreamer_amd.train import load_checkpoint, save_checkpoint
    g = np.load(os.path.join(GOLD, 'tiny_reward_categorical.npz'))
    oconf, conf, model = _fixture_model(g)
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    obs, noise = _vec_obs(g, 's0_', oconf)
    _step(model, opts, oconf, obs, model.init_state(oconf.batch_size), noise)
    path = str(tmp_path / 'latest.pt')
    save_checkpoint(path, model, opts, 1)
    ck = torch.load(path, map_location='cpu')
    # the saved state dict loads into the reference's name list, strictly: same names, same order, same shapes
    want = CFP.shapes_of_fixture(g)
    assert [(k, tuple(v.shape)) for k, v in ck['model_state_dict'].items()] == list(want.items())
    assert np.array_equal(ck['model_state_dict'][SUPPORT_KEY].numpy(), g['support'])
    conf2 = fixture_conf(g, reward_decoder_categorical=[-3, -2, 1, 4])[1]      # another support: the checkpoint's must replace it
    fresh = Dreamer(conf2).to(DEV)
    fopts = fresh.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    assert load_checkpoint(path, fresh, fopts, map_location=DEV) == 1
    assert np.array_equal(fresh.wm.decoder.reward._support.detach().cpu().numpy(), g['support'])
    a, b = model.state_dict(), fresh.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    for o1, o2 in zip(opts, fopts):
        s1, s2 = o1.state_dict(), o2.state_dict()
        assert list(s1['state']) == list(s2['state']) and s1['param_groups'][0]['params'] == s2['param_groups'][0]['params']
        for i in s1['state']:
            for k in ('exp_avg', 'exp_avg_sq', 'step'):
                assert torch.equal(s1['state'][i][k].cpu(), s2['state'][i][k].cpu()), (i, k)


def test_trainer_runs_and_evaluate_logs_the_buckets(hip, tmp_path, monkeypatch):
    """train.run for six steps on the scripted environment of tests/test_gpu_train_loop.py with the categorical head: the loss
    is finite in both log windows and the evaluation at step 6 logs the per-bucket metrics through its dynamic slots."""
    import math
    from argparse import Namespace
    from tests import test_gpu_train_loop as TL
    base = TL._loop_conf()
    monkeypatch.setattr(TL, '_loop_conf', lambda: Namespace(**{**vars(base), 'reward_decoder_categorical': [-2, -0.5, 0, 1]}))
    conf, logdir, logged = TL._run(tmp_path, None)
    train = [m for s, m in logged if 'train/steps' in m]
    assert len(train) == 2 and all(math.isfinite(m['train/loss_reward']) for m in train)
    keys = {k for _, m in logged for k in m}
    assert 'test/logprob_reward0' in keys and 'test/logprob_reward' in keys, sorted(k for k in keys if k.startswith('test/'))
    assert not [k for k in keys if 'logprob_reward-1' in k]
    ck = torch.load(os.path.join(logdir, 'checkpoints', 'latest.pt'), map_location='cpu')
    assert ck['model_state_dict'][SUPPORT_KEY].tolist() == [-2.0, -0.5, 0.0, 1.0]
