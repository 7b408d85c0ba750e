"""-m gpu: the observation inputs beyond the image.

reward_input - the reward and terminal planes of encoders.py:52-59 folded into the encoder's first convolution
(csrc/conv_direct.hip: per-frame bias table forward, frame-weighted column sum backward); vecobs_size > 0 - the MLP
encoder whose output sits behind the image embedding and the DenseNormalDecoder with out_dim = V (dm_head_loss_normal_nd).

  * tests/golden/tiny_reward_input.npz, tiny_vecobs.npz (+ _grads) and tiny_obs_combo.npz (both keys, iwae_samples = 2), written by
    the real reference (scripts/gen_obs_golden.py), replayed through Dreamer.training_step -> four backward passes -> grad_clip ->
    AdamW for two steps with carried state.  Bars: those tests/test_gpu_training_step.py applies to tiny.npz
    (_check_reference_golden: indices equal, losses 2e-5 relative or 2e-6, loss_model 1e-3 absolute, metrics 1e-4 relative or
    5e-6, gradient norms 2e-3 relative, parameter checksums 2e-6 relative) and, for what that function does not look at, the bars
    of the same module's oracle comparison (_check_pair: logged tensors 1e-4 relative + 1e-4 * max(1, max|ref|), full gradients
    2e-3 relative L2, out_state h 1e-5 on equal parameters; from step 1 on 1e-4, derived at the assertion).
  * tiny_obs_inference.npz (Dreamer.inference reads obs['reward'], obs['terminal'], obs['vecobs']), tiny_obs_amp.npz (the reference
    under autocast), tiny_obs_eval.npz / tiny_obs_open_loop.npz (do_image_pred + do_dream_tensors under no_grad), all with both keys
    on, at the bars of the existing inference / amp / logging golden tests.
  * uint8 = float frames, and overlap_backward / wm_tail_on_side on = off, bit for bit, on tiny_reward_input and tiny_obs_combo.
  * the GRU cells, aux_critic, iwae_samples = 2, probe_gradients, Gaussian latents, NoNorm with reward_input: on a batch whose
    reward and terminal are zero, against the plain model with the same weights, bit for bit.
  * kernel level, in the style of tests/test_gpu_conv_stack.py: dm_conv_encoder_fwd_planes / _bwd_planes at 2 500 frames x depth 48
    and 1 536 frames x depth 32, uint8 and float frames, EVERY element of the layer-1 output, of embed and of all dW / db against
    torch conv2d in fp64 over the explicitly built 5-channel image, computed on the device.  Metric and bar are that module's
    (oracle/conv_reference.py check_tensor): err = max_i |got_i - ref64_i| / rms(ref64) <= max(10 * err_ref32, 64 * eps_fp32) with
    err_ref32 from the same torch functions in fp32.  The two plane slices of dW0 are constant over their 16 taps, bit for bit.
  * dm_head_loss_normal_nd against torch.distributions in fp64 at rows {15, 2500, 40000} x V {4, 27}, at the bounds the existing
    head losses are held to (tests/test_gpu_primitives.py test_head_loss: loss and mean 1e-5 relative + 1e-6, dout 1e-5 + 1e-9).
  * models built from the `miniworld` and `minecraft` sections run two steps at the sections' native shapes with finite losses.
"""
import ast
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_form_params as CFP                     # noqa: E402
from oracle import conv_reference as R               # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
ENC0 = 'wm.encoder.encoder_image.model.0'


def _hip_conf(oconf, **extra):
    from pydreamer_amd import config
    return config.load_config('defaults', 'atari', **{**vars(oconf), **extra})


def _build(conf, seed=0, shapes=None):
    """Model with the closed-form weights of its own (or the fixture's) state_dict table."""
    from pydreamer_amd.models import Dreamer
    model = Dreamer(conf)
    sd = model.state_dict()
    if shapes is None:
        shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert list(sd.keys()) == list(shapes.keys())
    model.load_state_dict(CFP.make_params(shapes, seed=seed), strict=True)
    return model.to(DEV)


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-12)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _close(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})'


def _fixture_obs(g, pre, oconf, u8=False):
    raw = {k: g[pre + 'in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
    obs = {k: v.to(DEV) for k, v in O.preprocess(raw, oconf).items()}
    if u8:
        obs['image'] = torch.from_numpy(raw['image_u8']).to(DEV)
    if pre + 'in_vecobs' in g.files:
        obs['vecobs'] = torch.from_numpy(g[pre + 'in_vecobs']).to(DEV)
    noise = {k: torch.from_numpy(g[pre + 'in_' + k]).to(DEV) for k in ('u_post', 'u_act', 'u_prior')}
    return obs, noise


# ------------------------------------------------------------------------------------------------ the reference's fixture
TRAIN_FIXTURES = {'tiny_reward_input': dict(reward_input=True, vecobs_size=0), 'tiny_vecobs': dict(reward_input=False, vecobs_size=27),
                  'tiny_obs_combo': dict(reward_input=True, vecobs_size=27)}


@pytest.mark.parametrize('name', list(TRAIN_FIXTURES))
def test_training_steps_match_the_reference(hip, name):
    g = np.load(os.path.join(GOLD, name + '.npz'))
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    assert extra == TRAIN_FIXTURES[name] and oconf.iwae_samples == (2 if name == 'tiny_obs_combo' else 1)
    assert float(g['min_edge_distance']) > 1e-5
    assert any(float(g[f's{s}_in_terminal'].max()) == 1.0 for s in range(2)), 'the terminal plane never carries a value'
    full = dict(g)
    if os.path.exists(os.path.join(GOLD, name + '_grads.npz')):
        full.update(np.load(os.path.join(GOLD, name + '_grads.npz')))
    model = _build(_hip_conf(oconf, **extra), shapes=CFP.shapes_of_fixture(g))
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    state = model.init_state(oconf.batch_size * oconf.iwae_samples)
    T, B, S, Hh = oconf.batch_length, oconf.batch_size, oconf.stoch_dim, oconf.imag_horizon
    for s in range(2):
        pre = f's{s}_'
        obs, noise = _fixture_obs(g, pre, oconf)
        losses, state, metrics, tensors, _ = model.training_step(obs, state, noise=noise)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        named = dict(model.named_parameters())
        grads = {k: v.grad.detach().clone() for k, v in named.items() if v.grad is not None}
        for opt in opts:
            opt.step()
        xh = model.last_extras
        assert np.array_equal(xh['post_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_post']), (s, 'posterior indices')
        assert np.array_equal(xh['act_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_act']), (s, 'action indices')
        lat = xh['dream_features'][1:, :, oconf.deter_dim:].reshape(Hh, -1, S, oconf.stoch_discrete).argmax(-1)
        assert np.array_equal(lat.cpu().numpy().astype(np.uint8), g[pre + 'idx_lat']), (s, 'imagined latent indices')
        for i, l in enumerate(losses):
            ref = g[pre + 'losses'][i]
            print(f'step {s} loss {i}: {float(l.detach()):.8g} reference {ref:.8g}')
            assert _rel(l, ref) < 2e-5 or abs(float(l) - ref) < 2e-6, (s, i, float(l), ref)
        assert abs(float(losses[0]) - g[pre + 'losses'][0]) < 1e-3
        for k, v in {**metrics, **gm}.items():
            ref = float(g[pre + 'metric_' + k])
            assert _rel(v, ref) < 1e-4 or abs(float(v) - ref) < 5e-6, (s, k, float(v), ref)
        for k in g.files:
            if k.startswith(pre + 'tensor_') and not k.startswith(pre + 'tensor_image_rec'):
                ref = torch.from_numpy(g[k])
                _close(tensors[k[len(pre + 'tensor_'):]], ref, 1e-4, 1e-4 * max(1.0, float(ref.abs().max())), f'step {s} {k}')
        rec = tensors['image_rec']
        ref = torch.from_numpy(g[pre + 'tensor_image_rec_frames'])
        _close(rec[:1, :1], ref, 1e-4, 1e-4 * max(1.0, float(ref.abs().max())), f'step {s} image_rec')
        # out_state h: 1e-5 while both sides hold the same parameters (step 0).  After an optimizer step the suite's own bar lets
        # every parameter differ by 1e-5 (AdamW's m / (sqrt(v) + eps) amplifies rounding where a gradient is near zero); a GRU
        # pre-activation sums hidden_dim + deter_dim = 128 products of such weights with inputs of magnitude <= 1, so h may
        # differ by sqrt(128) * 1e-5 = 1.1e-4 without anything being wrong: 1e-4 from step 1 on
        _close(state[0], torch.from_numpy(g[pre + 'out_state_h']), 0, 1e-5 if s == 0 else 1e-4, f'step {s} out_state h')
        assert torch.equal(state[1].cpu(), torch.from_numpy(g[pre + 'out_state_z'])), f'step {s} out_state z'
        names = [str(n) for n in g[pre + 'grad_names']]
        assert names == list(grads.keys())
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
        assert n_full >= (3 if s == 0 else 0)
        dW = grads[ENC0 + '.weight']
        for c in ((3, 4) if extra['reward_input'] else ()):        # the reference's plane gradients do not vary over the taps at all; neither may these
            plane = dW[:, c].reshape(dW.shape[0], 16)
            assert torch.equal(plane, plane[:, :1].expand_as(plane)), f'step {s}: dW[:, {c}] varies over its taps'
            assert float(plane.abs().max()) > 0
        sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
        np.testing.assert_allclose(sums, g[pre + 'param_abs_sums'], rtol=2e-6)


def _two_steps(model, g, oconf, u8=False):
    """Two trainer iterations on the fixture's inputs; everything a variant must reproduce bit for bit."""
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    st = model.init_state(oconf.batch_size * oconf.iwae_samples)
    hist = []
    for s in range(2):
        obs, noise = _fixture_obs(g, f's{s}_', oconf, u8=u8)
        losses, st2, metrics, tensors, _ = model.training_step(obs, st, noise=noise)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        grads = torch.cat([o.flat_grad for o in opts]).clone()
        for opt in opts:
            opt.step()
        st = tuple(x.clone() for x in st2)
        hist.append(([float(x) for x in losses], {k: float(v) for k, v in metrics.items()},
                     {k: v.detach().float().cpu() for k, v in tensors.items()}, grads.cpu(),
                     torch.cat([o.flat_param for o in opts]).cpu()))
    return hist


def _assert_same_runs(a_hist, b_hist, what):
    for s, (a, b) in enumerate(zip(a_hist, b_hist)):
        assert a[0] == b[0], (what, s, a[0], b[0])
        assert a[1] == b[1], (what, s, {k: (a[1][k], b[1][k]) for k in a[1] if a[1][k] != b[1][k]})
        assert a[2].keys() == b[2].keys()
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), f'{what}: step {s}: tensor {k} differs'
        assert torch.equal(a[3], b[3]), f'{what}: step {s}: gradients differ'
        assert torch.equal(a[4], b[4]), f'{what}: step {s}: parameters differ'
    assert float(a_hist[0][3].abs().sum()) > 0


def _fixture_model(g, **more):
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    return oconf, _build(_hip_conf(oconf, **extra, **more), shapes=CFP.shapes_of_fixture(g))


@pytest.mark.parametrize('name', ['tiny_reward_input', 'tiny_obs_combo'])
def test_uint8_and_float_frames_are_bit_identical(hip, name):
    g = np.load(os.path.join(GOLD, name + '.npz'))
    runs = []
    for u8 in (False, True):
        oconf, model = _fixture_model(g)
        runs.append(_two_steps(model, g, oconf, u8=u8))
    _assert_same_runs(runs[0], runs[1], 'uint8 against float frames')


@pytest.mark.parametrize('name', ['tiny_reward_input', 'tiny_obs_combo'])
@pytest.mark.parametrize('switch', ['overlap_backward', 'wm_tail_on_side'])
def test_backward_placement_is_bit_identical(hip, switch, name):
    """The encoder backward with the planes and the backward of the two vecobs MLPs join the pre-launched world-model backward:
    same results whether that pass runs on its side stream or inside backward(), and whether the forward's tail (with the
    vecobs head and its loss) runs on the side stream or on the caller's."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    runs = []
    for on in (True, False):
        oconf, model = _fixture_model(g)
        assert model.overlap_backward and model.wm_tail_on_side
        setattr(model, switch, on)
        runs.append(_two_steps(model, g, oconf))
        if switch == 'wm_tail_on_side':
            assert (model.wm._last_pack.get('tail') is not None) == on
    _assert_same_runs(runs[0], runs[1], switch)


def test_inference_matches_the_reference(hip):
    """Dreamer.inference reads obs['reward'], obs['terminal'] (reward_input) and obs['vecobs'] (dreamer.py:102); bars of
    test_inference_matches_reference_golden: action probabilities 1e-4 relative + 2e-6, state and policy_value 2e-6."""
    g = np.load(os.path.join(GOLD, 'tiny_obs_inference.npz'))
    oconf, model = _fixture_model(g)
    u8 = torch.from_numpy(g['in_image_u8'])
    obs = dict(image=(u8.float() / 255.0 - 0.5).permute(0, 1, 4, 2, 3).contiguous().to(DEV), action=torch.from_numpy(g['in_action']).to(DEV),
               reset=torch.from_numpy(g['in_reset']).to(DEV), reward=torch.from_numpy(g['in_reward']).to(DEV),
               terminal=torch.from_numpy(g['in_terminal']).to(DEV), vecobs=torch.from_numpy(g['in_vecobs']).to(DEV))
    assert float(obs['terminal'].sum()) == 1.0 and float(obs['reward'].abs().min()) > 0
    state = (torch.from_numpy(g['in_h']).to(DEV), torch.from_numpy(g['in_z']).to(DEV))
    with torch.no_grad():
        dist, (h1, z1), metrics = model.inference(obs, state, noise=dict(u_post=torch.from_numpy(g['in_u']).to(DEV)))
        _close(dist.probs, torch.from_numpy(g['action_probs']), 1e-4, 2e-6, 'action probabilities')
        _close(h1, torch.from_numpy(g['out_h']), 0, 2e-6, 'out_state h')
        assert torch.equal(z1.cpu(), torch.from_numpy(g['out_z']))
        assert abs(float(metrics['policy_value']) - float(g['policy_value'])) < 2e-6
        for gone in ('terminal', 'vecobs'):      # inputs of the encoder now: leaving one out is an error, not a silent zero
            with pytest.raises(ValueError):
                model.inference({k: v for k, v in obs.items() if k != gone}, state)


def test_amp_against_the_reference_autocast(hip):
    """tests/golden/tiny_obs_amp.npz (both keys on), produced the way tiny_amp.npz is; the bars of
    test_amp_against_reference_autocast_golden: posterior indices teacher-forced to the reference's, loss_model within 1e-3
    relative of the reference's bf16 value AND of its fp32 value, the component metrics within 2e-2."""
    from pydreamer_amd import config
    g = np.load(os.path.join(GOLD, 'tiny_obs_amp.npz'))
    oconf, model = _fixture_model(g, amp=True)
    obs, noise = _fixture_obs(g, '', oconf)
    fidx = torch.from_numpy(g['bf16_idx_post'].astype(np.int64)).to(DEV)
    with torch.no_grad():
        losses, _, metrics, _, _ = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise, forced_idx=fidx)
    ref_bf16, ref_fp32 = float(g['bf16_losses'][0]), float(g['fp32_losses'][0])
    print('loss_model: build amp', float(losses[0]), 'reference autocast', ref_bf16, 'reference fp32', ref_fp32)
    assert abs(float(losses[0]) - ref_bf16) < 1e-3 * ref_bf16
    assert abs(float(losses[0]) - ref_fp32) < 1e-3 * ref_fp32
    for k in ('loss_image', 'loss_reward', 'loss_terminal', 'entropy_post'):
        assert _rel(metrics[k], float(g['bf16_metric_' + k])) < 2e-2, k
    print('loss_vecobs: build amp', float(metrics['loss_vecobs']), 'reference autocast', float(g['bf16_metric_loss_vecobs']))


@pytest.mark.parametrize('name', ['tiny_obs_eval', 'tiny_obs_open_loop'])
def test_logging_variants_match_the_reference(hip, name):
    """do_image_pred + do_dream_tensors, closed loop and with do_open_loop, under no_grad (train.py:353-359,380-385); the bars of
    test_logging_variants_match_reference_golden / test_open_loop_matches_reference_golden."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    open_loop = bool(g['open_loop'])
    oconf, model = _fixture_model(g)
    obs, _ = _fixture_obs(g, '', oconf)
    noise = {k[3:]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith('in_u_')}
    assert 'tensor_logprob_vecobs' in g.files and 'tensor_vecobs_pred' in g.files and 'metric_logprob_vecobs' in g.files
    with torch.no_grad():
        losses, st, metrics, tensors, dt = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise, do_image_pred=True,
                                                               do_dream_tensors=True, do_open_loop=open_loop)
    T, B, S = oconf.batch_length, oconf.batch_size, oconf.stoch_dim
    xh = model.last_extras
    assert np.array_equal(xh['post_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_post'])
    assert np.array_equal(xh['pred_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_pred'])
    assert np.array_equal(xh['dream_log_act_idx'].cpu().numpy().astype(np.uint8), g['idx_log_act'])
    np.testing.assert_allclose(st[0].cpu().numpy(), g['out_state_h'], rtol=0, atol=5e-6)
    for i, l in enumerate(losses):
        assert _rel(l, g['losses'][i]) < 2e-5 or abs(float(l) - g['losses'][i]) < 2e-6, (i, float(l), g['losses'][i])
    for k in [f[7:] for f in g.files if f.startswith('metric_')]:
        ref = float(g['metric_' + k])
        if np.isnan(ref):
            assert torch.isnan(metrics[k]), k
        else:
            assert _rel(metrics[k], ref) < 1e-4 or abs(float(metrics[k]) - ref) < 5e-6, (k, float(metrics[k]), ref)
    for k in [f[7:] for f in g.files if f.startswith('tensor_') and not f.endswith(('_sum', '_frame'))]:
        np.testing.assert_allclose(tensors[k].cpu().numpy(), g['tensor_' + k], rtol=1e-4, atol=2e-5, equal_nan=True, err_msg=k)
    assert _rel(tensors['image_pred'].double().sum(), g['tensor_image_pred_sum']) < 1e-5
    np.testing.assert_allclose(tensors['image_pred'][:1, :1].cpu().numpy(), g['tensor_image_pred_frame'], rtol=0, atol=3e-5)
    for k in [f[6:] for f in g.files if f.startswith('dream_') and not f.startswith('dream_image_pred')]:
        np.testing.assert_allclose(dt[k].cpu().numpy(), g['dream_' + k], rtol=1e-4, atol=2e-5, err_msg=k)
    assert _rel(dt['image_pred'].double().sum(), g['dream_image_pred_sum']) < 1e-5
    np.testing.assert_allclose(dt['image_pred'][-1:, :1].cpu().numpy(), g['dream_image_pred_frame'], rtol=0, atol=3e-5)


VARIANTS = [dict(gru_type='gru_layernorm'), dict(gru_type='gru_layernorm_dv2', gru_layers=2), dict(aux_critic=True),
            dict(iwae_samples=2), dict(probe_gradients=True), dict(stoch_discrete=0), dict(layer_norm=False)]


@pytest.mark.parametrize('kw', VARIANTS, ids=lambda kw: ','.join(f'{k}={v}' for k, v in kw.items()))
def test_reward_input_with_zero_planes_is_the_plain_encoder(hip, kw):
    """The other structural variants with the new input, checked without a reference: with reward = terminal = 0 in the batch the
    bias table IS the bias (fma(0, s, b) = b), so a reward_input model and a plain model holding the same weights (the 5-channel
    weight's image channels) run the same arithmetic: equal losses, metrics and gradients bit for bit, except the layer-0 bias
    gradient, which the two paths sum in different orders (held to the suite's gradient bar, 2e-3 relative L2), and the plane
    gradients are exactly zero."""
    oconf = O.tiny_conf(**kw)
    I = oconf.iwae_samples
    a = _build(_hip_conf(oconf, reward_input=True))
    from pydreamer_amd.models import Dreamer
    b = Dreamer(_hip_conf(oconf))
    sd = {k: v.detach().clone() for k, v in a.state_dict().items()}
    sd[ENC0 + '.weight'] = sd[ENC0 + '.weight'][:, :3].contiguous()
    b.load_state_dict(sd, strict=True)
    b = b.to(DEV)
    raw = O.synthetic_batch(oconf, seed=21, first=True)
    raw['reward'][:] = 0
    raw['terminal'][:] = 0
    obs = {k: v.to(DEV) for k, v in O.preprocess(raw, oconf).items()}
    out = []
    for model in (a, b):
        torch.manual_seed(5)                   # the samplers' draws come from torch's generator: the same in both runs
        losses, _, metrics, _, _ = model.training_step(obs, model.init_state(oconf.batch_size * I))
        for loss in losses:
            loss.backward()
        torch.cuda.synchronize()
        out.append(([float(x) for x in losses], {k: float(v) for k, v in metrics.items()},
                    {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}))
    (la, ma, ga), (lb, mb, gb) = out
    assert la == lb and ma == mb, (la, lb)
    assert all(np.isfinite(x) for x in la)
    assert ga.keys() == gb.keys()
    for k in ga:
        if k == ENC0 + '.weight':
            assert torch.equal(ga[k][:, :3], gb[k]), k
            assert not bool(ga[k][:, 3:].any()), 'plane gradients with zero planes'
        elif k == ENC0 + '.bias':
            assert _rel_l2(ga[k], gb[k]) < 2e-3, k
        else:
            assert torch.equal(ga[k], gb[k]), k


# ------------------------------------------------------------------------------------------------ kernel level
def _planes_reference(params, raw, reward, terminal, dembed, dtype, chunk=100):
    """torch conv2d over the explicitly built 5-channel image (encoders.py:52-59,80-96), on the device of its arguments.
    Returns y0 (N, 31, 31, d) - the post-ELU output of layer 1, NHWC - embed (N, 32 d) and dW / db of the four layers for the
    loss sum(embed * dembed)."""
    ws = [params[f'wm.encoder.encoder_image.model.{2 * i}.weight'].to(dtype).clone().requires_grad_(True) for i in range(4)]
    bs = [params[f'wm.encoder.encoder_image.model.{2 * i}.bias'].to(dtype).clone().requires_grad_(True) for i in range(4)]
    acc = [torch.zeros_like(p) for p in ws + bs]
    y0s, embeds = [], []
    N = raw.shape[0]
    for s in range(0, N, chunk):
        x = R.to_frames(raw[s:s + chunk], dtype).to(reward.device)      # x / 255 - 0.5 on the host, as the float path's frames
        n = x.shape[0]
        planes = torch.stack([reward[s:s + n].to(dtype), terminal[s:s + n].to(dtype)], 1)[:, :, None, None].expand(n, 2, 64, 64)
        x = torch.cat([x, planes], 1)
        y0 = F.elu(F.conv2d(x, ws[0], bs[0], stride=2))
        y = y0
        for i in range(1, 4):
            y = F.elu(F.conv2d(y, ws[i], bs[i], stride=2))
        embed = y.flatten(1)
        grads = torch.autograd.grad(embed, ws + bs, dembed[s:s + n].to(dtype))
        for a, gr in zip(acc, grads):
            a += gr
        y0s.append(y0.detach().permute(0, 2, 3, 1).contiguous())
        embeds.append(embed.detach())
    out = {'y0': torch.cat(y0s).cpu(), 'embed': torch.cat(embeds).cpu()}
    for i in range(4):
        out[f'dW{i}'], out[f'db{i}'] = acc[i].cpu(), acc[4 + i].cpu()
    return out


PLANE_CASES = [(2500, 48), (1536, 32)]


@pytest.mark.parametrize('frames,depth', PLANE_CASES, ids=[f'n{n}-d{d}' for n, d in PLANE_CASES])
def test_reward_input_encoder_every_element(hip, frames, depth):
    H = hip
    oconf = O.tiny_conf(cnn_depth=depth)
    model = _build(_hip_conf(oconf, reward_input=True))
    enc = model.wm.encoder.encoder_image
    E = enc.out_dim
    gen = torch.Generator().manual_seed(11 * 1000003 + frames)
    raw = torch.randint(0, 256, (frames, 64, 64, 3), generator=gen, dtype=torch.uint8)
    dembed = torch.randn(frames, E, generator=gen).to(DEV)
    reward = torch.tanh(torch.randn(frames, generator=gen)).to(DEV)
    terminal = (torch.rand(frames, generator=gen) < 0.1).float().to(DEV)
    assert 0 < float(terminal.sum()) < frames
    params = {k: v.detach() for k, v in model.state_dict().items()}
    ref64 = _planes_reference(params, raw, reward, terminal, dembed, torch.float64)
    ref32 = _planes_reference(params, raw, reward, terminal, dembed, torch.float32)
    # the float path's frames: the host's x / 255 - 0.5 (a device division by a constant is a multiplication by its reciprocal)
    image_f = (raw.float() / 255.0 - 0.5).permute(0, 3, 1, 2).contiguous().to(DEV)
    raw_dev = raw.to(DEV)
    outs = {}
    for u8 in (False, True):
        shp = model.wm.shape(1, frames, 1)
        if u8:
            shp.flags |= H.DM_FLAG_IMAGE_U8
        nbytes = H.workspace_bytes(shp)
        nan = float('nan')
        ws = torch.full((nbytes // 4,), nan, device=DEV)
        acts = torch.full((int(H.lib().dm_conv_encoder_acts_floats(ctypes.byref(shp))),), nan, device=DEV)
        ld = E + 256          # the embedding as the leading columns of a wider buffer; the columns behind it stay untouched
        embed = torch.full((frames, ld), nan, device=DEV)
        dembed_w = torch.full((frames, ld), nan, device=DEV)
        dembed_w[:, :E] = dembed
        gw = [torch.full_like(m.weight, nan) for m in enc.convs()]
        gb = [torch.full_like(m.bias, nan) for m in enc.convs()]
        image = raw_dev if u8 else image_f
        enc_p = H.conv_struct([m.weight for m in enc.convs()], [m.bias for m in enc.convs()])
        enc_g = H.conv_struct(gw, gb, cls=H.dm_conv_grads)
        H.call('dm_conv_encoder_fwd_planes', ctypes.byref(shp), H.ptr(image), ctypes.byref(enc_p), H.fptr(reward), H.fptr(terminal),
               H.fptr(acts), H.fptr(embed), ld, H.ptr(ws), nbytes, H.stream())
        H.call('dm_conv_encoder_bwd_planes', ctypes.byref(shp), H.ptr(image), ctypes.byref(enc_p), H.fptr(reward), H.fptr(terminal),
               H.fptr(acts), H.fptr(dembed_w), ld, ctypes.byref(enc_g), H.ptr(ws), nbytes, H.stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(embed[:, E:]).all()), 'columns behind the image embedding were written'
        # layer 1 runs as the direct kernel: its post-ELU NHWC output is the first carve of `acts`
        out = {'y0': acts[:frames * 961 * depth].view(frames, 31, 31, depth).cpu(), 'embed': embed[:, :E].cpu()}
        for i in range(4):
            out[f'dW{i}'], out[f'db{i}'] = gw[i].cpu(), gb[i].cpu()
        outs[u8] = out
        report, failures = [], []
        checks = [('layer-1 output', 'y0', ('frame', 'y', 'x', 'out')), ('embed', 'embed', ('frame', 'feature(c,y,x)'))]
        for i in range(4):
            checks += [(f'dW{i}', f'dW{i}', ('out', 'in', 'ky', 'kx')), (f'db{i}', f'db{i}', ('out',))]
        for name, k, axes in checks:
            try:
                R.check_tensor(name, out[k], ref64[k], ref32[k], axes, report)
            except AssertionError as e:
                failures.append(str(e))
        print(f'\n[reward_input encoder, {frames} frames, depth {depth}, {"uint8" if u8 else "float"} frames]')
        for name, err, err32, bar in report:
            print(f'  {name:<16} err {err:.3e}  err_ref32 {err32:.3e}  err/err_ref32 {err / max(err32, 1e-300):7.2f}  bar {bar:.3e}')
        assert not failures, ' | '.join(failures)
        dW0 = out['dW0']
        for c in (3, 4):
            plane = dW0[:, c].reshape(depth, 16)
            assert torch.equal(plane, plane[:, :1].expand_as(plane)), f'dW0[:, {c}] varies over its 16 taps'
            assert float(plane.abs().max()) > 0
    for k in outs[False]:
        assert torch.equal(outs[False][k].view(torch.int32), outs[True][k].view(torch.int32)), f'{k}: uint8 and float frames differ'


def test_planes_entry_points_refuse_other_depths(hip):
    """cnn_depth 24 has no direct layer-1 kernel: DM_E_SHAPE, nothing launched (the model refuses it at construction)."""
    H = hip
    shp = H.make_shape(T=1, B=2, I=1, H=1, D=64, Hd=64, S=8, C=8, E=768, A=6, mlp_hidden=400, mlp_layers=4, cnn_depth=24, img=64,
                       img_ch=3, flags=0)
    t = torch.zeros(1 << 20, device=DEV)
    p = H.conv_struct([t] * 4, [t] * 4)
    with pytest.raises(H.DreamerHipError) as e:
        H.call('dm_conv_encoder_fwd_planes', ctypes.byref(shp), H.ptr(t), ctypes.byref(p), H.fptr(t), H.fptr(t), H.fptr(t), H.fptr(t),
               768, H.ptr(t), t.numel() * 4, H.stream())
    assert 'cnn_depth' in str(e.value)


@pytest.mark.parametrize('V', [4, 27])
@pytest.mark.parametrize('rows', [15, 2500, 40000])
def test_head_loss_normal_nd(hip, rows, V):
    """The loss epilogue of a DenseNormalDecoder with out_dim = V (decoders.py:295-304) against torch.distributions in fp64."""
    import math
    import torch.distributions as D
    gen = torch.Generator().manual_seed(rows * 31 + V)
    out = (2.0 * torch.randn(rows, V, generator=gen)).to(DEV)
    tgt = torch.randn(rows, V, generator=gen).to(DEV)
    std = 0.3989422804
    const = std ** 2 * (math.log(std) + math.log(math.sqrt(2 * math.pi)))      # as the model derives it; ~0 because std = 1/sqrt(2 pi)
    nan = float('nan')
    loss, dout, mean = torch.full((rows,), nan, device=DEV), torch.full((rows, V), nan, device=DEV), torch.full((rows, V), nan, device=DEV)
    hip.call('dm_head_loss_normal_nd', rows, V, hip.fptr(out), hip.fptr(tgt), 1.0 / rows, const, hip.fptr(loss), hip.fptr(dout),
             hip.fptr(mean), hip.stream())
    o = out.double().cpu().requires_grad_(True)
    ref = -D.Independent(D.Normal(o, torch.ones_like(o) * std), 1).log_prob(tgt.double().cpu()) * std ** 2
    ref.mean().backward()
    _close(loss, ref, 1e-5, 1e-6, f'loss rows {rows} V {V}')
    _close(dout, o.grad, 1e-5, 1e-9, f'dout rows {rows} V {V}')
    _close(mean, o, 1e-5, 1e-6, f'mean rows {rows} V {V}')
    hip.call('dm_head_loss_normal_nd', rows, V, hip.fptr(out), hip.fptr(tgt), 0.0, const, hip.fptr(loss), None, None, hip.stream())
    _close(loss, ref, 1e-5, 1e-6, 'loss alone (null dout / mean_out)')


# ------------------------------------------------------------------------------------------------ the sections, natively
def test_minecraft_section_runs_two_steps(hip):
    """config section `minecraft` (vecobs_size 27 beside the image, 29 actions) at its native shape B=32, T=48, cnn_depth=48."""
    from pydreamer_amd import config
    conf = config.load_config('defaults', 'minecraft')
    assert (conf.vecobs_size, conf.action_dim, conf.batch_size, conf.batch_length) == (27, 29, 32, 48)
    model = _build(conf)
    assert model.wm.encoder.out_dim == 32 * conf.cnn_depth + 256
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    T, B, A = conf.batch_length, conf.batch_size, conf.action_dim
    gen = torch.Generator().manual_seed(4)
    state = model.init_state(B)
    for s in range(2):
        obs = dict(image=torch.randint(0, 256, (T, B, 64, 64, 3), generator=gen, dtype=torch.uint8).to(DEV),
                   action=F.one_hot(torch.randint(0, A, (T, B), generator=gen), A).float().to(DEV),
                   reward=torch.randn(T, B, generator=gen).to(DEV), terminal=(torch.rand(T, B, generator=gen) < 0.05).float().to(DEV),
                   reset=(torch.rand(T, B, generator=gen) < 0.01).to(DEV), vecobs=torch.randn(T, B, 27, generator=gen).to(DEV))
        losses, state, metrics, tensors, _ = model.training_step(obs, state)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in opts:
            opt.step()
        assert all(np.isfinite(float(x)) for x in losses), [float(x) for x in losses]
        vals = {k: float(v) for k, v in {**metrics, **gm}.items()}
        assert all(np.isfinite(v) for v in vals.values()) and vals['loss_vecobs'] > 0, vals
        assert tuple(tensors['vecobs_rec'].shape) == (T, B, 27)
        dist, st1, m = model.inference({k: v[:1] for k, v in obs.items()}, tuple(x.clone() for x in state))
        assert np.isfinite(float(m['policy_value'])) and tuple(dist.probs.shape) == (1, B, A)


def test_miniworld_section_runs_two_steps(hip):
    """config section `miniworld` (probe_model='none') at its native shape B=32, T=48, cnn_depth=32, with inference() in between."""
    from pydreamer_amd import config
    conf = config.load_config('defaults', 'miniworld')
    assert conf.reward_input and (conf.batch_size, conf.batch_length, conf.cnn_depth) == (32, 48, 32)
    model = _build(conf)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    T, B, A = conf.batch_length, conf.batch_size, conf.action_dim
    gen = torch.Generator().manual_seed(3)
    state = model.init_state(B)
    for s in range(2):
        obs = dict(image=torch.randint(0, 256, (T, B, 64, 64, 3), generator=gen, dtype=torch.uint8).to(DEV),
                   action=F.one_hot(torch.randint(0, A, (T, B), generator=gen), A).float().to(DEV),
                   reward=torch.randn(T, B, generator=gen).to(DEV), terminal=(torch.rand(T, B, generator=gen) < 0.05).float().to(DEV),
                   reset=(torch.rand(T, B, generator=gen) < 0.01).to(DEV))
        losses, state, metrics, tensors, _ = model.training_step(obs, state)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in opts:
            opt.step()
        assert all(np.isfinite(float(x)) for x in losses), [float(x) for x in losses]
        vals = {k: float(v) for k, v in {**metrics, **gm}.items()}
        assert all(np.isfinite(v) for v in vals.values()), vals
        one = {k: v[:1] for k, v in obs.items()}
        dist, st1, m = model.inference(one, tuple(x.clone() for x in state))
        assert np.isfinite(float(m['policy_value'])) and tuple(dist.probs.shape) == (1, B, A)
    with torch.no_grad():      # the logging variants take the new input too
        _, _, metrics, tensors, dream = model.training_step(obs, state, do_image_pred=True, do_dream_tensors=True)
        assert np.isfinite(float(metrics['logprob_image'])) and tuple(dream['image_pred'].shape[:2]) == (T, B)
        _, _, metrics, _, _ = model.training_step(obs, state, do_open_loop=True)
        assert np.isfinite(float(metrics['loss_model']))
