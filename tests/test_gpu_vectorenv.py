"""-m gpu: image-less world models - the `vectorenv` section (image_key, image_encoder and image_decoder empty, vecobs the only
observation).

  * tests/golden/tiny_vectorenv.npz (+ _grads; two steps with carried state), tiny_vectorenv_iwae.npz (iwae_samples = 2,
    reward_input = True - ignored -, gru_layernorm) and tiny_vectorenv_cont.npz (tanh_normal actor, 3 actions, Gaussian latents,
    aux_critic), written by the real reference (scripts/gen_vectorenv_golden.py), replayed through Dreamer.training_step -> four
    backward passes -> grad_clip -> AdamW.  Bars: those tests/test_gpu_obs_inputs.py applies to tiny_vecobs / tiny_obs_combo
    (indices equal, losses 2e-5 relative or 2e-6, loss_model 1e-3 absolute, metrics 1e-4 relative or 5e-6, gradient norms 2e-3
    relative, parameter checksums 2e-6 relative, logged tensors 1e-4 relative + 1e-4 * max(1, max|ref|), full gradients 2e-3
    relative L2, out_state h 1e-5 at step 0).  The metric and tensor KEY SETS equal the fixture's: no loss_image, no image_rec.
  * tiny_vectorenv_eval / _open_loop (do_image_pred + do_dream_tensors under no_grad: no logprob_image, no image_pred,
    dream_tensors == {}), tiny_vectorenv_inference (obs without `image`), tiny_vectorenv_amp, at the bars of the tiny_obs_* tests.
  * overlap_backward / wm_tail_on_side on = off, and the same step twice, bit for bit, on tiny_vectorenv and tiny_vectorenv_iwae.
  * kernel level: dm_mlp_head_fwd / dm_mlp_head_bwd at the vecobs encoder's shape (hidden 400, 2 layers, out_dim 256, with and
    without LayerNorm), in_dim {2, 3, 4, 6} x rows {15, 1536, 16384} - 16384 rows with in_dim 4 is the one case that takes the
    row-panel kernels with a 4-wide first k-tile - EVERY element of the output and of all gradients against the same MLP in torch
    fp64 on the device; metric and bar are oracle/conv_reference.py check_tensor's.  The same entries under amp precision at in_dim
    {4, 6}: check_tensor has no bf16 counterpart, so the bars are those of tests/test_gpu_training_step.py
    test_mlp_head_panel_bf16_operands (forward within 5e-3 of the bf16-operand arithmetic in fp64 and on average five times
    closer to it than the fp32 path is; gradients within 2e-2 relative L2 of the fp32 path's).
  * DeviceReplay(image_key=None) on the device against the host reader, bit for bit, windows that wrap an episode included.
  * a model built from load_config('defaults', 'vectorenv') runs two steps at the section's native shape.
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


def _fixture_model(g, **more):
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    assert extra['image_encoder'] is None and extra['image_decoder'] is None and extra['image_key'] is None
    model = Dreamer(config.load_config('defaults', 'vectorenv', **{**vars(oconf), **extra, **more}))
    shapes = CFP.shapes_of_fixture(g)
    assert list(model.state_dict().keys()) == list(shapes.keys())
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    return oconf, model.to(DEV)


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


def _fixture_obs(g, pre, oconf):
    """The batch as preprocessing.py hands it over with image_key empty: no `image` anywhere."""
    action = F.one_hot(torch.from_numpy(g[pre + 'in_action_idx']), oconf.action_dim).float()
    obs = dict(action=action, reward=torch.from_numpy(g[pre + 'in_reward']), terminal=torch.from_numpy(g[pre + 'in_terminal']),
               reset=torch.from_numpy(g[pre + 'in_reset']), vecobs=torch.from_numpy(g[pre + 'in_vecobs']))
    noise = {k: torch.from_numpy(g[pre + 'in_' + k]).to(DEV) for k in ('u_post', 'u_act', 'u_prior', 'eps_act') if pre + 'in_' + k in g.files}
    return {k: v.to(DEV) for k, v in obs.items()}, noise


# ------------------------------------------------------------------------------------------------ the reference's fixtures
TRAIN_FIXTURES = {'tiny_vectorenv': (2, 1), 'tiny_vectorenv_iwae': (1, 2), 'tiny_vectorenv_cont': (1, 1)}      # steps, iwae_samples


@pytest.mark.parametrize('name', list(TRAIN_FIXTURES))
def test_training_steps_match_the_reference(hip, name):
    g = np.load(os.path.join(GOLD, name + '.npz'))
    steps, I = TRAIN_FIXTURES[name]
    oconf, model = _fixture_model(g)
    assert oconf.iwae_samples == I and float(g['min_edge_distance']) > 1e-5
    assert model.wm.imageless and model.wm.encoder.encoder_image is None and model.wm.decoder.image is None
    full = dict(g)
    if os.path.exists(os.path.join(GOLD, name + '_grads.npz')):
        full.update(np.load(os.path.join(GOLD, name + '_grads.npz')))
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    state = model.init_state(oconf.batch_size * I)
    T, B, S, Hh = oconf.batch_length, oconf.batch_size, oconf.stoch_dim, oconf.imag_horizon
    for s in range(steps):
        pre = f's{s}_'
        obs, noise = _fixture_obs(g, pre, oconf)
        assert 'image' not in obs
        losses, state, metrics, tensors, dream_tensors = model.training_step(obs, state, noise=noise)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(oconf.grad_clip, oconf.grad_clip_ac)
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        for opt in opts:
            opt.step()
        xh = model.last_extras
        assert dream_tensors == {}
        # the key sets are the reference's: this is what proves loss_image and image_rec are absent
        assert set({**metrics, **gm}) == {k[len(pre + 'metric_'):] for k in g.files if k.startswith(pre + 'metric_')}
        assert set(tensors.keys()) == {k[len(pre + 'tensor_'):] for k in g.files if k.startswith(pre + 'tensor_')}
        assert not [k for k in list(metrics) + list(tensors.keys()) if 'image' in k]
        assert float(model.metric_buffer[1]) == 0.0, 'metric slot 1 (loss_image) was written'
        if pre + 'idx_post' in g.files:
            assert np.array_equal(xh['post_idx'].cpu().numpy().astype(np.uint8), g[pre + 'idx_post']), (s, 'posterior indices')
            lat = xh['dream_features'][1:, :, oconf.deter_dim:].reshape(Hh, -1, S, oconf.stoch_discrete).argmax(-1)
            assert np.array_equal(lat.cpu().numpy().astype(np.uint8), g[pre + 'idx_lat']), (s, 'imagined latent indices')
        if pre + 'idx_act' in g.files:
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
                _close(tensors[k[len(pre + 'tensor_'):]], ref, 1e-4, 1e-4 * max(1.0, float(ref.abs().max())), f'step {s} {k}')
        # out_state h: 1e-5 on equal parameters (step 0); 1e-4 from step 1 on (derived in tests/test_gpu_obs_inputs.py)
        _close(state[0], torch.from_numpy(g[pre + 'out_state_h']), 0, 1e-5 if s == 0 else 1e-4, f'step {s} out_state h')
        if oconf.stoch_discrete:
            assert torch.equal(state[1].cpu(), torch.from_numpy(g[pre + 'out_state_z'])), f'step {s} out_state z'
        else:
            _close(state[1], torch.from_numpy(g[pre + 'out_state_z']), 0, 1e-5, f'step {s} out_state z')
        names = [str(n) for n in g[pre + 'grad_names']]
        # a parameter the reference leaves without a gradient (the auxiliary ActorCritic's actor, dreamer.py:347-358) may hold a
        # `.grad` here - a slice of its optimizer's flat buffer - but then it is zero
        assert names == [n for n in grads if n in set(names)]
        for n in grads:
            assert n in names or (n.startswith('wm.ac_aux.') and not bool(grads[n].any())), n
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
        assert n_full >= (6 if name == 'tiny_vectorenv' and s == 0 else 0)
        sums = np.array([float(v.double().abs().sum()) for v in model.state_dict().values()])
        np.testing.assert_allclose(sums, g[pre + 'param_abs_sums'], rtol=2e-6)


@pytest.mark.parametrize('name', ['tiny_vectorenv_eval', 'tiny_vectorenv_open_loop'])
def test_logging_variants_match_the_reference(hip, name):
    """do_image_pred + do_dream_tensors, closed loop and with do_open_loop, under no_grad; the bars of
    tests/test_gpu_obs_inputs.py test_logging_variants_match_the_reference."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    open_loop = bool(g['open_loop'])
    oconf, model = _fixture_model(g)
    obs, _ = _fixture_obs(g, '', oconf)
    noise = {k[3:]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith('in_u_')}
    with torch.no_grad():
        losses, st, metrics, tensors, dt = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise, do_image_pred=True,
                                                               do_dream_tensors=True, do_open_loop=open_loop)
    assert dt == {}
    want_t = {f[7:] for f in g.files if f.startswith('tensor_')}
    assert set(tensors.keys()) == want_t and set(metrics) == {f[7:] for f in g.files if f.startswith('metric_')}
    assert {k for k in want_t if k.startswith('logprob_') or k.endswith('_pred')} == {
        'logprob_reward', 'logprob_reward-1', 'logprob_reward1', 'logprob_terminal', 'logprob_terminal1', 'logprob_vecobs', 'reward_pred',
        'terminal_pred', 'vecobs_pred'}
    T, B, S = oconf.batch_length, oconf.batch_size, oconf.stoch_dim
    xh = model.last_extras
    assert np.array_equal(xh['post_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_post'])
    assert np.array_equal(xh['pred_idx'].cpu().numpy().astype(np.uint8).reshape(T, B, S), g['idx_pred'])
    np.testing.assert_allclose(st[0].cpu().numpy(), g['out_state_h'], rtol=0, atol=5e-6)
    for i, l in enumerate(losses):
        assert _rel(l, g['losses'][i]) < 2e-5 or abs(float(l) - g['losses'][i]) < 2e-6, (i, float(l), g['losses'][i])
    for k in metrics:
        ref = float(g['metric_' + k])
        if np.isnan(ref):
            assert torch.isnan(metrics[k]), k
        else:
            assert _rel(metrics[k], ref) < 1e-4 or abs(float(metrics[k]) - ref) < 5e-6, (k, float(metrics[k]), ref)
    for k in want_t:
        np.testing.assert_allclose(tensors[k].cpu().numpy(), g['tensor_' + k], rtol=1e-4, atol=2e-5, equal_nan=True, err_msg=k)


def test_inference_matches_the_reference(hip):
    """Dreamer.inference on an obs without `image`; bars of test_inference_matches_reference_golden: action probabilities 1e-4
    relative + 2e-6, state and policy_value 2e-6."""
    g = np.load(os.path.join(GOLD, 'tiny_vectorenv_inference.npz'))
    oconf, model = _fixture_model(g)
    obs = {k: torch.from_numpy(g['in_' + k]).to(DEV) for k in ('action', 'reset', 'reward', 'terminal', 'vecobs')}
    state = (torch.from_numpy(g['in_h']).to(DEV), torch.from_numpy(g['in_z']).to(DEV))
    with torch.no_grad():
        dist, (h1, z1), metrics = model.inference(obs, state, noise=dict(u_post=torch.from_numpy(g['in_u']).to(DEV)))
        _close(dist.probs, torch.from_numpy(g['action_probs']), 1e-4, 2e-6, 'action probabilities')
        _close(h1, torch.from_numpy(g['out_h']), 0, 2e-6, 'out_state h')
        assert torch.equal(z1.cpu(), torch.from_numpy(g['out_z']))
        assert abs(float(metrics['policy_value']) - float(g['policy_value'])) < 2e-6
        with pytest.raises(ValueError, match='vecobs'):      # the encoder's only input: leaving it out is an error
            model.inference({k: v for k, v in obs.items() if k != 'vecobs'}, state)


def test_amp_against_the_reference_autocast(hip):
    """tests/golden/tiny_vectorenv_amp.npz, produced the way tiny_obs_amp.npz is; the bars of
    test_amp_against_the_reference_autocast there: posterior indices teacher-forced to the reference's, loss_model within 1e-3
    relative of the reference's bf16 value AND of its fp32 value, the component metrics within 2e-2."""
    g = np.load(os.path.join(GOLD, 'tiny_vectorenv_amp.npz'))
    assert np.array_equal(g['fp32_idx_post'], g['bf16_idx_post'])
    oconf, model = _fixture_model(g, amp=True)
    obs, noise = _fixture_obs(g, '', oconf)
    fidx = torch.from_numpy(g['bf16_idx_post'].astype(np.int64)).to(DEV)
    with torch.no_grad():
        losses, _, metrics, _, _ = model.training_step(obs, model.init_state(oconf.batch_size), noise=noise, forced_idx=fidx)
    ref_bf16, ref_fp32 = float(g['bf16_losses'][0]), float(g['fp32_losses'][0])
    print('loss_model: build amp', float(losses[0]), 'reference autocast', ref_bf16, 'reference fp32', ref_fp32)
    assert abs(float(losses[0]) - ref_bf16) < 1e-3 * ref_bf16
    assert abs(float(losses[0]) - ref_fp32) < 1e-3 * ref_fp32
    assert 'loss_image' not in metrics
    for k in ('loss_vecobs', 'loss_reward', 'loss_terminal', 'entropy_post'):
        print(k, float(metrics[k]), float(g['bf16_metric_' + k]))
        assert _rel(metrics[k], float(g['bf16_metric_' + k])) < 2e-2, k


# ------------------------------------------------------------------------------------------------ determinism
def _run_steps(model, g, oconf, steps):
    opts = model.init_optimizers(oconf.adam_lr, oconf.adam_lr_actor, oconf.adam_lr_critic, oconf.adam_eps)
    st = model.init_state(oconf.batch_size * oconf.iwae_samples)
    hist = []
    for s in range(steps):
        obs, noise = _fixture_obs(g, f's{s}_', oconf)
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


@pytest.mark.parametrize('name', ['tiny_vectorenv', 'tiny_vectorenv_iwae'])
@pytest.mark.parametrize('switch', ['overlap_backward', 'wm_tail_on_side', 'twice'])
def test_backward_placement_is_bit_identical(hip, switch, name):
    """The vecobs encoder's backward closes the pre-launched world-model backward: same bits whether that pass runs on its side
    stream or inside backward(), whether the forward's tail runs on the side stream or on the caller's, and run to run."""
    g = np.load(os.path.join(GOLD, name + '.npz'))
    runs = []
    for on in (True, False):
        oconf, model = _fixture_model(g)
        assert model.overlap_backward and model.wm_tail_on_side
        if switch != 'twice':
            setattr(model, switch, on)
        runs.append(_run_steps(model, g, oconf, TRAIN_FIXTURES[name][0]))
        if switch == 'wm_tail_on_side':
            assert (model.wm._last_pack.get('tail') is not None) == on
    _assert_same_runs(runs[0], runs[1], switch)


# ------------------------------------------------------------------------------------------------ kernel level
HIDDEN, LAYERS, OUT = 400, 2, 256


def _encoder_mlp(in_dim, ln, seed):
    from pydreamer_amd.models import MLP
    torch.manual_seed(seed)
    m = MLP(in_dim, OUT, HIDDEN, LAYERS, layer_norm=ln).to(DEV)
    if ln:
        with torch.no_grad():
            for i in range(LAYERS):
                m.model[3 * i + 1].weight.uniform_(0.5, 1.5)
                m.model[3 * i + 1].bias.uniform_(-0.5, 0.5)
    return m


def _bf16_product(rows, K, N):
    """Does precision = 1 round the operands of a rows x N x K Linear product?  Yes, except (csrc/gemm.hip dm_gemm_launch) where
    the product goes to the one-launch skinny kernel, which keeps fp32 operands (csrc/gemm_skinny.hip skinny_ok /
    dm_gemm_skinny_try: at most 512 rows, K >= 16 and a multiple of 4, N * K >= 64 Ki, and beyond 64 rows K <= 1024 with
    N * K <= 1100 Ki), and where K is no multiple of 4: those rare shapes run the scalar-load tile, which has no bf16 variant."""
    skinny = rows <= 512 and K >= 16 and K % 4 == 0 and N * K >= 64 * 1024 and (rows <= 64 or (K <= 1024 and N * K <= 1100 * 1024))
    return not skinny and K % 4 == 0


def _torch_mlp(m, x, dout, dtype, ln, bf16=False):
    """The same MLP in torch on the device of its arguments: (out, gradients in parameters() order).  bf16: the operands of the
    Linear products that precision = 1 rounds (_bf16_product) rounded to bf16, everything else in `dtype`."""
    ps = [p.detach().to(dtype).clone().requires_grad_(True) for p in m.parameters()]
    named = dict(zip([n for n, _ in m.named_parameters()], ps))
    rows = x.shape[0]

    def linear(h, i, N):
        w, b = named[f'model.{3 * i}.weight'], named[f'model.{3 * i}.bias']
        if bf16 and _bf16_product(rows, h.shape[1], N):
            h, w = h.float().bfloat16().to(dtype), w.float().bfloat16().to(dtype)
        return F.linear(h, w, b)
    h = x.to(dtype)
    for i in range(LAYERS):
        pre = linear(h, i, HIDDEN)
        if ln:
            pre = F.layer_norm(pre, (HIDDEN,), named[f'model.{3 * i + 1}.weight'], named[f'model.{3 * i + 1}.bias'], 1e-3)
        h = F.elu(pre)
    out = linear(h, LAYERS, OUT)
    if dout is None:
        return out.detach(), None
    return out.detach(), [t.detach() for t in torch.autograd.grad(out, ps, dout.to(dtype))]


def _call_entries(H, m, x, dout, rows, in_dim):
    """dm_mlp_head_fwd + dm_mlp_head_bwd through the C-ABI into NaN-filled buffers: (out, gradients in parameters() order)."""
    nan = float('nan')
    ws = torch.empty(4 * int(H.lib().dm_mlp_ws_floats(rows, HIDDEN, LAYERS)), dtype=torch.uint8, device=DEV)
    acts = torch.full((int(H.lib().dm_mlp_acts_floats(rows, HIDDEN, LAYERS)),), nan, device=DEV)
    out = torch.full((rows, OUT), nan, device=DEV)
    grads = [torch.full_like(p, nan) for p in m.parameters()]
    gof = {id(p): t for p, t in zip(m.parameters(), grads)}
    st, gs = m.struct(), m.grad_struct(gof)
    H.call('dm_mlp_head_fwd', rows, in_dim, HIDDEN, LAYERS, OUT, H.fptr(x), in_dim, ctypes.byref(st), H.fptr(acts), H.fptr(out),
           H.ptr(ws), ws.numel(), H.stream())
    H.call('dm_mlp_head_bwd', rows, in_dim, HIDDEN, LAYERS, OUT, H.fptr(x), in_dim, ctypes.byref(st), H.fptr(acts), H.fptr(dout),
           ctypes.byref(gs), None, 0, 0, H.ptr(ws), ws.numel(), H.stream())
    torch.cuda.synchronize()
    return out, grads


@pytest.mark.parametrize('ln', [True, False], ids=['layernorm', 'nonorm'])
@pytest.mark.parametrize('rows', [15, 1536, 16384])
@pytest.mark.parametrize('in_dim', [2, 3, 4, 6])
def test_vecobs_encoder_mlp_every_element(hip, in_dim, rows, ln):
    H = hip
    m = _encoder_mlp(in_dim, ln, seed=7)
    gen = torch.Generator().manual_seed(rows * 31 + in_dim)
    x = torch.randn(rows, in_dim, generator=gen).to(DEV)
    dout = torch.randn(rows, OUT, generator=gen).to(DEV)
    out, grads = _call_entries(H, m, x, dout, rows, in_dim)
    out64, g64 = _torch_mlp(m, x, dout, torch.float64, ln)
    out32, g32 = _torch_mlp(m, x, dout, torch.float32, ln)
    report, failures = [], []
    checks = [('out', out, out64, out32, ('row', 'feature'))]
    for (n, p), got, r64, r32 in zip(m.named_parameters(), grads, g64, g32):
        checks.append(('d ' + n, got, r64, r32, ('out', 'in') if p.dim() == 2 else ('out',)))
    for name, got, r64, r32, axes in checks:
        try:
            R.check_tensor(name, got.cpu(), r64.cpu(), r32.cpu(), axes, report)
        except AssertionError as e:
            failures.append(str(e))
    print(f'\n[vecobs encoder MLP, in_dim {in_dim}, {rows} rows, layer_norm {ln}]')
    for name, err, err32, bar in report:
        print(f'  {name:<22} err {err:.3e}  err_ref32 {err32:.3e}  err/err_ref32 {err / max(err32, 1e-300):7.2f}  bar {bar:.3e}')
    assert not failures, ' | '.join(failures)


@pytest.mark.parametrize('rows', [15, 1536, 16384])
@pytest.mark.parametrize('in_dim', [4, 6])
def test_vecobs_encoder_mlp_amp(hip, in_dim, rows):
    """precision = 1 (conf.amp).  oracle/conv_reference.py check_tensor has no bf16 counterpart; the bars are those of
    tests/test_gpu_training_step.py test_mlp_head_panel_bf16_operands, against the same kind of reference: fp64 arithmetic on the
    operands as the library rounds them (_bf16_product).  At 15 rows that is the first Linear only - the 400-deep products of so
    few rows run on the skinny kernel, which keeps fp32 operands - and with in_dim 6 never the first one (no bf16 tile for a K that
    is no multiple of 4); at 6 x 15 nothing is rounded and the result is the fp32 path's, bit for bit."""
    H = hip
    m = _encoder_mlp(in_dim, True, seed=9)
    gen = torch.Generator().manual_seed(rows * 37 + in_dim)
    x = torch.randn(rows, in_dim, generator=gen).to(DEV)
    dout = (torch.randn(rows, OUT, generator=gen) / rows).to(DEV)
    out32, g32 = _call_entries(H, m, x, dout, rows, in_dim)
    m.precision = 1
    out, g16 = _call_entries(H, m, x, dout, rows, in_dim)
    out_b, _ = _call_entries(H, m, x, dout, rows, in_dim)
    assert torch.equal(out, out_b)
    if not any(_bf16_product(rows, K, N) for K, N in ((in_dim, HIDDEN), (HIDDEN, HIDDEN), (HIDDEN, OUT))):
        assert torch.equal(out, out32), 'no product of this shape takes bf16 operands: the fp32 kernels on the same operands'
        return
    ref, _ = _torch_mlp(m, x, None, torch.float64, True, bf16=True)
    err, gap = (out.double() - ref).abs(), (out32.double() - ref).abs()
    print(f'in_dim {in_dim} rows {rows}: err max {float(err.max()):.3e} mean {float(err.mean()):.3e}, fp32 path gap mean {float(gap.mean()):.3e}')
    assert float(err.max()) < 5e-3 and float(err.mean()) < 0.2 * float(gap.mean()), (float(err.max()), float(err.mean()), float(gap.mean()))
    for (n, _), a, b in zip(m.named_parameters(), g16, g32):
        e = _rel_l2(a, b)
        print(f'  d {n}: relative L2 to the fp32 path {e:.3e}')
        assert e < 2e-2, (n, e)


# ------------------------------------------------------------------------------------------------ the device-resident feed
def test_device_replay_without_frames_matches_the_host_reader(hip, tmp_path):
    from pydreamer_amd import replay as RP
    from tests.test_vectorenv_cpu import KW, _write_episodes
    repo = _write_episodes(tmp_path)
    depth, nb = 3, 14
    plain = iter(RP.SequentialReplay(repo, **KW))
    dr = RP.DeviceReplay(RP.SequentialReplay(repo, **KW), 2, DEV, depth=depth, clip_rewards='tanh', image_key=None)
    assert 'image' not in dr.names
    handed = []
    for i in range(nb):
        got = dr.next()
        if i % 2:
            dr.prefetch()
        assert all(v.is_cuda for v in got.values()) and 'image' not in got
        handed.append({k: v.clone() for k, v in got.items()})
    torch.cuda.synchronize()
    dr.close()
    wrapped = 0
    for i, got in enumerate(handed):
        want = RP.preprocess_batch(next(plain), 2, clip_rewards='tanh', image_key=None)
        assert sorted(got) == sorted(want)
        for k, w in want.items():
            gk = got[k].cpu().numpy()
            assert gk.dtype == w.dtype and gk.shape == w.shape, (i, k, gk.dtype, w.dtype)
            assert gk.tobytes() == np.ascontiguousarray(w).tobytes(), (i, k)
        wrapped += int(want['reset'][1:].any())
    assert wrapped > 0, 'no window wrapped an episode boundary'


# ------------------------------------------------------------------------------------------------ the section, natively
def test_vectorenv_section_runs_two_steps(hip, tmp_path):
    """config section `vectorenv` at its native shape B=32, T=48, deter_dim 2048, hidden_dim 1000, H=15, fed by a DeviceReplay of
    image-less episodes: two steps with carried state, finite losses, no image tensor anywhere."""
    from pydreamer_amd import config
    from pydreamer_amd import replay as RP
    from pydreamer_amd.models import Dreamer
    conf = config.load_config('defaults', 'vectorenv')
    assert (conf.batch_size, conf.batch_length, conf.deter_dim, conf.hidden_dim, conf.imag_horizon) == (32, 48, 2048, 1000, 15)
    torch.manual_seed(0)
    model = Dreamer(conf).to(DEV)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    T, B = conf.batch_length, conf.batch_size
    rs = np.random.RandomState(5)
    repo = RP.LocalEpisodeRepository(str(tmp_path))
    for ep, n in enumerate([150, 210, 180, 260]):
        d = dict(action=rs.randint(0, 2, n), reward=rs.randn(n).astype(np.float32), terminal=np.zeros(n, bool), reset=np.zeros(n, bool),
                 vecobs=rs.randn(n, 4).astype(np.float32))
        d['terminal'][-1] = True
        repo.save_data(d, ep, ep)
    dr = RP.DeviceReplay(RP.SequentialReplay(repo, T, B, allow_mid_reset=True, seed=3), conf.action_dim, DEV, clip_rewards='tanh',
                         image_key=conf.image_key)
    state = model.init_state(B)
    for s in range(2):
        obs = dr.next()
        assert 'image' not in obs and tuple(obs['vecobs'].shape) == (T, B, 4)
        losses, state, metrics, tensors, _ = model.training_step(obs, state)
        for opt in opts:
            opt.zero_grad()
        for loss in losses:
            loss.backward()
        gm = model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
        for opt in opts:
            opt.step()
        sched = dict(fwd=hip.last_schedule(0), rollout=hip.last_schedule(2))      # (of this thread's calls)
        vals = {k: float(v) for k, v in {**metrics, **gm}.items()}
        assert all(np.isfinite(float(x)) for x in losses), (f'dm_rssm_last_schedule {sched}', [float(x) for x in losses])
        assert all(np.isfinite(v) for v in vals.values()) and vals['loss_vecobs'] > 0, (f'dm_rssm_last_schedule {sched}', vals)
        assert not [k for k in list(metrics) + list(tensors.keys()) if 'image' in k]
        assert tuple(tensors['vecobs_rec'].shape) == (T, B, 4)
        dist, st1, m = model.inference({k: v[:1] for k, v in obs.items()}, tuple(x.clone() for x in state))
        assert np.isfinite(float(m['policy_value'])) and tuple(dist.probs.shape) == (1, B, 2)
    dr.close()
