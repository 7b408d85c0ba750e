"""CPU (-m "not gpu"): pin oracle/dreamer_oracle.py against golden vectors produced by the real reference
(oracle/gen_golden.py, run in the build container where /root/reference exists).

Bars: sampled indices (posterior / actor / imagined latents) bit-exact; losses and metrics within 2e-5 relative
(fp32, same torch CPU kernels, different op grouping); recurrent state within STATE_ATOL; per-parameter gradient norms within
1e-4 relative (+1e-7 abs); stored full gradients within 1e-4 of the tensor's max; post-AdamW parameter sums within 1e-6 of the
largest sum of absolute values, which are within PARAM_ABS_RTOL relative.
"""
import ast
import os

import numpy as np
import pytest
import torch

from oracle import dreamer_oracle as O

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
# fp32 summation order depends on the host's BLAS kernels (CPU vendor, ISA, thread count): on the same inputs the oracle's
# recurrent state moves by up to 2.7e-6 and a parameter's post-AdamW sum of absolute values by up to 2.0e-6 relative between
# the host that wrote the fixtures and others.  Sampled indices stay bit-exact on every host.
STATE_ATOL = 1e-5
PARAM_ABS_RTOL = 1e-5


def _load(name):
    return np.load(os.path.join(GOLD, f'{name}.npz'), allow_pickle=False)


def _conf_from(g):
    items = ast.literal_eval(str(g['conf_json']))      # repr of a sorted (key, value) list written by gen_golden.py
    return O.make_conf(**dict(items))


def _replay(name, steps):
    g = _load(name)
    conf = _conf_from(g)
    torch.manual_seed(0)
    model = O.OracleDreamer(conf, O.make_params(conf, seed=0))
    model.init_optimizers()
    state = model.init_state(conf.batch_size * conf.iwae_samples)
    results = []
    for s in range(steps):
        pre = f's{s}_'
        raw = {k: g[pre + 'in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
        obs = O.preprocess(raw, conf)
        noise = {k: torch.from_numpy(g[pre + 'in_' + k]) for k in ('u_post', 'u_act', 'u_prior', 'eps_act') if pre + 'in_' + k in g.files}
        assert np.array_equal(state[0].numpy(), g[pre + 'in_state_h']) or s > 0
        losses, new_state, metrics, tensors, extras = model.training_step(obs, state, noise)
        grad_metrics, grads = model.backward_clip_step(losses)
        sums = np.array([float(v.detach().double().sum()) for v in model.p.values()])
        abss = np.array([float(v.detach().double().abs().sum()) for v in model.p.values()])
        results.append((pre, losses, new_state, metrics, tensors, extras, grad_metrics, grads, (sums, abss)))
        state = new_state
    return g, conf, results


def _rel(a, b):
    a = float(a.detach()) if torch.is_tensor(a) else float(a)
    return abs(a - float(b)) / max(abs(float(b)), 1e-12)


def _check_step(g, conf, res):
    pre, losses, new_state, metrics, tensors, extras, grad_metrics, grads, (sums, abss) = res
    T, B, S, H = conf.batch_length, conf.batch_size, conf.stoch_dim, conf.imag_horizon
    # integer outputs: bit-exact
    assert np.array_equal(extras['post_idx'].reshape(T, B * conf.iwae_samples, S).numpy().astype(np.uint8), g[pre + 'idx_post'])
    assert np.array_equal(extras['act_idx'].numpy().astype(np.uint8), g[pre + 'idx_act'])
    assert np.array_equal(extras['lat_idx'].numpy().astype(np.uint8), g[pre + 'idx_lat'])
    # losses / metrics
    for i, l in enumerate(losses):
        assert _rel(l, g[pre + 'losses'][i]) < 2e-5 or abs(float(l) - g[pre + 'losses'][i]) < 2e-6, (i, float(l), g[pre + 'losses'][i])
    for k, v in {**metrics, **grad_metrics}.items():
        ref = float(g[pre + 'metric_' + k])
        assert _rel(v, ref) < 5e-5 or abs(float(v) - ref) < 2e-6, (k, float(v), ref)
    # tensors
    for k, v in tensors.items():
        if k == 'image_rec':
            assert _rel(v.double().sum(), g[pre + 'tensor_image_rec_sum']) < 1e-5
            np.testing.assert_allclose(v[:1, :1].numpy(), g[pre + 'tensor_image_rec_frames'], rtol=0, atol=2e-5)
        else:
            ref = g[pre + 'tensor_' + k]
            np.testing.assert_allclose(v.numpy(), ref, rtol=2e-5, atol=2e-5 * max(1.0, np.abs(ref).max()))
    np.testing.assert_allclose(new_state[0].numpy(), g[pre + 'out_state_h'], rtol=0, atol=STATE_ATOL)
    if conf.stoch_discrete:
        assert np.array_equal(new_state[1].numpy(), g[pre + 'out_state_z'])
    else:                           # Gaussian latents: z = mean + std * eps, as exact as the state it is drawn from
        np.testing.assert_allclose(new_state[1].numpy(), g[pre + 'out_state_z'], rtol=0, atol=STATE_ATOL)
    # gradients
    names = [str(n) for n in g[pre + 'grad_names']]
    assert names == list(grads.keys())
    for n, ref in zip(names, g[pre + 'grad_norms']):
        got = float(grads[n].double().norm())
        assert abs(got - ref) <= 1e-4 * ref + 1e-7, (n, got, ref)
    for key in g.files:
        if key == pre + 'grad_proj':      # gradient DIRECTION of every parameter: two closed-form projections (O.grad_probe)
            for i, (n, r, pr) in enumerate(zip(names, g[pre + 'grad_norms'], g[key])):
                got = O.grad_probe(grads[n], i)
                assert max(abs(got[0] - pr[0]), abs(got[1] - pr[1])) <= 1e-4 * r + 1e-9, (n, got, pr, r)
        elif key.startswith(pre + 'grad_') and key not in (pre + 'grad_norms', pre + 'grad_names'):
            n = key[len(pre + 'grad_'):]
            ref = g[key]
            np.testing.assert_allclose(grads[n].numpy(), ref, rtol=0, atol=1e-4 * max(np.abs(ref).max(), 1e-8))
    # post-step parameters
    np.testing.assert_allclose(abss, g[pre + 'param_abs_sums'], rtol=PARAM_ABS_RTOL)
    np.testing.assert_allclose(sums, g[pre + 'param_sums'], rtol=0, atol=1e-6 * abss.max())


def test_param_table_matches_reference_state_dict():
    """The golden generator asserted strict key/shape equality with the reference's state_dict; here we pin the count
    and total size it saw (Atari-literal 25.3 M parameters incl. critic_target)."""
    conf = O.atari_literal_conf()
    shapes = O.param_shapes(conf)
    total = sum(int(np.prod(s)) for k, s in shapes.items() if not k.startswith('ac.critic_target'))
    assert abs(total - 25.3e6) < 0.1e6, total
    assert len(shapes) == len(set(shapes))


def test_oracle_matches_reference_tiny_two_steps():
    g, conf, results = _replay('tiny', 2)
    for res in results:
        _check_step(g, conf, res)


def test_oracle_matches_reference_probe_gradients():
    """probe_gradients=True with probe_model=none (dreamer.py:60-87,183-186): three optimizers, losses = (loss_model + loss_probe,
    loss_actor, loss_critic), three gradient norms; the probe head's dummy parameter accumulates a gradient nobody zeroes or
    steps (0.5 after step 0, 1.0 after step 1 - it is in the fixture's grad_names).  Two consecutive steps."""
    g, conf, results = _replay('tiny_probe_gradients', 2)
    assert conf.probe_gradients is True
    for res in results:
        assert len(res[1]) == 3 and set(res[6]) == {'grad_norm', 'grad_norm_actor', 'grad_norm_critic'}
        _check_step(g, conf, res)


def test_oracle_matches_reference_iwae():
    """iwae_samples = 3 as a training step (two consecutive steps): batch expansion by I (rssm.py:35-41),
    sampled KL (dreamer.py:340-343), loss_model = -logavgexp(-loss_tbi) (functions.py:97-102), gradients included."""
    g, conf, results = _replay('tiny_iwae', 2)
    assert conf.iwae_samples == 3
    for res in results:
        _check_step(g, conf, res)


@pytest.mark.parametrize('gru_type', ['gru_layernorm', 'gru_layernorm_dv2'])
def test_oracle_matches_reference_layernorm_gru_cells(gru_type):
    """NormGRUCell / NormGRUCellLateReset (rnn.py:95-138) in place of nn.GRUCell, two training steps."""
    g, conf, results = _replay('tiny_' + gru_type, 2)
    assert conf.gru_type == gru_type
    for res in results:
        _check_step(g, conf, res)


def test_oracle_matches_reference_gru_cell_stack():
    """GRUCellStack with gru_layers = 3 (rnn.py:40-67; each cell deter_dim/3 wide, layer i fed by layer
    i-1's new state), two training steps."""
    g, conf, results = _replay('tiny_gru_layers3', 2)
    assert (conf.gru_layers, conf.deter_dim) == (3, 96)
    for res in results:
        _check_step(g, conf, res)


def test_oracle_matches_reference_no_layernorm():
    """SURVEY 8(a) variant: layer_norm=False - NoNorm (common.py:68-74) in every MLP head and in the RSSM cell's in / post /
    prior norms, two training steps; the state_dict has no norm parameters at all."""
    g, conf, results = _replay('tiny_no_layernorm', 2)
    assert conf.layer_norm is False and not any('norm' in k or k.endswith('.1.weight') for k in O.param_shapes(conf)
                                                  if k.startswith(('wm.core', 'ac.')))
    for res in results:
        _check_step(g, conf, res)


def test_oracle_matches_reference_gaussian_latents():
    """SURVEY 8(a) variant: stoch_discrete = 0 - Gaussian latents (rssm.py:103-117,195-203; functions.py:46-56 diag_normal:
    std = 2 sigmoid(.) + 0.1): reparameterised samples, the Normal KL with balancing, entropies, the rollout's prior
    samples; two training steps incl. the gradient direction of every parameter.  (The HIP path is checked against the
    same fixture in tests/test_gpu_training_step.py.)"""
    g, conf, results = _replay('tiny_gaussian_latents', 2)
    assert conf.stoch_discrete == 0 and O.feature_dim(conf) == conf.deter_dim + conf.stoch_dim
    for res in results:
        _check_step(g, conf, res)


def test_oracle_matches_reference_normal_tanh_actor():
    """SURVEY 8(a) variant: actor_dist = normal_tanh (functions.py:59-66: Independent(Normal(tanh(mean_), sigmoid(std_) + 0.01)),
    no transform on the sample), continuous actions under actor_grad = reinforce, two training steps incl. gradients."""
    g, conf, results = _replay('tiny_normal_tanh', 2)
    assert conf.actor_dist == 'normal_tanh' and conf.actor_grad == 'reinforce'
    for res in results:
        _check_step(g, conf, res)


def test_oracle_matches_reference_off_default_scalars():
    """Every scalar hyper-parameter of the path away from its default at once (loss weights, KL weight / balance, discount,
    GAE lambda, entropy weight, learning rates, Adam eps, target refresh every step) with gradient clips that BIND
    (grad_clip 100, grad_clip_ac 0.2), three consecutive training steps."""
    g, conf, results = _replay('tiny_scalars', 3)
    assert (conf.kl_weight, conf.kl_balance, conf.reward_weight, conf.grad_clip_ac, conf.target_interval) == (0.3, 0.65, 2.0, 0.2, 1)
    assert float(g['s0_metric_grad_norm']) > conf.grad_clip and float(g['s0_metric_grad_norm_actor']) > conf.grad_clip_ac
    for res in results:
        _check_step(g, conf, res)


def test_oracle_matches_reference_combined_variants():
    """The structural variants of SURVEY 8(a) TOGETHER: Gaussian latents, a 2-layer stack of late-reset LayerNorm GRU cells,
    NoNorm MLPs, the auxiliary critic and a tanh_normal actor on continuous actions; two training steps incl. gradients."""
    g, conf, results = _replay('tiny_combo', 2)
    assert (conf.stoch_discrete, conf.gru_type, conf.gru_layers, conf.layer_norm, conf.aux_critic, conf.actor_dist) == \
        (0, 'gru_layernorm_dv2', 2, False, True, 'tanh_normal')
    for res in results:
        _check_step(g, conf, res)


def test_oracle_matches_reference_plain_kl():
    """SURVEY 8(a) variant: kl_balance = 0.5 selects the un-balanced KL (dreamer.py:241: `None if kl_balance == 0.5`,
    dreamer.py:334-335), two training steps incl. gradients of the prior / posterior heads."""
    g, conf, results = _replay('tiny_kl_plain', 2)
    assert conf.kl_balance == 0.5
    for res in results:
        _check_step(g, conf, res)


@pytest.mark.parametrize('name', ['tiny_gaussian_iwae', 'tiny_gru_layernorm_layers2'])
def test_oracle_matches_reference_corners_ahead_of_the_product(name):
    """Two corners the HIP path still refuses, pinned in the oracle ahead of it: Gaussian latents with
    iwae_samples = 2 (the sampled Normal log-density KL, dreamer.py:340-343) and a 2-layer stack of NormGRUCell
    (rnn.py:40-67,95-114)."""
    g, conf, results = _replay(name, 1)
    _check_step(g, conf, results[0])


def test_oracle_matches_reference_aux_critic():
    """aux_critic (dreamer.py:267-279,347-358), two training steps."""
    g, conf, results = _replay('tiny_aux_critic', 2)
    assert conf.aux_critic
    for res in results:
        _check_step(g, conf, res)


def test_oracle_matches_reference_debug_literal():
    """BASELINE.json configs[0]: defaults+atari+debug, B=4, T=10, H=5, discrete(6)."""
    g, conf, results = _replay('debug_literal', 1)
    assert (conf.batch_size, conf.batch_length, conf.imag_horizon, conf.action_dim, conf.deter_dim) == (4, 10, 5, 6, 1024)
    _check_step(g, conf, results[0])


def test_oracle_matches_reference_continuous_actor():
    """BASELINE.json configs[4] family: defaults+dmc (tanh_normal Gaussian actor) with actor_grad=reinforce, tiny dims."""
    g, conf, results = _replay('tiny_dmc', 1)
    assert (conf.actor_dist, conf.actor_grad, conf.action_dim, conf.entropy) == ('tanh_normal', 'reinforce', 4, 1.0e-4)
    _check_step(g, conf, results[0])
    assert np.isfinite(g['s0_losses']).all()


def test_sampler_rule_edges():
    """Inverse-CDF rule: u=0 -> first category with mass, u->1 -> last, delta distribution exact."""
    p = torch.tensor([[0.0, 0.5, 0.5, 0.0], [0.25, 0.25, 0.25, 0.25], [0.0, 0.0, 1.0, 0.0]])
    assert O.sample_inverse_cdf(p, torch.tensor([0.0, 0.0, 0.3])).tolist() == [1, 0, 2]
    assert O.sample_inverse_cdf(p, torch.tensor([0.999, 0.999999, 0.999])).tolist() == [2, 3, 2]


def _check_full_size_step(name):
    """A full-size training step of the oracle against a slim golden written by the real reference; inputs are regenerated
    from the same seeds and fingerprinted."""
    g = _load(name)
    conf = _conf_from(g)
    raw = O.synthetic_batch(conf, seed=1234, first=True)
    noise = O.make_noise(conf, seed=777)
    assert int(raw['image_u8'].astype(np.int64).sum()) == int(g['s0_in_image_sum'])
    model = O.OracleDreamer(conf, O.make_params(conf, seed=0))
    model.init_optimizers()
    losses, new_state, metrics, tensors, extras = model.training_step(O.preprocess(raw, conf),
                                                                      model.init_state(conf.batch_size), noise)
    T, B, S = conf.batch_length, conf.batch_size, conf.stoch_dim
    # world model: bit-exact indices, losses to fp32 noise.  Measured here: all 80 000 posterior draws identical,
    # loss_model and grad_norm identical to the last bit.
    assert np.array_equal(extras['post_idx'].reshape(T, B, S).numpy().astype(np.uint8), g['s0_idx_post'])
    assert _rel(losses[0], g['s0_losses'][0]) < 2e-6
    # imagination: 37 500 actor + 1.2 M latent draws; ONE draw whose uniform sits within an ulp of a CDF edge flips under
    # the oracle's op grouping (measured: first difference at imagination step 4, one of 2500 rows) and that row then
    # follows another trajectory - 0.05 % of the actor indices, 3e-3 relative on loss_actor.  Bars set accordingly.
    act_same = (extras['act_idx'].numpy().astype(np.uint8) == g['s0_idx_act'])
    assert act_same[:4].all() and act_same.mean() > 0.998, act_same.mean(1)
    lat_same = (extras['lat_idx'].sum(-1).numpy().astype(np.uint16) == g['s0_idx_lat_rowsum'])
    assert lat_same.mean() > 0.997, lat_same.mean(1)
    grad_metrics, grads = model.backward_clip_step(losses)
    wm_keys = ('loss_model', 'loss_kl', 'entropy_prior', 'entropy_post', 'loss_image', 'loss_reward', 'loss_terminal',
               'grad_norm', 'grad_norm_probe')
    for k, v in {**metrics, **grad_metrics}.items():
        ref = float(g['s0_metric_' + k])
        tol = 2e-6 if k in wm_keys else 1e-2
        assert _rel(v, ref) < tol or abs(float(v) - ref) < 1e-3 * (k not in wm_keys) + 1e-7, (k, float(v), ref)
    # world-model gradient DIRECTIONS (two closed-form projections per parameter, O.grad_probe); the actor / critic
    # gradients inherit the one diverged imagination row and are left to the norm-level metrics above
    if 's0_grad_proj' in g.files:
        names = [str(n) for n in g['s0_grad_names']]
        for i, (n, r, pr) in enumerate(zip(names, g['s0_grad_norms'], g['s0_grad_proj'])):
            if not n.startswith('wm.') or n not in grads:
                continue
            got = O.grad_probe(grads[n], i)
            assert max(abs(got[0] - pr[0]), abs(got[1] - pr[1])) <= 1e-4 * r + 1e-9, (n, got, pr, r)


def test_oracle_matches_reference_at_atari_literal():
    """BASELINE.json configs[1] at full size (B=50,T=50,H=15, deter 600)."""
    _check_full_size_step('atari_literal')


def test_oracle_matches_reference_at_atari_native():
    """pydreamer's OWN Atari configuration as shipped (defaults+atari: B=32, T=48, deter_dim 1024, H=15, action_dim 18 - what the
    reference's README measured and `bench.py --workload atari-native` runs), full step incl. gradient directions."""
    g = _load('atari_native')
    conf = _conf_from(g)
    assert (conf.batch_size, conf.batch_length, conf.deter_dim, conf.imag_horizon) == (32, 48, 1024, 15)
    _check_full_size_step('atari_native')


def test_oracle_matches_reference_at_dmc_native():
    """BASELINE.json configs[4] at its native width (defaults+dmc: deter_dim 2048, tanh_normal actor, action_dim 6,
    actor_grad=reinforce, B=50, T=50, H=15) against the slim golden written by the real reference.  Forward only here
    (the backward of the 2048-wide model costs minutes on CPU; the GPU test covers the gradients against this fixture)."""
    g = _load('dmc_native')
    conf = _conf_from(g)
    assert conf.deter_dim == 2048 and conf.actor_dist == 'tanh_normal' and conf.action_dim == 6
    raw = O.synthetic_batch(conf, seed=1234, first=True)
    noise = O.make_noise(conf, seed=777)
    assert int(raw['image_u8'].astype(np.int64).sum()) == int(g['s0_in_image_sum'])
    model = O.OracleDreamer(conf, O.make_params(conf, seed=0))
    with torch.no_grad():
        losses, new_state, metrics, tensors, extras = model.training_step(O.preprocess(raw, conf),
                                                                          model.init_state(conf.batch_size), noise)
    T, B, S = conf.batch_length, conf.batch_size, conf.stoch_dim
    same = extras['post_idx'].reshape(T, B, S).numpy().astype(np.uint8) == g['s0_idx_post']
    assert same[:10].all() and same.mean() > 0.999, same.mean()
    assert _rel(losses[0], g['s0_losses'][0]) < 2e-5
    for i in (2, 3):
        assert _rel(losses[i], g['s0_losses'][i]) < 2e-2 or abs(float(losses[i]) - g['s0_losses'][i]) < 2e-3, i
    for k in ('loss_kl', 'entropy_prior', 'entropy_post', 'loss_image', 'loss_reward', 'loss_terminal'):
        assert _rel(metrics[k], float(g['s0_metric_' + k])) < 2e-5, k


@pytest.mark.parametrize('name,open_loop', [('tiny_eval', False), ('tiny_open_loop', True),
                                            ('tiny_eval_iwae', False), ('tiny_open_loop_iwae', True)])
def test_oracle_logging_variants_match_reference(name, open_loop):
    """do_image_pred + do_dream_tensors (dreamer.py:163-180,381-394; called by train.py:353-359,380-385), without and
    with do_open_loop (rssm.py:50-53), against the fixtures written by the real reference.  The *_iwae fixtures are
    evaluate()'s own call shape: iwae_samples=3 passed TOGETHER with the flags to a model whose conf.iwae_samples is 1."""
    g = _load(name)
    conf = _conf_from(g)
    Ie = int(g['iwae_samples']) if 'iwae_samples' in g.files else None
    raw = {k: g['in_' + k] for k in ('image_u8', 'action_idx', 'reward', 'terminal', 'reset')}
    noise = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('in_u_') or k.startswith('in_eps_')}
    model = O.OracleDreamer(conf, O.make_params(conf, seed=0))
    with torch.no_grad():
        losses, st, metrics, tensors, ex = model.training_step(O.preprocess(raw, conf), model.init_state(conf.batch_size * (Ie or 1)),
                                                               noise, do_image_pred=True, do_dream_tensors=True,
                                                               do_open_loop=open_loop, iwae_samples=Ie)
    assert np.array_equal(ex['post_idx'].numpy().astype(np.uint8).reshape(g['idx_post'].shape), g['idx_post'])
    np.testing.assert_allclose(st[0].numpy(), g['out_state_h'], rtol=0, atol=2e-6)
    assert np.array_equal(ex['pred_idx'].numpy().astype(np.uint8).reshape(g['idx_pred'].shape), g['idx_pred'])
    assert np.array_equal(ex['dream_log_idx']['act_idx'].numpy().astype(np.uint8), g['idx_log_act'])
    assert np.array_equal(ex['dream_log_idx']['lat_idx'].numpy().astype(np.uint8), g['idx_log_lat'])
    for k in [f[7:] for f in g.files if f.startswith('metric_')]:
        ref = float(g['metric_' + k])
        if np.isnan(ref):
            assert torch.isnan(metrics[k]), k
        else:
            assert _rel(metrics[k], ref) < 5e-5 or abs(float(metrics[k]) - ref) < 2e-6, (k, float(metrics[k]), ref)
    for k in [f[7:] for f in g.files if f.startswith('tensor_') and not f.endswith(('_sum', '_frame'))]:
        np.testing.assert_allclose(tensors[k].numpy(), g['tensor_' + k], rtol=2e-5, atol=2e-5, equal_nan=True, err_msg=k)
    assert _rel(tensors['image_pred'].double().sum(), g['tensor_image_pred_sum']) < 1e-5
    np.testing.assert_allclose(tensors['image_pred'][:1, :1].numpy(), g['tensor_image_pred_frame'], rtol=0, atol=2e-5)
    dt = ex['dream_tensors']
    for k in [f[6:] for f in g.files if f.startswith('dream_') and not f.startswith('dream_image_pred')]:
        np.testing.assert_allclose(dt[k].numpy(), g['dream_' + k], rtol=2e-5, atol=2e-5, err_msg=k)
    assert _rel(dt['image_pred'].double().sum(), g['dream_image_pred_sum']) < 1e-5
    np.testing.assert_allclose(dt['image_pred'][-1:, :1].numpy(), g['dream_image_pred_frame'], rtol=0, atol=2e-5)
