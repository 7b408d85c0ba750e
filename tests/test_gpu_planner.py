"""-m gpu: latent-space planning end to end - CEMPlanner, PlannerPolicy and the trainer's eval_behavior='plan' on the
tiny configuration (deter 64, action_dim 6) with closed-form parameters and explicit noise: a discrete model and a tanh_normal one
with Gaussian latents (stoch_discrete = 0).

  1 the candidates' imagined features are, bit for bit, WorldModel.training_step(do_open_loop=True) on the same start states,
    actions and noise; ret is the float64 return of the heads' outputs within dm_cem_update's bound (4 Hp + 3) u sum |terms|
  2 the executed action is the first action of the candidate with the largest ret, the lower index winning a tie
  3 over three iterations every iteration keeps best return >= mean elite return >= mean return (what the selection rule
     implies; the latents are re-drawn every iteration, so the elite mean itself need not rise - it is printed)
  4 an environment planned in a batch of three has the bits of the same environment planned alone
  5 PlannerPolicy in collect(): the episode files' policy columns are plan()'s stats, call by call; batch_size = 1 gives (A,)
  6 train.run with eval_behavior='plan' logs agent_eval/return"""
import os
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import dreamer_oracle as O
from pydreamer_amd import config, replay as R
from tests import closed_form_params as CFP
from tests.test_collect_cpu import _closed_in_order

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
B, J, K, HP = 3, 8, 2, 3


def _model(which):
    from pydreamer_amd.models import Dreamer
    oconf = O.tiny_conf()
    if which == 'discrete':
        conf = config.load_config('defaults', 'atari', **vars(oconf))
        params = O.make_params(oconf, seed=0)
    else:
        conf = config.load_config('defaults', 'atari', **{**vars(oconf), 'actor_dist': 'tanh_normal', 'stoch_discrete': 0})
        with torch.device('meta'):
            shapes = {k: tuple(v.shape) for k, v in Dreamer(conf).state_dict().items()}
        params = CFP.make_params(shapes, seed=0)
    model = Dreamer(conf)
    model.load_state_dict(params, strict=True)
    return model.to(DEV)


@pytest.fixture(scope='module', params=['discrete', 'tanh_normal_gauss'])
def model(request):
    return _model(request.param)


def _start(model, n, seed):
    """(n, F) feature rows [h|z]: h in (-1, 1) as a GRU state is, z one-hot per latent or a Normal draw."""
    c = model.conf
    gen = torch.Generator().manual_seed(seed)
    h = torch.tanh(torch.randn(n, c.deter_dim, generator=gen))
    if c.stoch_discrete:
        z = torch.nn.functional.one_hot(torch.randint(0, c.stoch_discrete, (n, c.stoch_dim), generator=gen), c.stoch_discrete).float()
        z = z.view(n, -1)
    else:
        z = torch.randn(n, c.stoch_dim, generator=gen)
    return torch.cat((h, z), -1).to(DEV).contiguous()


def _noise(model, planner, n, seed):
    c, kind = model.conf, model.ac.dist_kind
    gen = torch.Generator().manual_seed(seed)
    it, Hp, M, A, S = planner.iters, planner.horizon, n * planner.candidates, c.action_dim, c.stoch_dim
    u_cand = torch.rand(it, Hp, M, generator=gen) if kind == 0 else torch.randn(it, Hp, M, A, generator=gen)
    u_prior = torch.rand(it, Hp, M, S, generator=gen) if c.stoch_discrete else torch.randn(it, Hp, M, S, generator=gen)
    return dict(u_cand=u_cand.to(DEV), u_prior=u_prior.to(DEV))


def _planner(model, **kw):
    from pydreamer_amd.planner import CEMPlanner
    return CEMPlanner(model, **{**dict(horizon=HP, candidates=J, elites=K, iters=1, alpha=0.0, floor=0.05), **kw})


def test_rollout_is_the_open_loop_chain_and_ret_is_the_return(hip, model):
    c = model.conf
    planner = _planner(model)
    feat, noise = _start(model, B, 1), _noise(model, planner, B, 2)
    res = planner.plan(feat, noise, keep_rollout=True)
    roll, M, A, D_ = res['rollout'], B * J, c.action_dim, c.deter_dim
    # 1 the same chain through the tested evaluation path: an environment's J candidates as a batch of J columns, T = Hp, no
    #   resets (the planner launches every environment alone, so the comparison does too)
    for b in range(B):
        cols = slice(b * J, (b + 1) * J)
        start = feat[b:b + 1].repeat_interleave(J, dim=0)
        obs = dict(action=roll['actions'][:, cols].contiguous(), reset=torch.zeros(HP, J, dtype=torch.bool, device=DEV),
                   reward=torch.zeros(HP, J, device=DEV), terminal=torch.zeros(HP, J, device=DEV),
                   image=torch.zeros(HP, J, c.image_channels, c.image_size, c.image_size, device=DEV))
        with torch.no_grad():
            _, features, _, _, _, _ = model.wm.training_step(obs, (start[:, :D_].contiguous(), start[:, D_:].contiguous()),
                                                             do_open_loop=True, u_post=noise['u_prior'][0][:, cols].contiguous())
        assert torch.equal(features.reshape(HP, J, -1), roll['features'][:, cols]), f'environment {b}: the planner rolled out another chain'
    if model.ac.dist_kind == 0:
        assert bool((roll['actions'].sum(-1) == 1).all()) and bool((roll['actions'].max(-1).values == 1).all())
    else:
        assert float(roll['actions'].abs().max()) <= 1.0
    # ret against float64 on the heads' fp32 outputs, dm_cem_update's stated order: (4 Hp + 3) u sum |terms|
    g = float(np.float32(model.ac.gamma))
    r, tm, v = (roll[k].double().cpu().numpy() for k in ('reward', 'terminal', 'value'))
    w, ret64, mag = np.ones(M), np.zeros(M), np.zeros(M)
    for t in range(HP):
        term = g ** t * w * r[t]
        ret64, mag, w = ret64 + term, mag + np.abs(term), w * (1 - tm[t])
    term = g ** HP * w * v
    ret64, mag = ret64 + term, mag + np.abs(term)
    ret = res['ret'].cpu().numpy()
    err, tol = np.abs(ret - ret64), (4 * HP + 3) * U * mag
    print(f'[tol] ret: max err {err.max():.3e}, worst err/tol {(err / tol).max():.3f}')
    assert (err <= tol).all() and float(np.abs(r).max()) > 0 and (tm > 0).all() and (tm < 1).all()
    # 2 the executed action: the first action of the best candidate, the lower index winning a tie
    key = np.where(np.isfinite(ret), ret, -np.finfo(np.float32).max).reshape(B, J)
    order = np.stack([np.lexsort((np.arange(J), -key[b].astype(np.float64))) for b in range(B)])
    assert np.array_equal(res['elite'].cpu().numpy(), order[:, :K])
    rows = torch.from_numpy(order[:, 0] + np.arange(B) * J).to(DEV)
    assert torch.equal(res['action'], roll['actions'][0, rows])
    st = res['stats'].cpu().numpy()
    assert np.array_equal(st[:, 0], np.take_along_axis(key, order[:, :1], 1)[:, 0].astype(np.float32))
    # the same call again: the same bits
    again = planner.plan(feat, noise)
    for k in ('action', 'stats', 'prop', 'ret', 'elite'):
        assert torch.equal(res[k], again[k]), k


def test_without_the_value_the_return_stops_at_the_horizon(hip, model):
    planner = _planner(model, use_value=False)
    feat, noise = _start(model, B, 1), _noise(model, planner, B, 2)
    res = planner.plan(feat, noise, keep_rollout=True)
    roll = res['rollout']
    assert roll['value'] is None
    g = float(np.float32(model.ac.gamma))
    r, tm = (roll[k].double().cpu().numpy() for k in ('reward', 'terminal'))
    w, ret64, mag = np.ones(B * J), np.zeros(B * J), np.zeros(B * J)
    for t in range(HP):
        term = g ** t * w * r[t]
        ret64, mag, w = ret64 + term, mag + np.abs(term), w * (1 - tm[t])
    assert (np.abs(res['ret'].cpu().numpy() - ret64) <= (4 * HP + 3) * U * mag).all()


def test_iterations_keep_the_order_of_the_three_means(hip, model):
    """best return >= mean elite return >= mean return in every iteration: the elites are the K largest returns.  The elites of
    iteration n seed iteration n + 1, but its latents are drawn anew, so a rising elite mean is likely, not implied: printed."""
    planner = _planner(model, iters=3, candidates=64, elites=8)
    feat = _start(model, B, 3)
    for seed in (0, 1, 2):
        res = planner.plan(feat, _noise(model, planner, B, 10 + seed), keep_iterations=True)
        for n, (stats, ret) in enumerate(res['iterations']):
            st, mean = stats.cpu().numpy(), ret.view(B, -1).double().mean(1).cpu().numpy()
            print(f'[iter] seed {seed} iteration {n + 1}: best {st[:, 0]}, mean elite {st[:, 1]}, mean {mean}')
            assert (st[:, 0] >= st[:, 1]).all() and (st[:, 1] >= mean - 64 * U * np.abs(mean)).all()
        assert torch.equal(res['iterations'][-1][0], res['stats']) and torch.equal(res['iterations'][-1][1], res['ret'])
        prop = res['prop']
        if model.ac.dist_kind == 0:      # a proposal stays a distribution with the floor's share on every class
            assert bool((prop >= 0.05 / model.conf.action_dim * (1 - 8 * U)).all())
            assert float((prop.sum(-1) - 1).abs().max()) <= 16 * U
        else:
            assert bool((prop[..., model.conf.action_dim:] >= 0.05).all())


def test_an_environment_plans_the_same_alone_and_in_a_batch(hip, model):
    """plan() on B environments gives every environment, bit for bit, what plan() gives for it alone with its rows of the noise: the
    result does not depend on how the environments are grouped into launches."""
    planner = _planner(model, iters=2)
    feat, noise = _start(model, B, 4), _noise(model, planner, B, 5)
    whole = planner.plan(feat, noise, keep_iterations=True)
    for b in range(B):
        cols = slice(b * J, (b + 1) * J)
        alone = planner.plan(feat[b:b + 1], {k: v[:, :, cols].contiguous() for k, v in noise.items()}, keep_iterations=True)
        for k in ('action', 'stats', 'prop', 'elite'):
            assert torch.equal(whole[k][b:b + 1], alone[k]), (b, k)
        assert torch.equal(whole['ret'][cols], alone['ret']), b
        for (s0, r0), (s1, r1) in zip(whole['iterations'], alone['iterations']):
            assert torch.equal(s0[b:b + 1], s1) and torch.equal(r0[cols], r1), b


def test_planner_policy_in_collect(hip, tmp_path):
    from pydreamer_amd.collect import EpisodeRecorder, collect
    from pydreamer_amd.planner import PlannerPolicy
    from pydreamer_amd.policy import METRIC_KEYS, StepPreprocessor
    from tests.test_gpu_collect import ToyEnv
    model = _model('discrete')
    c = model.conf
    A, steps = c.action_dim, 14
    envs = [ToyEnv(b, lengths, A, frame=(64, 64, c.image_channels)) for b, lengths in enumerate([[4, 6], [7, 5], [5, 4, 6]])]
    repo = R.LocalEpisodeRepository(str(tmp_path))
    prep = StepPreprocessor(A, clip_rewards='tanh', image_key='image', batched=True)
    policy = PlannerPolicy(model, prep, batch_size=B, per_env=True, horizon=HP, candidates=J, elites=K, iters=2, floor=0.05)
    calls, real = [], policy.planner.plan
    policy.planner.plan = lambda feat, noise=None: (lambda res: (calls.append(res['stats'].cpu().numpy().astype(np.float64)), res)[1])(
        real(feat, noise))
    torch.manual_seed(3)
    out = collect(envs, policy, EpisodeRecorder(repo, B, steps_per_npz=10 ** 6), steps)
    order = _closed_in_order(envs)
    assert out['steps'] == B * steps and len(calls) == steps and out['episodes'] == len(order) >= 5 and len(out['files']) == 1
    want = {k: [] for k in METRIC_KEYS}
    for i, e in order:      # the call at environment step s chose the action of the episode's row s - start + 1
        L, s0 = len(envs[i].episodes[e]) - 1, envs[i].starts[e]
        col = lambda j: [calls[s0 + n][i, j] for n in range(L)]
        want['policy_value'] += col(0) + [np.nan]
        want['policy_entropy'] += col(2) + [np.nan]
        want['action_prob'] += [np.nan] + col(3)
    with np.load(out['files'][0]) as f:
        for k in METRIC_KEYS:
            assert np.array_equal(f[k], np.array(want[k]), equal_nan=True), k
        prob = f['action_prob'][~np.isnan(f['action_prob'])]
        assert (prob >= 0.05 / A * (1 - 8 * U)).all() and (prob <= 1).all()
    # the scalar protocol: batch_size = 1 returns an (A,) action and three Python floats; reset_state is NetworkPolicy's
    one = PlannerPolicy(model, StepPreprocessor(A, clip_rewards='tanh', image_key='image'), batch_size=1, horizon=HP, candidates=J,
                        elites=K, iters=1)
    env = ToyEnv(0, [4], A, frame=(64, 64, c.image_channels))
    action, metrics = one(env.reset())
    assert action.shape == (A,) and action.dtype == np.float32 and action.sum() == 1.0
    assert sorted(metrics) == sorted(METRIC_KEYS) and all(type(v) is float and np.isfinite(v) for v in metrics.values())
    one.reset_state()
    assert all(float(s.abs().max()) == 0 for s in one.state)


def test_act_returns_dreamer_acts_shapes(hip, model):
    c = model.conf
    planner = _planner(model, iters=2)
    A = c.action_dim
    obs = dict(action=torch.zeros(1, B, A, device=DEV), reset=torch.ones(1, B, dtype=torch.bool, device=DEV),
               reward=torch.zeros(1, B, device=DEV), terminal=torch.zeros(1, B, device=DEV),
               image=torch.rand(1, B, c.image_channels, 64, 64, device=DEV) - 0.5)
    state = tuple(s.to(DEV) for s in model.init_state(B))
    action, out_state, metrics = planner.act(obs, state, return_rows=True)
    assert action.shape == (1, B, A) and [tuple(s.shape) for s in out_state] == [tuple(s.shape) for s in state]
    assert all(metrics[k].dim() == 0 for k in ('policy_value', 'action_prob', 'policy_entropy'))
    assert all(tuple(metrics[k].shape) == (B,) for k in ('value', 'log_prob', 'entropy'))
    assert float(metrics['policy_value']) == pytest.approx(float(metrics['value'].mean()), rel=1e-6)
    if model.ac.dist_kind == 0:
        assert torch.allclose(metrics['log_prob'].exp().mean(), metrics['action_prob'], rtol=1e-6)
    else:
        assert float(metrics['log_prob'].abs().max()) == 0 and float(metrics['action_prob']) == 0


def test_the_trainer_evaluates_by_planning(hip, tmp_path):
    from pydreamer_amd.train import run
    from tests.test_gpu_train_loop import LoopEnv, _loop_conf
    conf = _loop_conf()
    conf = Namespace(**{**vars(conf), **dict(n_steps=2, log_interval=2, save_interval=2, eval_interval=2, eval_behavior='plan',
                                             plan_candidates=8, plan_elites=2, plan_iters=2, plan_horizon=3)})
    data_dir, eval_dir, logdir = (str(tmp_path / d) for d in ('episodes', 'eval_episodes', 'log'))
    os.makedirs(data_dir), os.makedirs(eval_dir)
    repo, eval_repo = R.LocalEpisodeRepository(data_dir), R.LocalEpisodeRepository(eval_dir)
    mk = lambda: [LoopEnv(b, lengths, conf.action_dim, conf.vecobs_size) for b, lengths in enumerate([[11, 12], [12, 10], [13, 11, 10]])]
    logged = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        steps = run(conf, repo, test_repository=repo, eval_repository=eval_repo, envs=mk(), eval_envs=mk(), eval_episodes=3,
                    logdir=logdir, logger=lambda m, s: logged.append((s, dict(m))), env_steps_per_grad_step=3, seed=1, steps_per_npz=10)
    assert not [str(w.message) for w in caught if 'Evaluation failed' in str(w.message)]
    assert steps == 2
    entries = [m for s, m in logged if 'agent_eval/return' in m]
    assert len(entries) == 1 and np.isfinite(entries[0]['agent_eval/return'])
    assert {'agent_eval/policy_value', 'agent_eval/action_prob', 'agent_eval/policy_entropy'} <= set(entries[0])
    assert eval_repo.count_steps()[2] >= 3
