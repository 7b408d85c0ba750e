"""Config surface of the hot path: the keys of pydreamer's `config/defaults.yaml` that Dreamer / WorldModel /
ActorCritic read (reference: dreamer.py:23-58,237-277; encoders.py:14-36; decoders.py:14-46; launch.py:16-41).

`load_config('defaults', 'atari', batch_size=50)` mirrors `launch.py --configs defaults atari --batch_size 50`:
named sections are merged in order, then overrides, giving an `argparse.Namespace` the modules read by attribute.
A user-supplied YAML with the same flat section->key layout can be merged with `yaml_path=`.
"""
from argparse import Namespace

SECTIONS = {
    'defaults': dict(
        # features
        image_key='image', image_size=64, image_channels=3, image_categorical=False, action_dim=0, clip_rewards=None,
        # training
        reset_interval=200, iwae_samples=1, kl_balance=0.8, kl_weight=1.0, image_weight=1.0, vecobs_weight=1.0,
        reward_weight=1.0, terminal_weight=1.0, adam_lr=3.0e-4, adam_lr_actor=1.0e-4, adam_lr_critic=1.0e-4,
        adam_eps=1.0e-5, keep_state=True, batch_length=48, batch_size=32, device='cuda:0', grad_clip=200,
        grad_clip_ac=200, image_decoder_min_prob=0, amp=False, probe_gradients=False,
        # model
        model='dreamer', deter_dim=2048, stoch_dim=32, stoch_discrete=32, hidden_dim=1000, gru_layers=1, gru_type='gru',
        layer_norm=True, vecobs_size=0, image_encoder='cnn', cnn_depth=48, image_encoder_layers=0, image_decoder='cnn',
        image_decoder_layers=0, reward_input=False, reward_decoder_layers=4, reward_decoder_categorical=None,
        terminal_decoder_layers=4,
        # probe
        probe_model='none', map_key=None, map_size=0, map_channels=0, map_categorical=True, goals_size=0, map_decoder='dense',
        map_hidden_layers=4, map_hidden_dim=1024,
        # actor critic
        gamma=0.995, lambda_gae=0.95, entropy=0.003, target_interval=100, imag_horizon=15, actor_grad='reinforce',
        actor_dist='onehot',
        # the two-hot symlog critic and the percentile return normalisation (DreamerV3's; no reference counterpart).
        # Inert unless critic_dist='twohot' / return_norm='percentile': critic_bins symlog-spaced bins over +-critic_bin_range,
        # advantages divided by max(return_norm_limit, running [lo, hi] percentile range of the imagined returns)
        critic_dist='mse', critic_bins=255, critic_bin_range=20.0, return_norm='none', return_norm_lo=0.05, return_norm_hi=0.95,
        return_norm_decay=0.99, return_norm_limit=1.0,
        # the world model's share of the same (DreamerV3's; no reference counterpart).  Inert by default.  kl_free: free
        # bits per (t, b) row in nats - max(kl_free, KL) enters loss_model and a row with KL <= kl_free sends no gradient into the
        # posterior or the prior; 0 = off; not with iwae_samples > 1.  reward_dist='twohot': the reward head predicts
        # reward_twohot_bins symlog-spaced bins over +-reward_twohot_range (two-hot cross-entropy against symlog(reward), mean decoded by
        # symexp) instead of a unit-variance Normal: its loss does not grow with the reward scale; not with reward_decoder_categorical
        kl_free=0.0, reward_dist='normal', reward_twohot_bins=255, reward_twohot_range=20.0,
        # aux critic
        aux_critic=False, aux_critic_weight=1.0, gamma_aux=0.99, lambda_gae_aux=0.95, target_interval_aux=1000,
        # the trainer loop (train.py; defaults.yaml:3-16, 34-35, 59-65, 113-118)
        n_steps=100_000_000, n_env_steps=1_000_000_000, offline_data_dir=None, offline_prefill_dir=None, offline_test_dir=None,
        offline_eval_dir=None, log_interval=100, logbatch_interval=1000, save_interval=500, eval_interval=2000,
        allow_mid_reset=True, buffer_size=10_000_000, buffer_size_offline=0, test_batches=61, test_batch_size=10,
        test_save_size=1, eval_batches=61, eval_samples=1, eval_batch_size=32, eval_save_size=1,
        generator_prefill_steps=50_000, limit_step_ratio=0, env_action_repeat=1,
        # the environment wrappers (envs.wrap_envs; defaults.yaml:119-120)
        env_time_limit=0, env_no_terminal=False,
        # Plan2Explore (explore.py; DreamerV2's expl_behavior / disag_* / expl_* keys - no reference counterpart).  Inert unless
        # expl_behavior='plan2explore'; expl_until counts collected environment steps, 0 = explore for the whole run
        expl_behavior='greedy', disag_models=10, disag_action_cond=True, expl_intr_scale=1.0, expl_extr_scale=0.0, expl_until=0,
        adam_lr_expl=3.0e-4,
        # latent-space planning (planner.py; PlaNet's CEM sizes - no reference counterpart).  Inert unless eval_behavior='plan':
        # then the trainer's evaluation episodes act by planning instead of with the actor.  plan_floor: the uniform-mix share of
        # a one-hot proposal, the minimum std of a continuous one; plan_value: the critic closes the planned return
        plan_horizon=12, plan_candidates=1000, plan_elites=100, plan_iters=10, plan_alpha=0.0, plan_floor=0.01, plan_value=True,
        eval_behavior='actor',
    ),
    'atari': dict(action_dim=18, clip_rewards='tanh', deter_dim=1024, kl_weight=0.1, gamma=0.99, entropy=0.001),
    'dmc': dict(action_dim=12, entropy=1.0e-4, actor_grad='dynamics', actor_dist='tanh_normal', clip_rewards='tanh'),
    # defaults.yaml:143-161, the keys the hot path reads.  probe_model stays 'none' here, NOT the reference's 'goals': the goals
    # probe needs goals_size >= 1, which the environment sets.  probe_model='goals' / 'map+goals' (with goals_size) and 'map' (the
    # map keys below) are all available
    'miniworld': dict(action_dim=3, image_key='image', image_size=64, image_channels=3, image_categorical=False,
                      reward_input=True, probe_model='none', cnn_depth=32, map_key='map', map_size=9, map_channels=14),
    # defaults.yaml:122-141, the keys the hot path reads: the dense categorical image path (models.dense_image_gate) with the
    # map probe.  The class image reaches the model as replay.preprocess_batch(image_categorical=image_channels) makes it
    'minigrid': dict(image_key='image', image_size=7, image_channels=4, image_categorical=True, map_key='map', map_size=11,
                     map_channels=4, map_categorical=True, action_dim=7, reward_input=True, image_encoder='dense',
                     image_encoder_layers=3, image_decoder='dense', image_decoder_layers=2, probe_model='map', imag_horizon=1),
    # defaults.yaml:236-242: no image at all - the vector observation is the only input (models.imageless_gate)
    'vectorenv': dict(action_dim=2, vecobs_size=4, image_key=None, image_encoder=None, image_decoder=None),
    'minecraft': dict(action_dim=29, vecobs_size=27, clip_rewards='log1p'),      # defaults.yaml:244-248
    'debug': dict(device='cpu', batch_length=15, batch_size=5, imag_horizon=3),
}


def load_config(*sections, yaml_path=None, **overrides):
    tables = {k: dict(v) for k, v in SECTIONS.items()}
    if yaml_path is not None:
        import yaml
        with open(yaml_path) as f:
            for name, table in (yaml.safe_load(f) or {}).items():
                tables.setdefault(name, {}).update(table or {})
    conf = {}
    for s in sections or ('defaults',):
        if s not in tables:
            raise KeyError(f'unknown config section {s!r}; known: {sorted(tables)}')
        conf.update(tables[s])
    unknown = [k for k in overrides if k not in conf]
    if unknown:
        raise KeyError(f'unknown config keys {unknown}')
    conf.update(overrides)
    return Namespace(**conf)


def atari_literal(**overrides):
    """BASELINE.json configs[1]: Atari defaults at B=50, T=50, H=15, deter=600, stoch 32x32."""
    base = dict(batch_size=50, batch_length=50, deter_dim=600, action_dim=18)
    base.update(overrides)
    return load_config('defaults', 'atari', **base)
