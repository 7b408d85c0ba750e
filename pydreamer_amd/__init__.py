"""pydreamer_amd — MI355X-native DreamerV2 gradient step (hand-written HIP behind pydreamer's module API)."""
__version__ = '0.1.0'


def __getattr__(name):      # `from pydreamer_amd import NetworkPolicy` without importing torch for `import pydreamer_amd` alone
    if name in ('NetworkPolicy', 'RandomPolicy', 'StepPreprocessor'):
        from . import policy
        return getattr(policy, name)
    if name in ('CEMPlanner', 'PlannerPolicy'):
        from . import planner
        return getattr(planner, name)
    if name in ('EpisodeRecorder', 'EpisodeStats'):      # (the loop itself is pydreamer_amd.collect.collect: the name is the submodule's)
        from . import collect
        return getattr(collect, name)
    if name in ('wrap_env', 'wrap_envs'):
        from . import envs
        return getattr(envs, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
