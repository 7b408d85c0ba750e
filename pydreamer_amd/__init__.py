"""pydreamer_amd — MI355X-native DreamerV2 gradient step (hand-written HIP behind pydreamer's module API)."""
__version__ = '0.1.0'


def __getattr__(name):      # `from pydreamer_amd import NetworkPolicy` without importing torch for `import pydreamer_amd` alone
    if name in ('NetworkPolicy', 'StepPreprocessor'):
        from . import policy
        return getattr(policy, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
