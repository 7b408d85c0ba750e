"""CPU (-m "not gpu"): the host side of the categorical reward decoder (reward_decoder_categorical): the entry
dm_head_loss_catsup and its host-side argument checks, the config surface and the parameter tree against the reference-written
fixtures (scripts/gen_reward_categorical_golden.py), what is refused, and this file's own fp64 restatement of the decoder
(bin / loss / mean / per-bucket masks) against the fixtures' recorded logits - which pins the reference the GPU tests use
(tests/test_gpu_reward_categorical.py imports `restate` from here) to the real one."""
import ast
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_form_params as CFP                     # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402
from pydreamer_amd import config, hip                # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
DM_E_SHAPE, DM_E_NULL = -1, -5
SUPPORT_KEY = 'wm.decoder.reward._support'
VEC_FIXTURES = ['tiny_reward_categorical', 'tiny_reward_categorical_iwae', 'tiny_reward_categorical_eval',
                'tiny_reward_categorical_open_loop', 'tiny_reward_categorical_amp']
ALL_FIXTURES = VEC_FIXTURES + ['tiny_reward_categorical_image_eval']


def fixture_conf(g, **more):
    oconf = O.make_conf(**dict(ast.literal_eval(str(g['conf_json']))))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    sections = ('defaults', 'vectorenv') if extra['image_decoder'] is None else ('defaults',)
    return oconf, config.load_config(*sections, **{**vars(oconf), **extra, **more})


def fixture_params(g):
    """The closed-form weights of the recorded names and shapes, with `_support` - excluded from the fill - as recorded."""
    params = CFP.make_params(CFP.shapes_of_fixture(g), seed=0)
    params[SUPPORT_KEY] = torch.from_numpy(g['support'])
    return params


def bins_fp32(target, support):
    """decoders.py:344-347 as the reference computes it: fp32, on the CPU, the first minimum wins."""
    t, s = torch.as_tensor(target, dtype=torch.float32).cpu(), torch.as_tensor(support, dtype=torch.float32).cpu()
    return torch.square(t.unsqueeze(-1) - s).argmin(-1)


def restate(logits, support, target, I=1):
    """fp64 restatement of DenseCategoricalSupportDecoder: logits (rows, K), target (rows / I).  Returns per-row loss, softmax,
    mean and the (rows / I) bins; the bins are the fp32 rule (they are integers: there is nothing to refine)."""
    x, s = torch.as_tensor(logits).double().cpu(), torch.as_tensor(support, dtype=torch.float32).cpu()
    b = bins_fp32(target, s).reshape(-1)
    br = b.repeat_interleave(I)
    lse = torch.logsumexp(x, -1)
    p = torch.softmax(x, -1)
    return lse - x.gather(-1, br[:, None])[:, 0], p, p @ s.double(), b


def _rc(name, *args):
    return getattr(hip.lib(), name)(*args)


def test_entry_is_exported_and_checks_its_arguments_on_the_host():
    """Nothing is launched: every pointer is NULL or a placeholder that a launch would fault on."""
    lib = hip.lib()
    assert 'dm_head_loss_catsup' in hip.exported_symbols() and hasattr(lib, 'dm_head_loss_catsup')
    P = 64
    call = lambda rows, I, K, ld, logits=P, sup=P, tgt=P, loss=P, dl=P, mean=P, b=P: _rc(
        'dm_head_loss_catsup', rows, I, K, logits, ld, sup, tgt, 1.0, loss, dl, mean, b, None)
    for rows, I, K, ld in ((8, 1, 1, 4), (8, 1, 33, 33), (8, 1, 4, 3), (9, 2, 4, 4), (8, 0, 4, 4), (-1, 1, 4, 4)):
        assert call(rows, I, K, ld) == DM_E_SHAPE, (rows, I, K, ld)
        # ... and with NULL pointers throughout: the sizes are refused before any pointer is looked at
        assert call(rows, I, K, ld, None, None, None, None, None, None, None) == DM_E_SHAPE, (rows, I, K, ld)
    assert call(8, 1, 4, 3) == DM_E_SHAPE and 'ld=3' in lib.dm_last_error().decode()
    assert call(8, 1, 4, 4, logits=None) == DM_E_NULL
    assert call(8, 1, 4, 4, sup=None) == DM_E_NULL
    # target == NULL is the mean-only form: loss, dlogits and bin must be NULL too
    assert call(8, 1, 4, 4, tgt=None, dl=None, b=None) == DM_E_NULL
    assert call(8, 1, 4, 4, tgt=None, loss=None, b=None) == DM_E_NULL
    assert call(8, 1, 4, 4, tgt=None, loss=None, dl=None) == DM_E_NULL
    assert 'mean-only' in lib.dm_last_error().decode()
    with pytest.raises(hip.DreamerHipError):
        hip.call('dm_head_loss_catsup', 8, 1, 33, P, 33, P, P, 1.0, P, P, P, P, None)
    assert call(0, 1, 4, 4) == 0      # zero rows: nothing to do, nothing launched


def test_config_key_parses_as_a_list(tmp_path):
    assert config.load_config('defaults').reward_decoder_categorical is None
    c = config.load_config('defaults', 'atari', reward_decoder_categorical=[-10, 0, 1, 10])
    assert c.reward_decoder_categorical == [-10, 0, 1, 10]
    y = tmp_path / 'user.yaml'
    y.write_text('sparse:\n  reward_decoder_categorical: [-10, 0, 1, 10]\n  clip_rewards: log1p\n')
    try:
        import yaml  # noqa: F401
    except ImportError:
        return
    c = config.load_config('defaults', 'sparse', yaml_path=str(y))
    assert c.reward_decoder_categorical == [-10, 0, 1, 10] and c.clip_rewards == 'log1p'


@pytest.mark.parametrize('name', ALL_FIXTURES)
def test_state_dict_and_support_match_the_reference(name):
    from pydreamer_amd.models import DenseCategoricalSupportDecoder, Dreamer
    g = np.load(os.path.join(GOLD, name + '.npz'))
    oconf, conf = fixture_conf(g)
    assert isinstance(conf.reward_decoder_categorical, list)
    torch.manual_seed(0)
    model = Dreamer(conf)      # on the CPU: the parameter tree needs no device
    head = model.wm.decoder.reward
    assert isinstance(head, DenseCategoricalSupportDecoder) and model.wm.decoder.reward_bins == len(g['support'])
    want = CFP.shapes_of_fixture(g)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert list(got.items()) == list(want.items())
    keys = list(got)
    assert keys.index(SUPPORT_KEY) + 1 == keys.index('wm.decoder.reward.model.model.0.weight')
    # the clipped support, bit for bit, and frozen; the MLP ends in K outputs with no Flatten slot behind it
    assert head._support.dtype == torch.float32 and not head._support.requires_grad
    assert np.array_equal(head._support.detach().numpy(), g['support'])
    assert tuple(head.model.model[3 * conf.reward_decoder_layers].weight.shape) == (len(g['support']), 400)
    # the optimizer's parameter numbering is the reference's: `_support` is IN the world-model group (and never gets a gradient)
    wm = model.param_groups()['wm']
    assert any(p is head._support for p in wm)
    if 'wm_param_count' in g.files:
        assert len(wm) == int(g['wm_param_count'])
    model.load_state_dict(fixture_params(g), strict=True)
    assert np.array_equal(head._support.detach().numpy(), g['support'])


def test_support_is_clipped_as_the_reference_clips_it():
    from pydreamer_amd.models import reward_support
    ns = lambda **kw: config.load_config('defaults', **kw)
    assert reward_support(ns()) is None and reward_support(ns(reward_decoder_categorical=[])) is None
    raw = [-10, 0, 1, 10]
    assert np.array_equal(reward_support(ns(reward_decoder_categorical=raw)), np.array(raw, dtype=np.float64))
    assert np.array_equal(reward_support(ns(reward_decoder_categorical=raw, clip_rewards='tanh')), np.tanh(np.array(raw, dtype=np.float64)))
    assert np.array_equal(reward_support(ns(reward_decoder_categorical=[0, 1, 10], clip_rewards='log1p')), np.log1p([0.0, 1.0, 10.0]))
    g = np.load(os.path.join(GOLD, 'tiny_reward_categorical_iwae.npz'))
    extra = dict(ast.literal_eval(str(g['extra_conf_json'])))
    assert extra['clip_rewards'] == 'tanh' and len(g['support']) == 3
    got = reward_support(ns(reward_decoder_categorical=extra['reward_decoder_categorical'], clip_rewards='tanh'))
    assert np.array_equal(torch.tensor(got).to(torch.float).numpy(), g['support'])


@pytest.mark.parametrize('kw,exc', [
    (dict(reward_decoder_categorical=[1.0]), ValueError),
    (dict(reward_decoder_categorical=[-2, 0, 1], clip_rewards='log1p'), ValueError),      # log1p(-2) is NaN
    (dict(reward_decoder_categorical=[-1, 0, 1], clip_rewards='log1p'), ValueError),      # log1p(-1) is -inf
    (dict(reward_decoder_categorical=[0.0, float('inf')]), ValueError),
    (dict(reward_decoder_categorical=[float(i) for i in range(33)]), NotImplementedError),
], ids=lambda v: v.__name__ if isinstance(v, type) else ','.join(f'{k}={x}' for k, x in v.items())[:60])
def test_refused_supports(kw, exc):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'), pytest.raises(exc):
        Dreamer(config.load_config('defaults', 'atari', **{'clip_rewards': None, **kw}))


TINY = dict(deter_dim=64, hidden_dim=64, stoch_dim=8, stoch_discrete=8, batch_length=5, batch_size=3, imag_horizon=4)


def test_thirty_two_values_and_the_other_gates_construct():
    """On the CPU at tiny sizes: the decoder is not built on the meta device (next test)."""
    from pydreamer_amd.models import Dreamer
    m = Dreamer(config.load_config('defaults', 'atari', **TINY, reward_decoder_categorical=[float(i) for i in range(32)], clip_rewards=None))
    assert m.wm.decoder.reward_bins == 32 and m.wm.decoder.reward._support.tolist() == [float(i) for i in range(32)]
    m = Dreamer(config.load_config('defaults', 'minigrid', **TINY, reward_decoder_categorical=[-1, 0, 1]))      # the dense image gate
    assert m.wm.dense and m.wm.decoder.reward_bins == 3
    m = Dreamer(config.load_config('defaults', 'atari', **TINY, reward_decoder_categorical=[-1, 0, 1], reward_input=True, cnn_depth=8,
                                   vecobs_size=5, aux_critic=True, amp=True))
    assert m.wm.decoder.reward_bins == 3 and m.wm.decoder.reward.model.precision == 1
    with torch.device('meta'):      # the Normal head holds no values: meta construction is as before
        m = Dreamer(config.load_config('defaults', 'atari'))
    assert m.wm.decoder.reward_bins == 0 and SUPPORT_KEY not in m.state_dict()


def test_meta_device_is_refused_because_the_support_would_be_lost():
    """`_support` holds values fixed at construction; a meta tensor drops them and no initialiser restores them."""
    from pydreamer_amd.models import Dreamer
    for section in ('atari', 'minigrid', 'vectorenv'):
        with torch.device('meta'), pytest.raises(NotImplementedError, match='meta'):
            Dreamer(config.load_config('defaults', section, **TINY, reward_decoder_categorical=[-1, 0, 1]))


# ------------------------------------------------------------------------------------------------ the restatement against the fixtures
def _check_restatement(g, pre, logits_key, loss_key, mean_key, I):
    sup, reward = g['support'], g[pre + 'in_reward']
    T, B = reward.shape
    x = torch.from_numpy(g[logits_key]).reshape(T * B * I, len(sup))
    loss, p, mean, b = restate(x, sup, reward, I)
    loss_tb = -(torch.logsumexp(-loss.view(T * B, I), -1) - np.log(I))      # -logavgexp(-loss_tbi) (decoders.py:356)
    mean_tb = mean.view(T * B, I).mean(-1)
    np.testing.assert_allclose(loss_tb.view(T, B).numpy(), g[loss_key], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(mean_tb.view(T, B).numpy(), g[mean_key], rtol=1e-5, atol=2e-6)
    return loss_tb.view(T, B), b.view(T, B)


@pytest.mark.parametrize('name,steps,I', [('tiny_reward_categorical', 2, 1), ('tiny_reward_categorical_iwae', 1, 2)])
def test_restatement_reproduces_the_training_fixtures(name, steps, I):
    g = np.load(os.path.join(GOLD, name + '.npz'))
    for s in range(steps):
        pre = f's{s}_'
        loss_tb, b = _check_restatement(g, pre, pre + 'aux_reward_logits', pre + 'tensor_loss_reward', pre + 'tensor_reward_rec', I)
        assert abs(float(loss_tb.mean()) - float(g[pre + 'metric_loss_reward'])) < 1e-5
        assert set(b.flatten().tolist()) == set(range(len(g['support']))), 'the training fixtures hit every bucket'
        assert not [k for k in g.files if 'logprob_reward' in k]


@pytest.mark.parametrize('name,skip', [('tiny_reward_categorical_eval', 2), ('tiny_reward_categorical_open_loop', 2),
                                       ('tiny_reward_categorical_image_eval', 1)])
def test_restatement_reproduces_the_per_bucket_tensors(name, skip):
    g = np.load(os.path.join(GOLD, name + '.npz'))
    K = len(g['support'])
    _check_restatement(g, '', 'aux_reward_logits', 'tensor_loss_reward', 'tensor_reward_rec', 1)
    lp, b = _check_restatement(g, '', 'aux_reward_logits_pred', 'tensor_logprob_reward', 'tensor_reward_pred', 1)
    assert 'tensor_logprob_reward-1' not in g.files and 'metric_logprob_reward-1' not in g.files
    assert [k for k in g.files if k.startswith('tensor_logprob_reward') and k != 'tensor_logprob_reward'] == \
        [f'tensor_logprob_reward{i}' for i in range(K)]
    hit = set()
    for i in range(K):
        ref = g[f'tensor_logprob_reward{i}']
        mask = (b == i).numpy()
        assert np.array_equal(~np.isnan(ref), mask), f'bucket {i}: the fp32 bin rule gives other entries than the reference'
        np.testing.assert_allclose(np.where(mask, lp.numpy(), np.nan), ref, rtol=1e-5, atol=2e-6, equal_nan=True)
        m = float(g[f'metric_logprob_reward{i}'])
        if mask.any():
            hit.add(i)
            assert abs(float(lp[torch.from_numpy(mask)].mean()) - m) < 1e-5
        else:
            assert np.isnan(m)
    assert hit == set(range(K)) - {skip}, 'one bucket is deliberately never hit'


def test_menu_holds_midpoints_and_values_beyond_both_ends():
    g = np.load(os.path.join(GOLD, 'tiny_reward_categorical.npz'))
    sup = g['support']
    r = np.concatenate([g['s0_in_reward'].ravel(), g['s1_in_reward'].ravel()])
    assert set(sup.tolist()) <= set(r.tolist())
    mids = (sup[:-1] + sup[1:]) / 2
    tie = [m for m in mids if m in r and (m - sup[list(mids).index(m)]) ** 2 == (m - sup[list(mids).index(m) + 1]) ** 2]
    assert tie, 'no exact midpoint among the rewards'
    assert r.min() < sup.min() and r.max() > sup.max()
    # a tie goes to the lower bucket
    for m in tie:
        assert int(bins_fp32(np.float32(m), sup)) == list(mids).index(m)
