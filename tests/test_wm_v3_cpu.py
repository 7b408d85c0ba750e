"""CPU (-m "not gpu"): the host side of the world model's free bits and symlog two-hot reward head - the three
entry points (dm_kl_free_fwd / dm_kl_free_bwd in csrc/elementwise.hip, dm_twohot_head_loss in csrc/twohot.hip) are exported,
declared and bound and refuse bad arguments on the host with nothing launched; the ABI version and the metric buffer keep their
sizes and the new slot table is disjoint from the others; the config keys are inert by default in every section; WorldModel and
MultiDecoder refuse bad values at construction (on the meta device, before anything is allocated); the default model's
state_dict is unchanged and reward_dist='twohot' changes only the shape of the reward head's output layer; the heads' forward
and backward plans and the step workspace hold at an output width of 255 and 256; and the float64 two-hot encoding of
tests/wm_v3_case.py sums to 1 per row and decodes an in-range target back to itself.  The last two groups - the plans at 255 / 256
and the float64 encoding - pin existing queries and the tests' own reference, not the feature: they pass without it; every other
test here fails without it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pydreamer_amd import config, hip
from tests import twohot_case as TC
from tests import wm_v3_case as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DM_E_SHAPE, DM_E_NULL = -1, -5
P = 64      # a placeholder pointer a launch would fault on
KEYS = dict(kl_free=0.0, reward_dist='normal', reward_twohot_bins=255, reward_twohot_range=20.0)
NEW = ('dm_kl_free_fwd', 'dm_kl_free_bwd', 'dm_twohot_head_loss')


def _rc(name, *args):
    return getattr(hip.lib(), name)(*args)


def _err():
    return hip.lib().dm_last_error().decode()


def _meta(conf):
    from pydreamer_amd.models import Dreamer
    with torch.device('meta'):
        return Dreamer(conf)


def test_symbols_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'dreamer_hip.h')).read()
    declared = set(re.findall(r'\b(dm_[a-z0-9_]+)\s*\(', hdr))
    lib = hip.lib()
    for n in NEW:
        assert n in declared and n in hip.exported_symbols() and hasattr(lib, n), n
    assert lib.dm_version() == hip.DM_ABI_VERSION == 17
    from pydreamer_amd import models as M
    assert M.METRIC_BUF_FLOATS == 48
    assert M.KL_FREE_METRIC_SLOTS['loss_kl_clip'] == 45 and M.KL_FREE_METRIC_SLOTS['kl_free_frac'] == 46
    others = (M.METRIC_SLOTS, M.GOALS_METRIC_SLOTS, M.RETURN_METRIC_SLOTS)
    for other in others:
        assert not set(M.KL_FREE_METRIC_SLOTS) & set(other)
        assert not set(M.KL_FREE_METRIC_SLOTS.values()) & set(other.values())
    assert all(0 <= i < M.METRIC_BUF_FLOATS for i in M.KL_FREE_METRIC_SLOTS.values())


def test_kl_free_fwd_checks_arguments_on_the_host():
    """dm_kl_free_fwd(rows, S, C, post, prior, free, kl, kl_clip, closed, ent_post, ent_prior, stream)."""
    ok = dict(rows=3, S=8, C=8, post=P, prior=P, free=1.0, kl=P, kl_clip=P, closed=P, ent_post=P, ent_prior=P, stream=None)
    call = lambda **kw: _rc('dm_kl_free_fwd', *{**ok, **kw}.values())
    for gone in ('post', 'prior', 'kl', 'kl_clip', 'closed'):
        assert call(**{gone: None}) == DM_E_NULL and 'null' in _err() and 'kl_free_fwd' in _err(), gone
    for free in (-1.0, -1e-30, float('inf'), float('-inf'), float('nan')):
        assert call(free=free) == DM_E_SHAPE and 'free' in _err() and 'kl_free_fwd' in _err(), free
    assert call(S=0) == DM_E_SHAPE and call(C=-1) == DM_E_SHAPE
    for C in (8, 64, 0):      # staged, plain, Gaussian: nothing to do, nothing launched
        assert call(rows=0, C=C) == 0 and call(rows=0, C=C, ent_post=None, ent_prior=None) == 0
    with pytest.raises(hip.DreamerHipError, match='kl_free_fwd'):
        hip.call('dm_kl_free_fwd', 3, 8, 8, P, P, -2.0, P, P, P, None, None, None)


def test_kl_free_bwd_checks_arguments_on_the_host():
    """dm_kl_free_bwd(rows, S, C, post, prior, closed, scale_post, scale_prior, dpost, dprior, stream)."""
    ok = dict(rows=3, S=8, C=8, post=P, prior=P, closed=P, scale_post=0.2, scale_prior=0.8, dpost=P, dprior=P, stream=None)
    call = lambda **kw: _rc('dm_kl_free_bwd', *{**ok, **kw}.values())
    for gone in ('post', 'prior', 'closed', 'dpost', 'dprior'):
        assert call(**{gone: None}) == DM_E_NULL and 'null' in _err() and 'kl_free_bwd' in _err(), gone
    assert call(S=0) == DM_E_SHAPE and call(C=-1) == DM_E_SHAPE
    for C in (8, 64, 0):
        assert call(rows=0, C=C) == 0
    # the pair without the gate keeps its own checks
    assert _rc('dm_kl_balance_fwd', 3, 8, 8, P, P, None, P, P, None) == DM_E_NULL
    assert _rc('dm_kl_balance_bwd', 3, 8, 8, P, P, 0.2, 0.8, None, P, None) == DM_E_NULL


def test_twohot_head_loss_checks_arguments_on_the_host():
    """dm_twohot_head_loss(rows, I, K, logits, ld, bins, target, scale, loss, dlogits, mean, stream)."""
    ok = dict(rows=6, I=2, K=255, logits=P, ld=255, bins=P, target=P, scale=1.0, loss=P, dlogits=P, mean=P, stream=None)
    call = lambda **kw: _rc('dm_twohot_head_loss', *{**ok, **kw}.values())
    for K in (1, 0, -3, 257):
        assert call(K=K, ld=300) == DM_E_SHAPE and f'K={K}' in _err() and 'twohot_head_loss' in _err()
    assert call(rows=-2) == DM_E_SHAPE and 'rows=-2' in _err()
    assert call(ld=254) == DM_E_SHAPE and 'ld=254' in _err()
    for I in (0, -1):
        assert call(I=I) == DM_E_SHAPE and f'I={I}' in _err()
    assert call(rows=7) == DM_E_SHAPE and 'rows=7' in _err() and call(rows=6, I=4) == DM_E_SHAPE
    for gone in ('logits', 'bins'):
        assert call(**{gone: None}) == DM_E_NULL and 'null' in _err() and 'twohot_head_loss' in _err(), gone
    assert call(loss=None, dlogits=None, mean=None) == DM_E_NULL and 'no output' in _err()
    assert call(target=None) == DM_E_NULL and call(target=None, loss=None) == DM_E_NULL and 'target' in _err()
    assert call(target=None, dlogits=None) == DM_E_NULL
    assert call(rows=0) == 0 and call(rows=0, target=None, loss=None, dlogits=None) == 0      # nothing to do, nothing launched
    # the critic's entries keep their NULL refusals
    assert _rc('dm_twohot_loss', 3, 5, 7, P, 7, P, P, None, 1.0, P, P, P, None) == DM_E_NULL
    assert _rc('dm_twohot_loss', 3, 5, 7, P, 7, P, P, P, 1.0, None, P, P, None) == DM_E_NULL
    assert _rc('dm_twohot_decode', 3, 7, P, 7, P, None, None) == DM_E_NULL
    with pytest.raises(hip.DreamerHipError, match='twohot_head_loss'):
        hip.call('dm_twohot_head_loss', 6, 4, 7, P, 7, P, P, 1.0, P, P, P, None)


def test_config_defaults_and_overrides():
    over = dict(kl_free=1.0, reward_dist='twohot', reward_twohot_bins=31, reward_twohot_range=10.0)
    for name in config.SECTIONS:
        c = config.load_config('defaults', name) if name != 'defaults' else config.load_config('defaults')
        assert {k: getattr(c, k) for k in KEYS} == KEYS, name
        c = config.load_config('defaults', name, **over)
        assert {k: getattr(c, k) for k in over} == over, name
    m = _meta(config.load_config('defaults', 'atari', **over))
    head = m.wm.decoder.reward
    assert (m.wm.kl_free, type(head).__name__, head.K, head.bin_range, head.model.out_dim) == (1.0, 'DenseTwoHotDecoder', 31, 10.0, 31)
    assert head.target_rows is False


@pytest.mark.parametrize('bad,exc', [
    (dict(kl_free=-1.0), ValueError), (dict(kl_free=float('inf')), ValueError), (dict(kl_free=float('nan')), ValueError),
    (dict(kl_free=1.0, iwae_samples=2), NotImplementedError),
    (dict(reward_dist='gauss'), ValueError), (dict(reward_twohot_bins=1), ValueError), (dict(reward_twohot_bins=257), ValueError),
    (dict(reward_twohot_bins=0), ValueError), (dict(reward_twohot_bins=31.5), ValueError), (dict(reward_twohot_range=0.0), ValueError),
    (dict(reward_twohot_range=-1.0), ValueError), (dict(reward_twohot_range=float('inf')), ValueError),
    (dict(reward_twohot_range=float('nan')), ValueError),
    (dict(reward_dist='twohot', reward_decoder_categorical=[-10, 0, 1, 10], clip_rewards=None), ValueError)])
def test_refusals_at_construction(bad, exc):
    key = 'kl_free' if 'kl_free' in bad else 'reward_decoder_categorical' if 'reward_decoder_categorical' in bad else next(iter(bad))
    with pytest.raises(exc, match=key):
        _meta(config.load_config('defaults', 'atari', **bad))
    if 'kl_free' not in bad and 'reward_decoder_categorical' not in bad:      # ... whatever reward_dist says
        with pytest.raises(exc, match=key):
            _meta(config.load_config('defaults', 'atari', **{**dict(reward_dist='twohot'), **bad}))
    from pydreamer_amd.models import DenseTwoHotDecoder
    for kw in (dict(bins=1), dict(bins=257), dict(bin_range=0.0), dict(bin_range=float('nan'))):
        with torch.device('meta'), pytest.raises(ValueError, match='reward_twohot'):
            DenseTwoHotDecoder(40, **kw)


def test_iwae_with_free_bits_is_refused_at_the_call_too():
    m = _meta(config.load_config('defaults', 'atari', kl_free=0.5))
    obs = dict(action=torch.zeros(2, 3, 18), reward=torch.zeros(2, 3), reset=torch.zeros(2, 3, dtype=torch.bool), terminal=torch.zeros(2, 3))
    with pytest.raises(NotImplementedError, match='kl_free'):
        m.training_step(obs, None, iwae_samples=2)
    with pytest.raises(NotImplementedError, match='kl_free'):
        m.wm.training_step(obs, None, iwae_samples=2)


def test_state_dict_keys():
    from pydreamer_amd.models import DenseNormalDecoder, DenseTwoHotDecoder, MLP
    base = _meta(config.load_config('defaults', 'atari'))
    keys = list(base.state_dict())
    mlp_keys = [f'model.{3 * i + j}.{w}' for i in range(4) for j in (0, 1) for w in ('weight', 'bias')] + ['model.12.weight', 'model.12.bias']
    assert [k for k in keys if k.startswith('wm.decoder.reward.')] == [f'wm.decoder.reward.model.{k}' for k in mlp_keys]
    assert base.state_dict()['wm.decoder.reward.model.model.12.weight'].shape == (1, 400)
    assert isinstance(base.wm.decoder.reward, DenseNormalDecoder) and base.wm.kl_free == 0.0
    assert list(_meta(config.load_config('defaults', 'atari', kl_free=1.0)).state_dict()) == keys
    on = _meta(config.load_config('defaults', 'atari', reward_dist='twohot', reward_twohot_bins=31, kl_free=1.0))
    sd, sd0 = on.state_dict(), base.state_dict()
    assert list(sd) == keys
    differ = [k for k in keys if sd[k].shape != sd0[k].shape]
    assert differ == ['wm.decoder.reward.model.model.12.weight', 'wm.decoder.reward.model.model.12.bias']
    assert sd[differ[0]].shape == (31, 400) and sd[differ[1]].shape == (31,)
    assert sd_default_bins(_meta(config.load_config('defaults', 'atari', reward_dist='twohot'))) == 255
    # a real (CPU) world model: the output layer is zero behind the tf2 initialiser, the bins are the fp32 linspace
    from pydreamer_amd.models import WorldModel
    c = config.load_config('defaults', 'atari', deter_dim=32, hidden_dim=32, stoch_dim=4, stoch_discrete=4, cnn_depth=4,
                           reward_dist='twohot', reward_twohot_bins=7, reward_twohot_range=5.0)
    head = WorldModel(c).decoder.reward
    assert isinstance(head, DenseTwoHotDecoder) and isinstance(head.model, MLP) and head.model.out_dim == 7
    assert not head.model.model[12].weight.any() and not head.model.model[12].bias.any() and head.model.model[9].weight.any()
    assert torch.equal(head.bins, torch.linspace(-5.0, 5.0, 7)) and 'bins' not in head.state_dict()


def sd_default_bins(model):
    return model.state_dict()['wm.decoder.reward.model.model.12.bias'].shape[0]


def test_packed_metric_names_follow_the_switch():
    from pydreamer_amd import models as M
    from pydreamer_amd.train import default_slots
    off, on = _meta(config.load_config('defaults', 'atari')), _meta(config.load_config('defaults', 'atari', kl_free=1.0))
    off.metric_buffer = on.metric_buffer = None
    assert off.packed_metrics()[0] == list(M.METRIC_SLOTS)
    names, _, idx = on.packed_metrics()
    assert names == list(M.METRIC_SLOTS) + list(M.KL_FREE_METRIC_SLOTS) and idx[-2:] == [45, 46]
    assert 'kl_free_frac' not in default_slots(off) and default_slots(on)['kl_free_frac'][0] == 46
    assert default_slots(on)['loss_kl_clip'][0] == 45
    both = _meta(config.load_config('defaults', 'atari', kl_free=1.0, return_norm='percentile'))
    both.metric_buffer = None
    assert both.packed_metrics()[0] == list(M.METRIC_SLOTS) + list(M.RETURN_METRIC_SLOTS) + list(M.KL_FREE_METRIC_SLOTS)


def _plan(which, rows, in_dim, out_dim, sparse_cols=0, has_acts=1, precision=0, ws_bytes=1 << 40):
    out = (ctypes.c_int32 * 8)()
    rc = hip.lib().dm_mlp_plan_query(which, rows, in_dim, 400, 4, out_dim, in_dim, sparse_cols, 16, 1, precision, has_acts, 0, 0, 0,
                                     ws_bytes, out)
    return rc, (out[6] & 0xFFFFFFFF) | ((out[7] & 0xFFFFFFFF) << 32)


@pytest.mark.parametrize('K', [255, 256])
def test_heads_plan_and_workspace_at_the_two_hot_width(K):
    """The reward head at out_dim 255 / 256: heads_loss (T B rows, activations kept, sparse one-hot columns), the dream windows
    ((H + 1) T B rows, no activations) and the heads' backward each get a plan, and the plan's need fits dm_mlp_ws_floats of those
    rows - what MLP.fwd checks - and the heads' part of dm_workspace_query, which sizes the step workspace.  The tiny shapes and
    the Atari-literal ones (2 500 and 40 000 rows, features 600 + 32 x 32), fp32 and bf16 operands."""
    lib = hip.lib()
    for (T, B, Hh, D_, S, C) in ((5, 3, 4, 64, 8, 8), (50, 50, 15, 600, 32, 32)):
        F_, sparse = D_ + S * C, S * C
        shp = hip.make_shape(T=T, B=B, I=1, H=Hh, D=D_, Hd=D_, S=S, C=C, E=256, A=6, mlp_hidden=400, mlp_layers=4, cnn_depth=8, img=64,
                             img_ch=3, flags=0)
        parts = (ctypes.c_size_t * 8)()
        assert lib.dm_workspace_query(ctypes.byref(shp), parts, 8) == 0, _err()
        for rows, has_acts in ((T * B, 1), ((Hh + 1) * T * B, 0)):
            bound = int(lib.dm_mlp_ws_floats(rows, 400, 4))
            assert bound <= parts[7]
            for precision in (0, 1):
                for which in (0, 1):
                    if which == 1 and not has_acts:
                        continue      # nobody differentiates the dream's reward head
                    for sp in (0, sparse):
                        rc, need = _plan(which, rows, F_, K, sp if which == 0 else 0, has_acts, precision)
                        assert rc == 0, (K, rows, which, precision, sp, _err())
                        assert 0 < need <= bound, (K, rows, which, precision, sp, need, bound)
                        rc2, need2 = _plan(which, rows, F_, K, sp if which == 0 else 0, has_acts, precision, ws_bytes=4 * bound)
                        assert rc2 == 0 and need2 <= bound


@pytest.mark.parametrize('K,R', [(2, 20.0), (3, 20.0), (7, 5.0), (255, 20.0), (256, 20.0)])
def test_float64_two_hot_encoding(K, R):
    bins = torch.linspace(-R, R, K).double()
    g = torch.Generator().manual_seed(K)
    hi = float(TC.symexp(torch.tensor(min(R, 15.0), dtype=torch.float64)))
    inside = (torch.rand(400, generator=g, dtype=torch.float64) * 2 - 1) * hi
    special = torch.cat([TC.symexp(bins)[:: max(1, K // 16)], torch.tensor([0.0, 1e-30, -1e-30], dtype=torch.float64)])
    target = torch.cat([inside, special])
    y = WC.twohot_encode(target, bins)
    assert y.shape == (target.numel(), K) and bool((y >= 0).all()) and bool(((y > 0).sum(-1) <= 2).all())
    assert torch.allclose(y.sum(-1), torch.ones(target.numel(), dtype=torch.float64), rtol=0, atol=1e-14)
    back = TC.symexp((y * bins).sum(-1))
    assert torch.allclose(back, target, rtol=1e-10, atol=1e-12), float((back - target).abs().max())
    # beyond either end the encoding is the end bin itself
    far = WC.twohot_encode(torch.tensor([1e30, -1e30], dtype=torch.float64), bins)
    assert float(far[0, -1]) == 1.0 and float(far[1, 0]) == 1.0
    # the restated head: cross-entropy against the encoding, and the free-bits rule
    logits = torch.randn(target.numel(), K, generator=g, dtype=torch.float64)
    loss, dl, mean = WC.twohot_head(logits, bins, target)
    assert torch.allclose(loss, -(y * torch.log_softmax(logits, -1)).sum(-1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dl, torch.softmax(logits, -1) - y, rtol=0, atol=1e-14)
    kl = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    clip, closed = WC.free_bits(kl, 1.0)
    assert clip.tolist() == [1.0, 1.0, 2.0] and closed.tolist() == [1.0, 1.0, 0.0]
    free, gap = WC.mid_free(np.array([0.1, 0.2, 1.0, 1.1, 3.0, 9.0]))
    assert abs(free - 1.05) < 1e-12 and abs(gap - 0.1) < 1e-12      # the central third is [1.0, 1.1]
