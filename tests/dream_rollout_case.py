"""dm_dream_rollout stand-alone through the C-ABI against an fp64 restatement of the imagination rollout (dreamer.py:188-216,
rssm.py:155-184, a2c.py:43-55): the case table and the body shared by test_gpu_dream_rollout.py (the GPU runs) and
test_dream_rollout_case_cpu.py (the preconditions those runs rely on).  Not a test module.

make_case(), oracle_run(), plan_bits() and plan_floats() need no GPU: the per-case seeds of CASES were chosen with them
(free-running fp64 oracle, minimum distance of a uniform from an fp64 CDF edge over all draws of a row).

plan_bits() restates the predicates RolloutCtx::plan (csrc/rssm.hip) chooses its schedule with - dm_z_embed_ok
(elementwise.hip), dm_mlp_chain_ok with its 256-row floor and dm_mlp_chain_sparse_ok (mlp_chain.hip), dm_panel_ok (panel.hip);
plan_floats() restates its carving.  Neither reads the library's report.
"""
import ctypes
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import dreamer_oracle as O

DEV = 'cuda'
EDGE = 1e-6               # the band around a CDF edge inside which fp32 summation order may legitimately flip a draw
EXACT_MAX_ROWS = 301      # up to here every row must be clear of EDGE; above, rows inside it are left out (<= 0.1 % of them)
MLP_HIDDEN, MLP_LAYERS = 400, 4
BITS = ('wzt', 'wat', 'actor_wpack', 'actor_add0', 'fuse_act', 'tw_on')
ACTOR_KINDS = {'onehot': 0, 'tanh_normal': 1, 'normal_tanh': 2}
GRU_KINDS = {'gru': 0, 'gru_layernorm': 1, 'gru_layernorm_dv2': 2}

MID = dict(deter_dim=256, hidden_dim=256, stoch_dim=8, stoch_discrete=32)
GAUSS = dict(stoch_dim=16, stoch_discrete=0)
TWIN = dict(deter_dim=400, hidden_dim=400)            # the cell's products at K = 400 = DM_HSTORE_MIN_K_DENSE (gemm.hip)


def bits(s):
    """'wzt+wat' -> {every SCHED_ROLL bit: bool}"""
    on = set(filter(None, s.split('+')))
    assert on <= set(BITS), on
    return {k: k in on for k in BITS}


def fmt(b):
    return '+'.join(k for k in BITS if b[k]) or 'none'


# ---------------------------------------------------------------- the case table -----------------
# name -> dict(M, H, kw (overrides of O.tiny_conf), seed, start, bits (the schedule that must run, written out by hand from
# the predicates; test_dream_rollout_case_cpu.py holds it against plan_bits()), bf16)
CASES = OrderedDict()
ALL5 = 'wzt+wat+actor_wpack+actor_add0+fuse_act'
# Seeds: the first of 5, 6, ... at which no draw of the case comes closer than 2e-6 to an fp64 CDF edge - 5 unless named here
# (the distances: the table in test_gpu_dream_rollout.py).  40 x 32 latents at 300 rows make 1.9 M (draw, edge) pairs: 262 seeds fail.
SEEDS = {'tiny-M301': 6, 'mid-M301': 9, 'hd1028-M300': 8, 'gru_layernorm-mid-M300': 12, 'gru_layernorm_dv2-mid-M300': 8,
         'stoch40x32-M64': 15, 'stoch40x32-M300': 267, 'stoch65x4-M300': 12, 'mixed-start-M300': 6}


def _case(name, M, kw, want, H=5, start='onehot', bf16=False):
    assert name not in CASES, name
    CASES[name] = dict(name=name, M=M, H=H, kw=dict(kw), seed=SEEDS.get(name, 5), start=start, bits=bits(want), bf16=bf16)


# 1. row boundaries of the default cell
for _M in (1, 37, 64, 65, 255, 256, 301):
    _case(f'tiny-M{_M}', _M, {}, ALL5 if _M >= 256 else 'wzt+wat')
    _case(f'mid-M{_M}', _M, MID, ALL5 if _M >= 256 else 'wzt+wat')
_case('tiny-M16384-panel', 16384, {}, 'wzt+wat', H=2)
# 2. H = 1: no second step, nothing gathered
_case('h1-M37', 37, {}, '', H=1)
_case('h1-M300', 300, {}, 'actor_wpack+fuse_act', H=1)
# 3. hidden 1028: past the gather's 1024
_case('hd1028-M65', 65, dict(hidden_dim=1028), '')
_case('hd1028-M300', 300, dict(hidden_dim=1028), 'actor_wpack+fuse_act')
# 4. continuous actors
for _d in ('tanh_normal', 'normal_tanh'):
    _kw = dict(actor_dist=_d, action_dim=4)
    _case(f'{_d}-mid-M37', 37, dict(MID, **_kw), 'wzt')
    _case(f'{_d}-mid-M65', 65, dict(MID, **_kw), 'wzt')
    _case(f'{_d}-M300', 300, _kw, 'wzt+actor_wpack+actor_add0')
    _case(f'{_d}-A17-M300', 300, dict(actor_dist=_d, action_dim=17), 'wzt')
# 5. a one-hot actor wider than the whole-MLP kernel's 32 outputs
_case('A33-M300', 300, dict(action_dim=33), 'wzt+wat')
# 6. deter 36: the dense part of the actor's first layer is no multiple of 8
_case('deter36-M300', 300, dict(deter_dim=36), 'wzt+wat+actor_wpack+fuse_act')
# 7. Gaussian latents
_case('gauss-M37', 37, GAUSS, '')
_case('gauss-M300', 300, GAUSS, 'actor_wpack+fuse_act')
_case('gauss-tanh_normal-M37', 37, dict(GAUSS, actor_dist='tanh_normal', action_dim=4), '')
_case('gauss-tanh_normal-M300', 300, dict(GAUSS, actor_dist='tanh_normal', action_dim=4), 'actor_wpack')
# 8. cells
for _g in ('gru_layernorm', 'gru_layernorm_dv2'):
    _case(f'{_g}-M37', 37, dict(gru_type=_g), 'wzt+wat')
    _case(f'{_g}-M300', 300, dict(gru_type=_g), ALL5)
    _case(f'{_g}-mid-M300', 300, dict(MID, gru_type=_g), ALL5)
_case('gru2-M37', 37, dict(gru_layers=2), 'wzt+wat')
_case('gru2-M300', 300, dict(gru_layers=2), ALL5)
_case('gru4-deter96-M65', 65, dict(gru_layers=4, deter_dim=96), 'wzt+wat')
_case('gru4-deter96-M300', 300, dict(gru_layers=4, deter_dim=96), ALL5)
_case('dv2x2-M65', 65, dict(gru_type='gru_layernorm_dv2', gru_layers=2), 'wzt+wat')
_case('dv2x2-M300', 300, dict(gru_type='gru_layernorm_dv2', gru_layers=2), ALL5)
# 9. layer_norm=False
_case('nonorm-M37', 37, dict(layer_norm=False), 'wzt+wat')
_case('nonorm-M300', 300, dict(layer_norm=False), 'wzt+wat')
# 10. ragged latent widths
_case('stoch5x12-M300', 300, dict(stoch_dim=5, stoch_discrete=12), ALL5)
for _S, _C in ((40, 32), (65, 4)):
    _case(f'stoch{_S}x{_C}-M64', 64, dict(stoch_dim=_S, stoch_discrete=_C), 'wzt+wat')
    _case(f'stoch{_S}x{_C}-M300', 300, dict(stoch_dim=_S, stoch_discrete=_C), ALL5)
# 11. start states that are not one-hot
_case('mixed-start-M300', 300, {}, ALL5, start='mixed')
# 12. kept activations / no index buffer (their own seeds: the options change no value, the cases are compared like any other)
_case('keep-M65', 65, {}, 'wzt+wat')
_case('keep-M300', 300, {}, ALL5)
_case('keep-tanh_normal-M300', 300, dict(actor_dist='tanh_normal', action_dim=4), 'wzt+actor_wpack+actor_add0')
# 13. workspace fallbacks
_case('ws-M300', 300, {}, ALL5)
# 14. bf16 twins (compared run against run, not against the oracle: no precondition on the seed)
for _H in (42, 39):
    _case(f'twins-M64-H{_H}', 64, TWIN, 'wzt+wat+tw_on', H=_H, bf16=True)
    _case(f'twins-M520-H{_H}', 520, TWIN, 'wzt+wat+actor_wpack+fuse_act+tw_on', H=_H, bf16=True)


# ---------------------------------------------------------------- inputs and oracle --------------
def conf_of(kw):
    return O.tiny_conf(**kw)


def make_case(M, H, conf_kw=None, seed=5, start='onehot'):
    """Config, parameters and inputs of one case (CPU tensors).  start: 'onehot' (h = tanh(randn), z one-hot - or randn for
    Gaussian latents), or 'mixed': rows r % 3 == 0 as before, r % 3 == 1 a dense z of random positive values with about a third
    of the entries set to exactly 0, r % 3 == 2 the rows of init_state (h = 0, z = 0)."""
    oconf = conf_of(conf_kw or {})
    D_, Hd, S, C, A = oconf.deter_dim, oconf.hidden_dim, oconf.stoch_dim, oconf.stoch_discrete, oconf.action_dim
    Z = S * (C or 1)
    g = torch.Generator().manual_seed(seed)
    c = dict(oconf=oconf, params=O.make_params(oconf), M=M, H=H, D=D_, Hd=Hd, S=S, C=C, A=A, Z=Z, F=D_ + Z,
             kind=ACTOR_KINDS[oconf.actor_dist], seed=seed)
    c['AO'] = A if c['kind'] == 0 else 2 * A
    h = torch.tanh(torch.randn(M, D_, generator=g))
    z = F.one_hot(torch.randint(0, C, (M, S), generator=g), C).float().reshape(M, Z) if C else torch.randn(M, S, generator=g)
    c['u_act'] = torch.rand(H, M, generator=g) if c['kind'] == 0 else torch.randn(H, M, A, generator=g)
    c['u_prior'] = torch.rand(H, M, S, generator=g) if C else torch.randn(H, M, S, generator=g)
    if start == 'mixed':      # (its own generator: the layout of the other inputs does not depend on the start state)
        g2 = torch.Generator().manual_seed(1000 + seed)
        dense = torch.rand(M, Z, generator=g2) + 0.05
        dense[torch.rand(M, Z, generator=g2) < 0.33] = 0.0
        r = torch.arange(M) % 3
        z = torch.where((r == 1).unsqueeze(-1), dense, z)
        z[r == 2] = 0.0
        h[r == 2] = 0.0
    else:
        assert start == 'onehot', start
    c['h0'], c['z0'] = h, z
    return c


def case_inputs(case):
    return make_case(case['M'], case['H'], case['kw'], case['seed'], case['start'])


def _draw(logits, u):
    """The sampler's rule on the given logits (..., n) in their own precision: cumsum of the softmax,
    idx = #{k : cdf_k <= u * cdf_last} clamped; and the distance of u * cdf_last from the nearest edge, the last (the clamp,
    not a decision) excluded."""
    cdf = torch.cumsum(torch.softmax(logits, -1), -1)
    target = u.to(cdf.dtype).unsqueeze(-1) * cdf[..., -1:]
    idx = (cdf <= target).sum(-1).clamp(max=logits.shape[-1] - 1)
    return idx, (cdf[..., :-1] - target).abs().min(-1).values


def _continuous(kind, y, eps):
    """functions.py:59-78 with torch.normal(mean, std) restated as mean + std * eps (O.sample_continuous, which casts to float,
    in the precision of y)."""
    mean_, std_ = y.chunk(2, -1)
    if kind == 2:
        return torch.tanh(mean_) + (torch.sigmoid(std_) + 0.01) * eps
    return torch.tanh(5 * torch.tanh(mean_ / 5) + (F.softplus(std_) + 0.1) * eps)


def oracle_run(c, dtype=torch.float64):
    """The rollout in `dtype` (fp64: the oracle; fp32: the floor a derived bar is taken from) on the CPU.  Returns features
    (H+1, M, F), actions (H, M, A), action indices (H, M), latent indices (H, M, S), the actor's output per step (H, M, AO)
    and per row the minimum distance over all its draws of a uniform from a CDF edge (inf for a row without draws)."""
    oconf, H, M, S, C, A, kind = c['oconf'], c['H'], c['M'], c['S'], c['C'], c['A'], c['kind']
    p = {k: v.to(dtype) for k, v in c['params'].items() if k.startswith(('wm.core.', 'ac.actor.'))}
    h, z = c['h0'].to(dtype), c['z0'].to(dtype)
    feats, actions, aidx, zidx, outs = [], [], [], [], []
    dist = torch.full((M,), float('inf'), dtype=torch.float64)
    with torch.no_grad():
        for i in range(H):
            feature = torch.cat((h, z), -1)
            y = O.mlp(p, 'ac.actor.model', feature, MLP_LAYERS)
            if kind == 0:
                ai, d = _draw(y, c['u_act'][i])
                action = F.one_hot(ai, A).to(dtype)
                dist = torch.minimum(dist, d.double())
            else:
                action, ai = _continuous(kind, y, c['u_act'][i].to(dtype)), torch.zeros(M, dtype=torch.long)
            feats.append(feature); actions.append(action); aidx.append(ai); outs.append(y)
            h = O.cell_trunk(p, action, h, z)
            prior = O.prior_head(p, h)
            if C:
                zi, d = _draw(prior.reshape(M, S, C), c['u_prior'][i])
                z = F.one_hot(zi, C).to(dtype).reshape(M, S * C)
                dist = torch.minimum(dist, d.double().min(-1).values)
            else:
                mean, std = O.gaussian_params(prior)
                z, zi = mean + std * c['u_prior'][i].to(dtype), torch.zeros(M, S, dtype=torch.long)
            zidx.append(zi)
        feats.append(torch.cat((h, z), -1))
    return dict(feat=torch.stack(feats), actions=torch.stack(actions), act_idx=torch.stack(aidx), lat_idx=torch.stack(zidx),
                logits=torch.stack(outs), row_dist=dist)


# ---------------------------------------------------------------- RolloutCtx::plan restated ------
def z_embed_ok(n):
    return n <= 1024 and n % 4 == 0


def chain_ok(rows, in_dim, hidden, layers, out_dim, normed):
    """dm_mlp_chain_ok with the default dm_mlp_chain_min_rows (x = the feature rows: ldx = in_dim, 16-byte aligned)"""
    return hidden == 400 and rows >= 256 and 1 <= layers <= 8 and 1 <= out_dim <= 32 and in_dim % 4 == 0 and in_dim >= 4 and normed


def panel_ok(rows, hidden):
    return hidden == 400 and rows >= 16384


def chain_sparse_ok(in_dim, sparse_cols, bf16):
    dense = in_dim - sparse_cols
    return not bf16 and 0 < sparse_cols < in_dim and in_dim <= 4096 and dense % 8 == 0 and dense >= 32


def plan_bits(oconf, M, H, bf16=False, twins=True, fuse_switch=True, fits=('wzt', 'wpack', 'add0')):
    """The schedule word of a dm_dream_rollout call from the shape (and which optional workspace blocks fit)."""
    D_, Hd, S, C, A = oconf.deter_dim, oconf.hidden_dim, oconf.stoch_dim, oconf.stoch_discrete, oconf.action_dim
    Z, kind = S * (C or 1), ACTOR_KINDS[oconf.actor_dist]
    F_, AO = D_ + Z, A if kind == 0 else 2 * A
    wzt = bool(C) and H > 1 and z_embed_ok(Hd) and 'wzt' in fits
    wpack = chain_ok(M, F_, MLP_HIDDEN, MLP_LAYERS, AO, oconf.layer_norm) and not panel_ok(M, MLP_HIDDEN) and 'wpack' in fits
    add0 = wpack and bool(C) and wzt and chain_sparse_ok(F_, Z, bf16) and z_embed_ok(MLP_HIDDEN) and 'add0' in fits
    tw_on = bf16 and twins and oconf.gru_type == 'gru' and oconf.gru_layers == 1 and oconf.layer_norm and F_ % 8 == 0
    return dict(wzt=wzt, wat=wzt and kind == 0, actor_wpack=wpack, actor_add0=add0, fuse_act=kind == 0 and wpack and fuse_switch,
                tw_on=tw_on)


def plan_floats(c, keep_acts=False, tw_on=False):
    """RolloutCtx::plan's carving in floats (every take rounded up to a 64-float granule): `must` - the split-K scratch, the
    actor's activation ping-pong and output (not with kept activations), ea / x1 / za (M x Hd each), the LayerNorm statistics,
    gi / gh (M x 3D each), the prior's parameters, the LayerNorm cells' gate sums and statistics, the bf16 twins - then the
    optional blocks in the order they are taken: `wzt` (z_mlp^T, a_mlp^T, the latent and action indices), `wpack` (the actor's
    fragment-major weights: 25 column blocks x ceil(K / 32) x 512 floats per layer), `add0` (the actor's W0^T and the gathered
    addend)."""
    pad = lambda n: (n + 63) // 64 * 64
    half = lambda n: pad((n + 1) // 2)
    M, H, D_, Hd, S, C, A, Z, F_, AO = (c[k] for k in ('M', 'H', 'D', 'Hd', 'S', 'C', 'A', 'Z', 'F', 'AO'))
    ZP = S * (C or 2)
    oconf = c['oconf']
    must = 16 * 1024 * 1024
    if not keep_acts:
        must += MLP_LAYERS * (2 * pad(M * MLP_HIDDEN) + pad(2 * M)) + pad(M * AO)
    must += 3 * pad(M * Hd) + pad(2 * M) + 2 * pad(3 * M * D_) + pad(M * ZP)
    if GRU_KINDS[oconf.gru_type]:
        must += pad(3 * M * D_) + pad(6 * M * oconf.gru_layers)
    if tw_on:
        must += half(3 * D_ * Hd) + half(3 * D_ * D_) + half(Hd * D_) + half(ZP * Hd) + half(M * Hd) + half((H + 1) * M * F_)
    pack = lambda K: 25 * ((K + 31) // 32) * 512
    return dict(must=must, wzt=pad(Z * Hd) + pad(A * Hd) + pad(M * S) + pad(M),
                wpack=pack(F_) + (MLP_LAYERS - 1) * pack(MLP_HIDDEN), add0=pad(F_ * MLP_HIDDEN) + pad(M * MLP_HIDDEN))


def cut_bytes(c, short_of):
    """A workspace that ends one 64-float granule short of the named block of RolloutCtx::plan ('must', 'wzt', 'wpack', 'add0'),
    everything taken before it granted."""
    f = plan_floats(c)
    order = ('must', 'wzt', 'wpack', 'add0')
    return 4 * (sum(f[k] for k in order[:order.index(short_of) + 1]) - 64)


# ---------------------------------------------------------------- the GPU run --------------------
_models = {}


def _model(c, bf16):
    """The Dreamer the case's parameters live in (one per configuration and test session)."""
    from pydreamer_amd import config
    from pydreamer_amd.models import Dreamer
    key = (tuple(sorted(vars(c['oconf']).items())), bf16)
    if key not in _models:
        model = Dreamer(config.load_config('defaults', 'atari', **{**vars(c['oconf']), 'amp': bf16}))
        model.load_state_dict(c['params'], strict=True)
        _models[key] = model.to(DEV)
    return _models[key]


def run_case(c, expect, keep_acts=False, with_act_idx=True, ws_bytes=None, bf16=False, fuse_act=None, twins=None, label=''):
    """One dm_dream_rollout call (the struct packing of Dreamer._dream_from_features) on the case's inputs.  `expect`: the
    SCHED_ROLL bits that must be reported - asserted BEFORE anything is read back.  keep_acts: actor_acts / actor_logits given
    (the trainer's call) or NULL; with_act_idx: act_idx given or NULL; ws_bytes: the workspace size handed over (default
    dm_workspace_bytes); bf16: DM_FLAG_BF16; fuse_act / twins: dm_rollout_fuse_act_enable / dm_bf16_twins_enable for this call
    (None: leave), restored afterwards.  Returns CPU tensors: feat, actions, act_idx, logits (None where not asked for), bits."""
    from pydreamer_amd import hip as H
    model = _model(c, bf16)
    M, Hh, F_, A, S, AO = c['M'], c['H'], c['F'], c['A'], c['S'], c['AO']
    shp = model.wm.shape(1, M, Hh)
    assert bool(shp.flags & H.DM_FLAG_BF16) == bf16 and (shp.flags & 3) == c['kind']
    ws = torch.empty(H.workspace_bytes(shp), dtype=torch.uint8, device=DEV)
    if ws_bytes is not None:
        assert ws_bytes <= ws.numel(), (ws_bytes, ws.numel())
    dev = lambda x: x.to(DEV).contiguous()
    start, u_act, u_prior = dev(torch.cat((c['h0'], c['z0']), -1)), dev(c['u_act']), dev(c['u_prior'])
    SENT = 7.0      # no feature, action or actor output of these cases is exactly 7: a buffer left at it was not written
    feats = torch.full((Hh + 1, M, F_), SENT, device=DEV)
    actions = torch.full((Hh, M, A), SENT, device=DEV)
    act_idx = torch.full((Hh, M), -1, dtype=torch.int32, device=DEV) if with_act_idx else None
    a_acts = a_logits = None
    if keep_acts:
        a_acts = torch.empty(int(model.ac.actor.acts_floats(Hh * M)), device=DEV)
        a_logits = torch.full((Hh * M, AO), SENT, device=DEV)
    cell_p, actor_p = H.rssm_struct(model.wm.core.cell.ordered()), model.ac.actor.struct()
    lib = H.lib()
    keep_fuse, keep_tw = lib.dm_rollout_fuse_act_enable(-1), lib.dm_bf16_twins_enable(-1)
    try:
        if fuse_act is not None:
            lib.dm_rollout_fuse_act_enable(int(fuse_act))
        if twins is not None:
            lib.dm_bf16_twins_enable(int(twins))
        H.call('dm_dream_rollout', ctypes.byref(shp), M, H.fptr(start), ctypes.byref(cell_p), ctypes.byref(actor_p),
               H.fptr(u_act), H.fptr(u_prior), H.fptr(feats), H.fptr(actions), H.ptr(act_idx), H.fptr(a_acts), H.fptr(a_logits),
               H.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, H.stream())
        torch.cuda.synchronize()
    except H.DreamerHipError:
        torch.cuda.synchronize()
        untouched = bool((feats == SENT).all()) and bool((actions == SENT).all())
        raise RolloutRefused(lib.dm_last_error().decode('utf-8', 'replace'), untouched)
    finally:
        lib.dm_rollout_fuse_act_enable(keep_fuse)
        lib.dm_bf16_twins_enable(keep_tw)
    got = H.last_schedule(2)
    print(f'SCHEDULE {label} M={M} H={Hh} {fmt(got)}')
    for k in BITS:
        assert got[k] == expect[k], f'{label}: schedule bit {k} is {got[k]}, expected {expect[k]} (reported {fmt(got)}, expected {fmt(expect)})'
    cpu = lambda t: None if t is None else t.cpu()
    return dict(feat=cpu(feats), actions=cpu(actions), act_idx=cpu(act_idx), bits=got,
                logits=None if a_logits is None else a_logits.cpu().view(Hh, M, AO))


class RolloutRefused(Exception):
    """dm_dream_rollout returned an error; `untouched`: the output buffers still hold their fill value."""

    def __init__(self, message, untouched):
        super().__init__(message)
        self.message, self.untouched = message, untouched


# ---------------------------------------------------------------- bars ---------------------------
def excess(a, b, rtol=0.0):
    """max over elements of |a - b| - rtol |b| (the quantity an absolute bar applies to)"""
    a, b = a.double(), b.double()
    return float(((a - b).abs() - rtol * b.abs()).max()) if a.numel() else 0.0


def clear_rows(c, ora):
    """The rows whose draws all stay EDGE clear of an fp64 CDF edge.  Up to EXACT_MAX_ROWS rows that must be all of them (the
    seed was chosen so); above, at most 0.1 % of the rows may be left out."""
    good = ora['row_dist'] >= EDGE
    if c['M'] <= EXACT_MAX_ROWS:
        assert bool(good.all()), (f"precondition: a uniform lies {float(ora['row_dist'].min()):.2e} from an fp64 CDF edge "
                                  f"(choose another seed than {c['seed']})")
    else:
        assert float((~good).float().mean()) <= 1e-3, f'{int((~good).sum())} of {c["M"]} rows within EDGE of an fp64 CDF edge'
    return good


def figures(c, ora, out, good):
    """The measured quantities of one run against the oracle, on the rows of `good`."""
    D_, C, kind = c['D'], c['C'], c['kind']
    fh, fo = out['feat'][:, good], ora['feat'][:, good]
    fig = dict(feat=excess(fh, fo), min_edge=float(ora['row_dist'][good].min()), left_out=int((~good).sum()))
    if C:
        fig['lat_wrong'] = int((fh[1:, :, D_:] != fo[1:, :, D_:].float()).any(-1).sum())      # one-hot rows: exact or wrong
    if kind == 0:
        fig['act_wrong'] = int((out['actions'][:, good] != ora['actions'][:, good].float()).any(-1).sum())
        if out['act_idx'] is not None:
            fig['idx_wrong'] = int((out['act_idx'][:, good].long() != ora['act_idx'][:, good]).sum())
    else:
        fig['act'] = excess(out['actions'][:, good], ora['actions'][:, good], 1e-4)
    if out['logits'] is not None:
        fig['logits'] = excess(out['logits'][:, good], ora['logits'][:, good], 1e-5)
    return fig


def check(c, ora, out, label, feat_bar=2e-5):
    """The bars: features within feat_bar (2e-5 unless the case derives its own) of fp64 - the Gaussian z columns among them -,
    kept actor outputs within 2e-5 + 1e-5 relative, continuous actions within 1e-4 relative + 1e-5; every action index,
    one-hot action row and one-hot latent row equal to the fp64 draw.  Prints the figures first."""
    good = clear_rows(c, ora)
    fig = figures(c, ora, out, good)
    print(f'PARITY {label} ' + ' '.join(f'{k}={v:.2e}' if isinstance(v, float) else f'{k}={v}' for k, v in fig.items()))
    assert torch.isfinite(out['feat']).all() and torch.isfinite(out['actions']).all(), label
    for k in ('lat_wrong', 'act_wrong', 'idx_wrong'):
        assert fig.get(k, 0) == 0, f'{label}: {fig[k]} row-steps differ from the fp64 draw ({k})'
    assert fig['feat'] <= feat_bar, (label, 'features', fig['feat'])
    assert fig.get('act', 0.0) <= 1e-5, (label, 'continuous actions', fig['act'])
    assert fig.get('logits', 0.0) <= 2e-5, (label, 'actor outputs', fig['logits'])
    return fig
