"""CPU (-m "not gpu"): dm_workspace_bytes is the maximum of the operators' own workspace layouts.

dm_workspace_query reports, per fused operator, the floats its layout function (csrc/conv.hip, csrc/rssm.hip) takes on an
arena without a base with every optional piece wanted; dm_workspace_bytes is 4 * (their maximum + 4096).  Checked here without
a device: that identity over a grid of shapes, the floor every existing operator has (its split-K region), the zero of the
convolution parts where the convolution entry points refuse the shape, the rollout's part against the restatement of its
carving in tests/dream_rollout_case.py, and that no shape asks for more memory than the hand-written formula it replaces did.
"""
import ctypes
import itertools

import dream_rollout_case as R

SPLITK_FLOATS = 16 * 1024 * 1024
SLACK_FLOATS = 4096
PARTS = ('enc_fwd', 'enc_bwd', 'dec_fwd', 'dec_bwd', 'chain', 'bptt', 'rollout', 'mlp')
CONV_PARTS = PARTS[:4]
DM_FLAG_BF16 = 128
GRU_SHIFT, GRU_LAYERS_SHIFT = 5, 8

DEFAULTS = dict(T=50, B=50, I=1, H=15, D=600, Hd=1000, S=32, C=32, A=18, mlp_hidden=400, mlp_layers=4, cnn_depth=48, img=64,
                img_ch=3)
BASES = {
    'defaults': {},
    'img_ch1': dict(img_ch=1),
    'gauss': dict(C=0),
    'imageless': dict(cnn_depth=0, img=0, img_ch=0),
    'depth1': dict(cnn_depth=1),
    'wide': dict(T=48, B=32, D=2048),
    'tiny': dict(T=4, B=3, D=64, Hd=64, S=4, C=4, A=3, cnn_depth=8, H=3),
    'one': dict(T=1, B=1, H=1),
}


def grid():
    """(key, dm_shape fields): every base crossed with DM_FLAG_BF16, the recurrent cell (nn.GRUCell and the two LayerNorm cells),
    gru_layers 1 / 2, a one-hot / continuous actor, I in {1, 3}, H in {1, 15} and the base's own.  key = (base, bf16, I, H) is
    what the replaced formula depended on; E = 32 cnn_depth, the width the convolution encoder requires."""
    for name, over in BASES.items():
        base = dict(DEFAULTS, **over)
        for bf16, kind, layers, actor, I, H in itertools.product((0, 1), (0, 1, 2), (1, 2), (0, 1), (1, 3),
                                                                 sorted({1, 15, base['H']})):
            f = dict(base, I=I, H=H, E=32 * base['cnn_depth'] or 64,
                     flags=actor | (kind << GRU_SHIFT) | ((layers - 1) << GRU_LAYERS_SHIFT) | (DM_FLAG_BF16 if bf16 else 0))
            yield (name, bf16, I, H), f


def query(hip, fields):
    """-> (dm_workspace_bytes, {part: floats})"""
    shp = hip.make_shape(**fields)
    parts = (ctypes.c_size_t * len(PARTS))()
    assert hip.lib().dm_workspace_query(ctypes.byref(shp), parts, len(PARTS)) == 0, hip.lib().dm_last_error()
    return hip.workspace_bytes(shp), dict(zip(PARTS, (int(v) for v in parts)))


# dm_workspace_bytes of the hand-written formula, recorded at commit 2936300 ("Split the MLP heads' launcher into a plan, one
# layout and path functions") for every shape of grid(): it read T, B, I, H, the widths and DM_FLAG_BF16 only, so the 96
# shapes of a key had one value (checked when these were recorded).  {base: {(bf16, I, H): bytes}}
RECORDED = {
    'defaults': {
        (0, 1, 1): 3576761088, (0, 1, 15): 3576761088, (0, 3, 1): 10593241088, (0, 3, 15): 10593241088,
        (1, 1, 1): 3577424896, (1, 1, 15): 3577424896, (1, 3, 1): 10593904896, (1, 3, 15): 10593904896},
    'img_ch1': {
        (0, 1, 1): 3576761088, (0, 1, 15): 3576761088, (0, 3, 1): 10593241088, (0, 3, 15): 10593241088,
        (1, 1, 1): 3577424896, (1, 1, 15): 3577424896, (1, 3, 1): 10593904896, (1, 3, 15): 10593904896},
    'gauss': {
        (0, 1, 1): 3576761088, (0, 1, 15): 3576761088, (0, 3, 1): 10593241088, (0, 3, 15): 10593241088,
        (1, 1, 1): 3577424896, (1, 1, 15): 3577424896, (1, 3, 1): 10593904896, (1, 3, 15): 10593904896},
    'imageless': {
        (0, 1, 1): 308115456, (0, 1, 15): 346876928, (0, 3, 1): 608595456, (0, 3, 15): 882876928, (1, 1, 1): 308115456,
        (1, 1, 15): 353701376, (1, 3, 1): 608595456, (1, 3, 15): 886080768},
    'depth1': {
        (0, 1, 1): 1081608192, (0, 1, 15): 1081608192, (0, 3, 1): 3110488064, (0, 3, 15): 3110488064, (1, 1, 1): 1081608704,
        (1, 1, 15): 1081608704, (1, 3, 1): 3110488576, (1, 3, 15): 3110488576},
    'wide': {
        (0, 1, 1): 2223983872, (0, 1, 15): 2223983872, (0, 3, 1): 6534909184, (0, 3, 15): 6534909184, (1, 1, 1): 2224647680,
        (1, 1, 15): 2224647680, (1, 3, 1): 6535572992, (1, 3, 15): 6535572992},
    'tiny': {
        (0, 1, 1): 137431296, (0, 1, 3): 137431296, (0, 1, 15): 137431296, (0, 3, 1): 140493568, (0, 3, 3): 140493568,
        (0, 3, 15): 140493568, (1, 1, 1): 138500864, (1, 1, 3): 138500864, (1, 1, 15): 138500864, (1, 3, 1): 142875648,
        (1, 3, 3): 142875648, (1, 3, 15): 142875648},
    'one': {
        (0, 1, 1): 193750016, (0, 1, 15): 193750016, (0, 3, 1): 194581760, (0, 3, 15): 194581760, (1, 1, 1): 208674816,
        (1, 1, 15): 208674816, (1, 3, 1): 209835264, (1, 3, 15): 209835264},
}


def test_bytes_is_the_maximum_of_the_parts(hip):
    count = 0
    for key, f in grid():
        total, parts = query(hip, f)
        assert total == 4 * (max(parts.values()) + SLACK_FLOATS), (key, f, total, parts)
        has_image = f['cnn_depth'] >= 1 and f['img'] == 64 and f['img_ch'] >= 1
        for name, v in parts.items():
            if name in CONV_PARTS and not has_image:
                assert v == 0, (key, name, v)
            else:
                assert v >= SPLITK_FLOATS, (key, f, name, v)
        count += 1
    assert count == 7 * 96 + 144          # ('tiny' has a horizon of its own)


def test_never_more_than_the_recorded_formula(hip):
    for key, f in grid():
        total, parts = query(hip, f)
        was = RECORDED[key[0]][key[1:]]
        assert total <= was, f'{key} {f}: {total} bytes, the formula asked for {was} ({parts})'


def test_shapes_the_convolutions_refuse(hip):
    """Image-less and dense-image models report cnn_depth 0 / 1 and any image size: no division by zero, nothing wraps, and a
    geometry the entry points refuse sizes no convolution scratch."""
    for over in (dict(cnn_depth=0, img=0, img_ch=0), dict(cnn_depth=1, img=7, img_ch=3), dict(cnn_depth=1, img=0, img_ch=0),
                 dict(cnn_depth=48, img=32, img_ch=3), dict(cnn_depth=48, img=96, img_ch=3), dict(cnn_depth=48, img=64, img_ch=0),
                 dict(cnn_depth=0, img=64, img_ch=3), dict(cnn_depth=-1, img=64, img_ch=3), dict(cnn_depth=48, img=-64, img_ch=3)):
        f = dict(DEFAULTS, E=1536, flags=0, **over)
        total, parts = query(hip, f)
        assert [parts[k] for k in CONV_PARTS] == [0, 0, 0, 0], (over, parts)
        assert total == 4 * (max(parts.values()) + SLACK_FLOATS) < 1 << 32, (over, total)
    # the dense image path at 64 x 64: the decoder's geometry is one the entry points accept, the encoder's (E != 32) is not
    total, parts = query(hip, dict(DEFAULTS, E=400, flags=0, cnn_depth=1))
    assert parts['enc_fwd'] == parts['enc_bwd'] == 0 and parts['dec_fwd'] > SPLITK_FLOATS
    assert hip.lib().dm_workspace_query(None, None, 0) != 0
    assert hip.lib().dm_workspace_bytes(None) == 0


def test_rollout_part_against_its_restatement(hip):
    """dream_rollout_case.plan_floats() restates RolloutCtx's carving by hand.  The sizing wants every optional block (it cannot
    know the actor's pointers), so the part covers all of them for every case and is exactly their sum where the case takes all."""
    exact = 0
    for name, case in R.CASES.items():
        oconf = R.conf_of(case['kw'])
        c = dict(oconf=oconf, M=case['M'], H=case['H'], D=oconf.deter_dim, Hd=oconf.hidden_dim, S=oconf.stoch_dim,
                 C=oconf.stoch_discrete, A=oconf.action_dim)
        c['Z'] = c['S'] * (c['C'] or 1)
        c['F'] = c['D'] + c['Z']
        kind = R.ACTOR_KINDS[oconf.actor_dist]
        c['AO'] = c['A'] if kind == 0 else 2 * c['A']
        bits = R.plan_bits(oconf, case['M'], case['H'], bf16=case['bf16'])
        assert bits == case['bits'], name
        fl = R.plan_floats(c, keep_acts=False, tw_on=bits['tw_on'])
        want = fl['must'] + fl['wzt'] + fl['wpack'] + fl['add0']
        f = dict(T=1, B=case['M'], I=1, H=case['H'], D=c['D'], Hd=c['Hd'], S=c['S'], C=c['C'], E=256, A=c['A'],
                 mlp_hidden=R.MLP_HIDDEN, mlp_layers=R.MLP_LAYERS, cnn_depth=8, img=64, img_ch=3,
                 flags=kind | (R.GRU_KINDS[oconf.gru_type] << GRU_SHIFT) | ((oconf.gru_layers - 1) << GRU_LAYERS_SHIFT) |
                 (DM_FLAG_BF16 if case['bf16'] else 0))
        part = query(hip, f)[1]['rollout']
        assert part >= want, (name, part, want, fl)
        if bits['wzt'] and bits['actor_wpack'] and bits['actor_add0']:
            assert part == want, (name, part, want, fl)
            exact += 1
    assert exact >= 20
