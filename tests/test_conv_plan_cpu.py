"""CPU (-m "not gpu"): dm_conv_plan_query, the per-layer plans of the convolution encoder and decoder asked without a device.

tests/conv_plan_cases.py writes out by hand which form every layer takes at every (cnn_depth, channels) the GPU suites run
(tests/test_gpu_conv_stack.py CASES, tests/test_gpu_convt_kskip.py DEPTHS).  Here: the library's plans are that table at every
frame count of those suites; the bf16-stored gather operand (hpath), the k-tile lists (kskip) and the image layer's direct
backward follow their flags and switches; the 2^31 bound of the gather form; every plan's workspace need against its part of
dm_workspace_query; and DM_E_SHAPE for the geometries the entry points refuse.  Nothing is allocated or launched.
"""
import ast
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/conv_plan_cases.py
import conv_plan_cases as PC                         # noqa: E402

DM_E_SHAPE = -1
WHICH = (PC.ENC_FWD, PC.ENC_BWD, PC.DEC_FWD, PC.DEC_BWD)
HPATH = PC.BITS['hpath'] << 8


def _codes(case):
    return [tuple(PC.code(t) for t in row) for row in (case.enc_fwd, case.enc_bwd, case.dec_fwd, case.dec_bwd)]


def _plans(hip, shp, planes=0):
    """-> ([codes of the four plans], [kskip], [need])"""
    got = [PC.query(hip, which, shp, planes) for which in WHICH]
    assert all(rc == 0 for rc, *_ in got), hip.lib().dm_last_error()
    return [g[1] for g in got], [g[2] for g in got], [g[3] for g in got]


def _parts(hip, shp):
    parts = (ctypes.c_size_t * 8)()
    assert hip.lib().dm_workspace_query(ctypes.byref(shp), parts, 8) == 0
    return [int(v) for v in parts[:4]]


class _Switch:
    """with _Switch(lib.dm_..._enable, value): the switch holds `value` inside and its earlier state afterwards"""

    def __init__(self, fn, value):
        self.fn, self.value = fn, value

    def __enter__(self):
        self.before = self.fn(-1)
        self.fn(self.value)

    def __exit__(self, *exc):
        self.fn(self.before)


def _assigned(path, name):
    """the literal assigned to `name` at the top level of a test module, without importing it (it wants a GPU)"""
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), path)).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], 'id', None) == name:
            return eval(compile(ast.Expression(node.value), path, 'eval'))      # noqa: S307 (the repository's own file)
    raise KeyError(name)


def test_table_covers_the_gpu_suites_and_follows_its_rules():
    stack = _assigned('test_gpu_conv_stack.py', 'CASES')
    assert len(stack) == 19
    for depth, ch, frames in stack:
        assert frames in PC.BY_KEY[(depth, ch)].frames, (depth, ch, frames)
    for depth in _assigned('test_gpu_convt_kskip.py', 'DEPTHS'):
        assert set(_assigned('test_gpu_convt_kskip.py', 'FRAMES')) <= set(PC.BY_KEY[(depth, 3)].frames)
    for c in PC.CASES:
        assert (c.enc_fwd, c.enc_bwd, c.dec_fwd, c.dec_bwd) == PC.rule(c.depth, c.ch), (c.depth, c.ch)
    # what the GPU suites' docstrings say about these depths
    gathers = lambda c: [(n, l) for n, row in (('enc_bwd', c.enc_bwd), ('dec_fwd', c.dec_fwd)) for l, t in enumerate(row) if t == 'gather']
    assert gathers(PC.BY_KEY[(6, 3)]) == []
    assert gathers(PC.BY_KEY[(12, 3)]) == [('enc_bwd', 2)]
    for depth in (16, 24):      # decoder layer 3 forward (index 2 of layers 1..4), the encoder's layer-3 and layer-2 data gradients
        assert gathers(PC.BY_KEY[(depth, 3)]) == [('enc_bwd', 1), ('enc_bwd', 2), ('dec_fwd', 2)]
    assert PC.BY_KEY[(6, 3)].dec_bwd[2:] == ('implicit+padded', 'implicit+padded+repitch')


@pytest.mark.parametrize('case', PC.CASES, ids=lambda c: f'd{c.depth}-c{c.ch}')
def test_plans_are_the_table(hip, case):
    """fp32, default switches, every frame count the GPU suites run at this (depth, channels): the four plans are the table's rows,
    kskip is on for the two entry points that have gather layers to speak of, and each need is its part of dm_workspace_query
    (the encoder forward's part sizes the reward_input variant wherever the shape admits it)."""
    want = _codes(case)
    planes = int(case.enc_fwd[0] == 'direct')
    for frames in case.frames:
        shp = PC.shape(hip, case.depth, case.ch, frames)
        codes, kskip, need = _plans(hip, shp)
        assert codes == want, (frames, codes, want)
        assert kskip == [0, 1, 1, 0]
        parts = _parts(hip, shp)
        assert need[1:] == parts[1:] and need[0] <= parts[0], (frames, need, parts)
        if planes:
            codes_p, _, need_p = _plans(hip, shp, planes=1)
            assert codes_p[0] == want[0] and codes_p[1] == (PC.code('direct+planes'),) + want[1][1:] and codes_p[2:] == want[2:]
            assert need_p == parts, (frames, need_p, parts)
        else:
            assert need[0] == parts[0]
            assert PC.query(hip, PC.ENC_FWD, shp, planes=1)[0] == PC.query(hip, PC.ENC_BWD, shp, planes=1)[0] == DM_E_SHAPE


@pytest.mark.parametrize('case', PC.CASES, ids=lambda c: f'd{c.depth}-c{c.ch}')
def test_bf16_hpath_kskip_and_twins(hip, case):
    """DM_FLAG_BF16: same forms, no k-tile lists, and the bf16-stored gather operand only where K >= 1024 - of these depths at
    depth 64 alone, decoder layer 3 (K = 9 * 128) and the encoder data gradient out of layer 2 (K = 4 * 256), not out of layer 1
    (K = 512).  Needs are the parts of dm_workspace_query; with dm_bf16_twins_enable(0) no hpath and a smaller need."""
    lib = hip.lib()
    want = _codes(case)
    if case.depth == 64:
        want[1] = (want[1][0], want[1][1], want[1][2] | HPATH, want[1][3])
        want[2] = (want[2][0], want[2][1], want[2][2] | HPATH, want[2][3])
    shp = PC.shape(hip, case.depth, case.ch, 131, flags=hip.DM_FLAG_BF16)
    codes, kskip, need = _plans(hip, shp, planes=int(case.enc_fwd[0] == 'direct'))
    if case.enc_fwd[0] == 'direct':
        want[1] = (PC.code('direct+planes'),) + want[1][1:]
    assert codes == want, (codes, want)
    assert kskip == [0, 0, 0, 0]
    assert need == _parts(hip, shp)
    with _Switch(lib.dm_bf16_twins_enable, 0):
        off, _, need_off = _plans(hip, shp, planes=int(case.enc_fwd[0] == 'direct'))
        assert off == [tuple(v & ~HPATH for v in row) for row in want]
        # (the decoder forward's only twin is the gather form's weight copy: none where it has no gather layer)
        assert need_off[0] == need[0] and need_off[1] < need[1] and need_off[3] < need[3], (need_off, need)
        assert (need_off[2] < need[2]) if 'gather' in case.dec_fwd else (need_off[2] == need[2]), (need_off, need)
    assert lib.dm_bf16_twins_enable(-1) == 1
    fp32 = _plans(hip, PC.shape(hip, case.depth, case.ch, 131))[0]
    assert not any(v & HPATH for row in fp32 for v in row)


def test_kskip_switch(hip):
    lib = hip.lib()
    shp = PC.shape(hip, 48, 3, 131)
    assert _plans(hip, shp)[1] == [0, 1, 1, 0]
    with _Switch(lib.dm_convt_kskip_enable, 0):
        codes, kskip, need = _plans(hip, shp)
        assert kskip == [0, 0, 0, 0] and codes == _codes(PC.BY_KEY[(48, 3)])
        assert need[1:] == _parts(hip, shp)[1:]          # the lists are sized whether or not the switch is on
    assert lib.dm_convt_kskip_enable(-1) == 1 and _plans(hip, shp)[1] == [0, 1, 1, 0]


@pytest.mark.parametrize('depth,ch', [(48, 3), (8, 3), (24, 3), (48, 1)])
def test_image_layer_backward_switch(hip, depth, ch):
    """dm_dec_l4_bwd_direct_enable(0): the image layer's backward is implicit + padded at every shape, nothing else moves, and
    where that removes the direct kernels' scratch the need is smaller - never larger - than the part."""
    lib = hip.lib()
    shp = PC.shape(hip, depth, ch, 131)
    on, _, need_on = _plans(hip, shp)
    with _Switch(lib.dm_dec_l4_bwd_direct_enable, 0):
        off, _, need_off = _plans(hip, shp)
    assert lib.dm_dec_l4_bwd_direct_enable(-1) == 1
    assert off[:3] == on[:3] and off[3] == on[3][:3] + (PC.code('implicit+padded'),)
    assert need_off[:3] == need_on[:3]
    direct = PC.BY_KEY[(depth, ch)].dec_bwd[3].startswith('direct')
    assert (need_off[3] < need_on[3]) if direct else (need_off[3] == need_on[3])
    assert need_on == [min(a, b) for a, b in zip(need_on, _parts(hip, shp))]


def test_gather_form_stops_at_2_to_the_31(hip):
    """convt_gather_ok: the scattered output (n, 31, 31, 48) must stay under 2^31 elements - 46 554 frames at depth 48 still plan
    the gather form for the encoder data gradient out of layer 1 and for decoder layer 3, 46 555 plan the column form; the layer-2
    data gradient (n, 15, 15, 96) is far from the bound.  The query computes sizes only."""
    assert 961 * 48 * 46554 < 2 ** 31 <= 961 * 48 * 46555
    G, C = PC.code('gather'), PC.code('column')
    for frames, form in ((46554, G), (46555, C)):
        for T, B, I in ((1, frames, 1), (frames, 1, 1)) + (((15518, 1, 3),) if frames == 46554 else ((9311, 1, 5),)):
            assert T * B * I == frames
            codes, _, need = _plans(hip, PC.shape(hip, 48, 3, frames, T=T, B=B, I=I))
            assert codes[1] == (PC.code('direct'), form, G, C), (frames, codes[1])
            assert codes[2] == (PC.code('one_pixel'), C, form, PC.code('direct')), (frames, codes[2])
            assert all(n > 16 * 1024 * 1024 for n in need)


REFUSED = (dict(cnn_depth=0, img=0, img_ch=0), dict(cnn_depth=1, img=7, img_ch=3), dict(cnn_depth=1, img=0, img_ch=0),
           dict(cnn_depth=48, img=32, img_ch=3), dict(cnn_depth=48, img=96, img_ch=3), dict(cnn_depth=48, img=64, img_ch=0),
           dict(cnn_depth=0, img=64, img_ch=3), dict(cnn_depth=-1, img=64, img_ch=3), dict(cnn_depth=48, img=-64, img_ch=3))


def test_refused_geometries(hip):
    """The shapes of test_workspace_cpu.py::test_shapes_the_convolutions_refuse: DM_E_SHAPE from every plan, as from the entry
    points; the dense image path at 64 x 64 (E != 32 cnn_depth) has decoder plans and no encoder plans."""
    lib = hip.lib()
    for over in REFUSED:
        shp = PC.shape(hip, 48, 3, 2500, E=1536, **over)
        assert _parts(hip, shp) == [0, 0, 0, 0]
        for which in WHICH:
            assert PC.query(hip, which, shp)[0] == DM_E_SHAPE, (over, which)
    dense = PC.shape(hip, 1, 3, 2500, E=400)
    assert [PC.query(hip, which, dense)[0] for which in WHICH] == [DM_E_SHAPE, DM_E_SHAPE, 0, 0]
    assert lib.dm_conv_plan_query(4, ctypes.byref(dense), 0, (ctypes.c_int32 * 8)(), None) == DM_E_SHAPE
    assert lib.dm_conv_plan_query(0, None, 0, (ctypes.c_int32 * 8)(), None) != 0
    assert lib.dm_conv_plan_query(2, ctypes.byref(dense), 0, (ctypes.c_int32 * 8)(), None) == 0      # the need is optional
