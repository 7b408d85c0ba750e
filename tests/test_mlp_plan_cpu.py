"""CPU (-m "not gpu"): dm_mlp_plan_query, the plan of the MLP heads' forward and backward asked without a device.

tests/test_gpu_mlp_windows.py pins the kernel that answered each window on the MI355X; the query runs the same mlp_fwd_plan /
mlp_bwd_plan as a call (csrc/mlp.hip), so the dispatch table, the sparse-tail and bf16-copy rules, the fall-back under a tight
workspace and the bound dm_mlp_ws_floats promises every caller are checked here on any machine.
"""
import ctypes
import itertools

PANEL, CHAIN, PER_LAYER = 0, 1, 2
ADD_NONE, ADD_HERE, ADD_CALLER = 0, 1, 2
DM_E_SHAPE, DM_E_WORKSPACE = -1, -2
SPLITK_FLOATS = 16 * 1024 * 1024
PLENTY = 1 << 40                    # bytes: room for every optional piece at any shape below
FWD, BWD = 0, 1


def _query(hip, rows, which=FWD, in_dim=136, hidden=400, layers=4, out_dim=6, ldx=None, sparse_cols=0, base_align=16, normed=1,
           precision=0, has_acts=1, has_wpack=0, has_add0=0, has_sample=0, ws_bytes=PLENTY):
    """-> (return code, dict of out[8]); ldx defaults to in_dim"""
    out = (ctypes.c_int32 * 8)()
    rc = hip.lib().dm_mlp_plan_query(which, rows, in_dim, hidden, layers, out_dim, in_dim if ldx is None else ldx, sparse_cols,
                                     base_align, normed, precision, has_acts, has_wpack, has_add0, has_sample, ws_bytes, out)
    path, k0, addend, packs, copies, fuse_out, lo, hi = list(out)
    return rc, dict(path=path, k0=k0, addend=addend, packs=packs, copies=copies, fuse_out=fuse_out,
                    need=(lo & 0xFFFFFFFF) | ((hi & 0xFFFFFFFF) << 32))


def _ok(hip, rows, **kw):
    rc, r = _query(hip, rows, **kw)
    assert rc == 0, (rows, kw, rc, hip.lib().dm_last_error())
    return r


DISPATCH = [
    (255, {}, PER_LAYER), (256, {}, CHAIN), (16383, {}, CHAIN), (16384, {}, PANEL),
    (300, dict(out_dim=32), CHAIN), (300, dict(out_dim=33), PER_LAYER), (300, dict(in_dim=138), PER_LAYER),
    (300, dict(ldx=137), PER_LAYER), (300, dict(base_align=4), PER_LAYER), (300, dict(hidden=200), PER_LAYER),
    (300, dict(normed=0), PER_LAYER),
    (16400, dict(ldx=137), PANEL),                  # the panels keep scalar loads
    (16400, dict(in_dim=138), PER_LAYER), (16400, dict(base_align=4), PER_LAYER), (16400, dict(normed=0), PER_LAYER),
]


def test_dispatch_table(hip):
    """hidden 400, 4 layers, LayerNorm, fp32, 16-byte bases, ldx = in_dim = 136 unless the row says otherwise."""
    assert hip.lib().dm_mlp_chain_min_rows(0) == 256
    for has_acts in (1, 0):
        for rows, kw, path in DISPATCH:
            assert _ok(hip, rows, has_acts=has_acts, **kw)['path'] == path, (rows, kw, has_acts)
    r = _ok(hip, 16400, out_dim=32)
    assert (r['path'], r['fuse_out']) == (PANEL, 1)
    r = _ok(hip, 16400, out_dim=33)
    assert (r['path'], r['fuse_out']) == (PANEL, 0)
    try:
        assert hip.lib().dm_mlp_chain_min_rows(1024) == 256
        assert _ok(hip, 300)['path'] == PER_LAYER
        assert _ok(hip, 1024)['path'] == CHAIN
    finally:
        hip.lib().dm_mlp_chain_min_rows(256)
    assert _ok(hip, 300)['path'] == CHAIN


def test_backward_dispatch(hip):
    """The backward has two paths: row panels from 16 384 rows at hidden 400 (LayerNorm, 16-byte output weights), else per layer."""
    for rows, kw, path in [(16383, {}, PER_LAYER), (16384, {}, PANEL), (16400, dict(base_align=4), PER_LAYER),
                           (16400, dict(normed=0), PER_LAYER), (16400, dict(hidden=200), PER_LAYER), (300, {}, PER_LAYER)]:
        assert _ok(hip, rows, which=BWD, **kw)['path'] == path, (rows, kw)
    assert _ok(hip, 16400, which=BWD, precision=1)['copies'] == 1
    assert _ok(hip, 16400, which=BWD, precision=1, layers=1)['copies'] == 0
    assert _ok(hip, 16400, which=BWD)['copies'] == 0
    assert _query(hip, 300, which=BWD, layers=9)[0] == DM_E_SHAPE


def test_sparse_tail(hip):
    """in_dim 136; 300 rows = the whole-MLP kernel, 16 400 rows = the row panels."""
    for rows, path in ((300, CHAIN), (16400, PANEL)):
        r = _ok(hip, rows, sparse_cols=64)
        assert (r['path'], r['k0'], r['addend']) == (path, 72, ADD_HERE), r
        assert r['packs'] == (path == CHAIN) and r['copies'] == 0
        r = _ok(hip, rows, sparse_cols=64, precision=1)                    # bf16 operands: the product is cheaper than the gather
        assert (r['path'], r['k0'], r['addend'], r['copies']) == (path, 136, ADD_NONE, int(path == PANEL)), r
        for sp in (112, 60):                                               # dense 24 < 32; dense 76: not a multiple of 8
            r = _ok(hip, rows, sparse_cols=sp)
            assert (r['path'], r['k0'], r['addend']) == (path, 136, ADD_NONE), (sp, r)
        r = _ok(hip, rows, in_dim=4104, sparse_cols=64)                    # wider than the 4096 columns dm_mlp_ws_floats sizes for
        assert (r['path'], r['k0'], r['addend']) == (path, 4104, ADD_NONE), r
        r = _ok(hip, rows, in_dim=4104, precision=1)
        assert (r['path'], r['copies']) == (path, 0), r
        r = _ok(hip, rows, sparse_cols=0)
        assert (r['k0'], r['addend']) == (136, ADD_NONE)
        for sp in (136, 137, -1):
            assert _query(hip, rows, sparse_cols=sp)[0] == DM_E_SHAPE, sp
            assert b'sparse_cols' in hip.lib().dm_last_error()
    r = _ok(hip, 300, sparse_cols=64, ldx=140)                             # a padded row stride keeps the split
    assert (r['path'], r['k0'], r['addend']) == (CHAIN, 72, ADD_HERE), r
    r = _ok(hip, 16400, sparse_cols=64, ldx=137)                           # the gather reads x in 16-byte pieces
    assert (r['path'], r['k0'], r['addend']) == (PANEL, 136, ADD_NONE), r


def test_callers_pieces(hip):
    """DmMlpFwd's wpack / add0 / sample, the imagination rollout's: their coupling rules are errors of the plan."""
    r = _ok(hip, 300, sparse_cols=64, has_wpack=1, has_add0=1)
    assert (r['path'], r['k0'], r['addend'], r['packs']) == (CHAIN, 72, ADD_CALLER, 0), r
    r = _ok(hip, 300, sparse_cols=64, has_wpack=1)                          # packed for all columns: no split
    assert (r['path'], r['k0'], r['addend'], r['packs']) == (CHAIN, 136, ADD_NONE, 0), r
    r = _ok(hip, 300, sparse_cols=60, has_wpack=1, has_add0=1)              # the split does not apply: the addend is not used
    assert (r['k0'], r['addend']) == (136, ADD_NONE), r
    assert _ok(hip, 300, has_sample=1, has_wpack=1)['path'] == CHAIN
    assert _query(hip, 300, sparse_cols=64, has_add0=1)[0] < 0              # an addend without the weights packed for it
    assert b'addend' in hip.lib().dm_last_error()
    for rows in (16400, 200):
        assert _query(hip, rows, has_sample=1, has_wpack=1)[0] == DM_E_SHAPE
        assert b'fused sampler' in hip.lib().dm_last_error()


def _steps(hip, piece, rows, **kw):
    """Lower ws_bytes over the steps the query itself names: the optional `piece` goes first, the call last."""
    full = 4 * hip.lib().dm_mlp_ws_floats(rows, kw.get('hidden', 400), kw.get('layers', 4))
    a = _ok(hip, rows, ws_bytes=full, **kw)
    assert a[piece] == 1 and SPLITK_FLOATS < a['need'] <= full // 4, a
    assert _ok(hip, rows, ws_bytes=4 * a['need'], **kw) == a                 # an exact fit keeps the piece
    b = _ok(hip, rows, ws_bytes=4 * a['need'] - 4, **kw)
    assert b[piece] == 0 and b['copies'] == 0 and b['addend'] == ADD_NONE and b['path'] == a['path'], b
    assert b['k0'] == kw.get('in_dim', 136) and SPLITK_FLOATS <= b['need'] < a['need'], b
    assert _ok(hip, rows, ws_bytes=4 * b['need'], **kw) == b
    rc, _ = _query(hip, rows, ws_bytes=4 * b['need'] - 4, **kw)
    assert rc == DM_E_WORKSPACE, (rc, b)
    assert b'workspace too small' in hip.lib().dm_last_error()
    return a, b


def test_fallback_under_a_tight_workspace(hip):
    for has_acts in (0, 1):
        a, b = _steps(hip, 'addend', 300, sparse_cols=64, has_acts=has_acts)
        assert (a['path'], a['k0'], b['packs']) == (CHAIN, 72, 1)
        # without an activation set the ping-pong prefix is mandatory; with one, only the split-K region is
        assert (b['need'] == SPLITK_FLOATS) == bool(has_acts)
        a, b = _steps(hip, 'copies', 16400, precision=1, has_acts=has_acts)
        assert a['path'] == PANEL and (b['need'] == SPLITK_FLOATS) == bool(has_acts)
        a, b = _steps(hip, 'addend', 16400, sparse_cols=64, has_acts=has_acts)
        assert (a['path'], a['k0']) == (PANEL, 72)
    a, b = _steps(hip, 'copies', 16400, which=BWD, precision=1)
    assert a['path'] == PANEL


BOUND_ROWS = (1, 63, 64, 255, 256, 300, 2500, 16383, 16384, 16400, 40000, 100000)


def test_ws_floats_bounds_every_layout(hip):
    """need_floats of every plan, given room for every optional piece, is at most dm_mlp_ws_floats(rows, hidden, layers)."""
    lib = hip.lib()
    grid = [(400, layers) for layers in (1, 4, 8)] + [(64, 4), (1000, 4)]
    count, paths, pieces = 0, set(), set()
    for (hidden, layers), rows, in_dim, sp, prec, has_acts, which in itertools.product(
            grid, BOUND_ROWS, (4, 136, 632, 1624, 4096), (0, 64, 1024), (0, 1), (0, 1), (FWD, BWD)):
        rc, r = _query(hip, rows, which=which, in_dim=in_dim, hidden=hidden, layers=layers, sparse_cols=sp, precision=prec,
                       has_acts=has_acts)
        if rc != 0:
            assert rc == DM_E_SHAPE and sp >= in_dim and which == FWD, (rc, rows, in_dim, hidden, layers, sp, prec, has_acts, which)
            continue
        if hidden != 400:
            assert r['path'] == PER_LAYER
        bound = lib.dm_mlp_ws_floats(rows, hidden, layers)
        assert r['need'] <= bound, f'{"bwd" if which else "fwd"} rows {rows} in_dim {in_dim} hidden {hidden} layers {layers} ' \
            f'sparse {sp} precision {prec} acts {has_acts}: the plan needs {r["need"]} floats, dm_mlp_ws_floats says {bound} ({r})'
        count += 1
        paths.add((which, r['path']))
        pieces.add((which, r['addend'], r['copies']))
    assert count > 5000
    assert paths == {(FWD, PANEL), (FWD, CHAIN), (FWD, PER_LAYER), (BWD, PANEL), (BWD, PER_LAYER)}
    assert pieces == {(FWD, ADD_NONE, 0), (FWD, ADD_HERE, 0), (FWD, ADD_NONE, 1), (BWD, ADD_NONE, 0), (BWD, ADD_NONE, 1)}


# (rows, hidden, layers) -> (dm_mlp_ws_floats, dm_mlp_acts_floats), recorded before the launcher was split into plan and paths
RECORDED = {
    (2500, 400, 4): (23907136, 8020224),
    (40000, 400, 4): (86715136, 128320000),
    (1, 400, 1): (19478144, 960),
    (16700, 400, 4): (47687936, 53573632),
    (300, 400, 4): (20219136, 962560),
    (16384, 400, 8): (48707136, 105119744),
    (255, 64, 2): (17245760, 66304),
    (100000, 400, 4): (187217536, 320800000),
    (700, 1000, 3): (28320704, 4204416),
    (63, 400, 8): (20145600, 404480),
    (0, 400, 4): (19715136, 0),
    (5, 400, 9): (0, 0),                     # more layers than DM_MAX_MLP_LAYERS
}


def test_workspace_sizes_unchanged(hip):
    for shape, (ws, acts) in RECORDED.items():
        assert hip.lib().dm_mlp_ws_floats(*shape) == ws, shape
        assert hip.lib().dm_mlp_acts_floats(*shape) == acts, shape
