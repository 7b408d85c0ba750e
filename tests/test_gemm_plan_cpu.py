"""CPU (-m "not gpu"): dm_gemm_plan_query, the planner of dm_gemm_launch asked without a device.

tests/test_gpu_gemm_menu.py pins every (main loop, tile, layout pair) cell to the kernel the MI355X ran, from the profiler's row.
The query runs the same skinny-kernel predicate and the same gemm_plan() as a launch, so the same tables are checked here on any
machine: an edit of the cost model that re-routes a case fails in the CPU suite, by name.
"""
import ctypes
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/gemm_pin.py, tests/gemm_menu_cases.py
import gemm_pin as GP                                # noqa: E402
from gemm_menu_cases import BF16_CASES, F32_CASES, H_CASES, LAYOUTS, UNREACHABLE      # noqa: E402
from test_gpu_gemm_menu import LD_EXTRA, SKINNY_CASES      # noqa: E402

WS_BYTES = 256 << 20           # the workspace of the GPU tests
LOOP_SKINNY = 4
DM_E_SHAPE = -1


def _query(hip, mode, al, bl, M, N, K, epi='none', lda=None, base_align=16):
    """-> (return code, out[8]) for a call shaped like the GPU tests': dense operands (lda = the minor extent unless given),
    ldc = N + LD_EXTRA, the epilogue's flags and addend (dm_gemm_bf16h, mode 2, has no addend)."""
    lda = lda if lda is not None else (K if al == 0 else M)
    ldb = K if bl == 0 else N
    flags = hip.DM_GEMM_ACCUM | hip.DM_GEMM_ELU if epi == 'full' else 0
    out = (ctypes.c_int32 * 8)()
    rc = hip.lib().dm_gemm_plan_query(mode, al, bl, M, N, K, lda, ldb, N + LD_EXTRA, flags, int(epi == 'full' and mode != 2),
                                      base_align, WS_BYTES, out)
    return rc, list(out)


def _cell(al, bl, out):
    """out[8] of a tiled plan -> ((loop, tile, splits) in the tables' names, after the consistency checks of the row)"""
    loop, tile, splits, k_per_split, n_groups, vec, kind, zero = out
    assert 0 <= loop < 4 and 0 <= tile < 5 and splits >= 1 and k_per_split % 32 == 0 and n_groups in (1, 2, 4) and zero == 0
    assert kind == tile * 4 + al * 2 + bl + (24 if loop == 1 else 0) and kind < GP.NKINDS
    return (GP.LOOPS[loop], GP.TILES[tile], splits)


@pytest.fixture
def dma_switch(hip):
    """dm_gemm_dma_enable as a setter; back at the default (1) afterwards"""
    def set_level(level):
        assert hip.lib().dm_gemm_dma_enable(level) == level
    try:
        yield set_level
    finally:
        hip.lib().dm_gemm_dma_enable(1)


def test_f32_table_rows(hip, dma_switch):
    """Every row of F32_CASES under dm_gemm_dma_enable(0), (1) and (2): exactly the (loop, tile, splits) the table names."""
    for level in (0, 1, 2):
        dma_switch(level)
        for al, bl, M, N, K, epi, *expected in F32_CASES:
            rc, out = _query(hip, 0, al, bl, M, N, K, epi)
            assert rc == 0 and out[5] == 1, (level, al, bl, M, N, K, rc, out)
            assert _cell(al, bl, out) == expected[level], f'fp32 {al}{bl} {M}x{N}x{K}, switch {level}: the plan is {_cell(al, bl, out)}'
            assert out[2] == GP.cell(al, bl, expected[level])[4] and out[3] * out[2] >= K > out[3] * (out[2] - 1)


@pytest.mark.parametrize('mode,cases', [(1, BF16_CASES), (2, H_CASES)], ids=['bf16', 'bf16store'])
def test_bf16_table_rows(hip, dma_switch, mode, cases):
    """Every row of BF16_CASES (DM_GEMM_BF16) and H_CASES (dm_gemm_bf16h); the LDS-DMA switch does not reach these loops."""
    for level in (1, 0, 2):
        dma_switch(level)
        for al, bl, M, N, K, epi, expected in cases:
            rc, out = _query(hip, mode, al, bl, M, N, K, epi)
            assert rc == 0 and out[5] == 1, (al, bl, M, N, K, rc, out)
            assert _cell(al, bl, out) == expected, f'mode {mode} {al}{bl} {M}x{N}x{K}, switch {level}: the plan is {_cell(al, bl, out)}'


def test_skinny_cases(hip):
    """The plain dense skinny cases of the menu test's section (c), with and without DM_GEMM_BF16: the query answers skinny."""
    assert len(SKINNY_CASES) > 100
    for (bl, M, N, K, epi, strided), mode in itertools.product(SKINNY_CASES, (0, 1)):
        rc, out = _query(hip, mode, 0, bl, M, N, K, epi, lda=K + 64 if strided else K)
        assert rc == 0 and out == [LOOP_SKINNY, -1, 0, 0, 0, 0, -1, 0], (mode, bl, M, N, K, rc, out)


def test_scalar_load_path(hip, dma_switch):
    """Operand bases that are only 4-byte aligned: the 64x64 register-staged tile with scalar loads, whatever the shape, the
    switch and the DM_GEMM_BF16 flag (the scalar-load variant keeps fp32 operands); bf16 storage refuses such a base."""
    for level in (0, 1, 2):
        dma_switch(level)
        for al, bl, M, N, K, epi, *_ in F32_CASES:
            for mode in (0, 1):
                rc, out = _query(hip, mode, al, bl, M, N, K, epi, base_align=4)
                assert rc == 0 and out[5] == 0, (level, mode, al, bl, M, N, K, rc, out)
                assert _cell(al, bl, out)[:2] == ('regstaged', '64x64')
    al, bl, M, N, K, epi, _ = H_CASES[0]
    assert _query(hip, 2, al, bl, M, N, K, epi, base_align=4)[0] == DM_E_SHAPE
    assert '16-byte aligned' in hip.lib().dm_last_error().decode()


# 24 x 24 x 18 ragged extents (multiples of 4 but not of 32: no tile divides them, all take 16-byte loads), within the
# bounds the comment on UNREACHABLE gives: 36 .. 16388 rows, K up to 131076, products up to 4.5 G multiply-adds
SWEEP_MN = (36, 68, 100, 132, 196, 260, 388, 516, 644, 772, 1028, 1284, 1540, 2052, 2564, 3076, 3588, 4100, 5124, 6148, 8196,
            10244, 12292, 16388)
SWEEP_K = (28, 36, 68, 132, 260, 452, 516, 1028, 2052, 4100, 8196, 16388, 32772, 40004, 65540, 98308, 114692, 131076)


def test_sweep_never_reaches_an_unreachable_cell(hip, dma_switch):
    """No shape of the grid, in any layout pair and precision mode, with the switch at 1 or 2, is planned onto a cell that
    gemm_menu_cases.UNREACHABLE lists (bf16 storage takes extents in multiples of 8: the grid's + 4)."""
    assert len(SWEEP_MN) == 24 and len(SWEEP_K) == 18 and all(x % 4 == 0 and x % 32 != 0 for x in SWEEP_MN + SWEEP_K)
    shapes = [s for s in itertools.product(SWEEP_MN, SWEEP_MN, SWEEP_K) if s[0] * s[1] * s[2] <= 4.5e9]
    assert len(shapes) > 5000
    for level in (1, 2):
        dma_switch(level)
        for mode, (al, bl), (M, N, K) in itertools.product((0, 1, 2), LAYOUTS, shapes):
            if mode == 2:
                M, N, K = M + 4, N + 4, K + 4
            rc, out = _query(hip, mode, al, bl, M, N, K)
            assert rc == 0, (level, mode, al, bl, M, N, K, rc)
            if out[0] != LOOP_SKINNY:
                loop, tile, _ = _cell(al, bl, out)
                assert (loop, tile, al, bl) not in UNREACHABLE, f'switch {level}, mode {mode}: {al}{bl} {M}x{N}x{K} reaches {loop} {tile}'
