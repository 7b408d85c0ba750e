"""The dense GEMM family behind dm_gemm_f32 / dm_gemm_bf16h, one case per kernel, each PINNED to the kernel that answered.

Which kernel runs depends on the shape alone (dm_gemm_launch's cost model, gemm_skinny.hip's shape test), so every case names
the kernel it is meant for and asserts it from the per-launch profiler row (tests/gemm_pin.py): a cost-model change that re-routes
a case fails here by name instead of silently testing another kernel.  The expected kernels in the tables are what the MI355X
reported for these shapes.

  (a) one case per CELL = (main loop, tile, operand-layout pair): 4 loops x 5 tiles x 4 layout pairs, ragged in M, N and K at
      once (no extent a multiple of a tile or of 32, all on the 16-byte-load path), reached by default dispatch on the shape;
  (b) a CPU test that the tables name all 80 cells but the UNREACHABLE ones;
  (c) the skinny kernel (three row-block variants, both grids, both B layouts, M walked in 64-row chunks), pinned by "no row";
  (d) one-hot rows on the tiled loops.

Recipe of every GPU case: asymmetric N(0,1) operands from fixed seeds; fp64 reference on the device (of the bf16-rounded operands
for the bf16 loops); C is a window of a NaN-filled buffer with ldc > N and everything outside the window must still be NaN;
inside, |C - ref| <= 3e-6 * sqrt(K) * 4 (the bound of test_gpu_primitives.py::test_gemm_layouts), and with an epilogue the bound of
test_gemm_dma_equals_register_staged_loop (rtol 2e-6, atol + 1e-5).
"""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # tests/gemm_pin.py
import gemm_pin as GP                                # noqa: E402
from gemm_menu_cases import (BF16_CASES, BF16_SHAPES, EPILOGUES, F32_CASES, H_CASES, H_SHAPES, LAYOUTS,      # noqa: E402,F401
                             UNREACHABLE, _cross)      # the case tables (a), shared with tests/test_gemm_plan_cpu.py

DEV = 'cuda'

# ---------------------------------------------------------------------------------------------------------- (b) coverage, CPU
def _named_cells():
    """(loop, tile, al, bl) -> list of (epilogue, splits) of the cases that name it"""
    cells = {}
    for al, bl, _, _, _, epi, *expected in F32_CASES + BF16_CASES + H_CASES:
        for loop, tile, splits in expected:
            cells.setdefault((loop, tile, al, bl), []).append((epi, splits))
    return cells


def test_tables_name_every_cell():
    """The tables name all 4 x 5 x 4 cells except UNREACHABLE (never a 64x64 one); per tile and loop at least one split-K case
    (K is ragged, so its last slice is shorter than the others), one with the full epilogue and one with bias alone."""
    named = _named_cells()
    every = set((loop, tile, al, bl) for loop in GP.LOOPS for tile in GP.TILES for al, bl in LAYOUTS)
    assert len(every) == 80
    assert all(isinstance(why, str) and why for why in UNREACHABLE.values())
    assert not any(tile == '64x64' for _, tile, _, _ in UNREACHABLE)
    assert not set(UNREACHABLE) & set(named), 'a cell listed as unreachable is named by a case'
    assert set(named) | set(UNREACHABLE) == every, f'cells without a case: {sorted(every - set(named) - set(UNREACHABLE))}'
    for loop, tile in itertools.product(GP.LOOPS, GP.TILES):
        cases = [c for (lp, tl, _, _), cs in named.items() if (lp, tl) == (loop, tile) for c in cs]
        assert any(splits > 1 for _, splits in cases), f'{loop} {tile}: no split-K case'
        assert any(epi == 'full' for epi, _ in cases), f'{loop} {tile}: no case with the full epilogue'
        assert any(epi == 'bias' for epi, _ in cases), f'{loop} {tile}: no bias-only case'
    for al, bl, M, N, K, *_ in F32_CASES + BF16_CASES + H_CASES:      # ragged everywhere, still 16-byte loads
        assert all(x % 32 != 0 and x % 96 != 0 and x % 4 == 0 for x in (M, N, K)), (M, N, K)
    assert all(x % 8 == 0 for _, _, M, N, K, *_ in H_CASES for x in (M, N, K))


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def _ids(cases):
    """layouts-MxNxK-epilogue: the expected kernels stay out of the test id"""
    return [f'{al}{bl}-{M}x{N}x{K}-{epi}' for al, bl, M, N, K, epi, *_ in cases]


PAD_ROWS, PAD_COLS, LD_EXTRA = 1, 8, 16      # the M x N window starts at (1, 8) of an (M + 2) x (N + 16) buffer


@pytest.fixture(scope='module')
def ws():
    return torch.empty(256 << 20, dtype=torch.uint8, device=DEV)


def _randn(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV)


def _nan_window(M, N, dtype=torch.float32, init=None):
    """NaN-filled buffer, the window (optionally preset: DM_GEMM_ACCUM reads it), its device pointer and ldc."""
    big = torch.full((M + 2 * PAD_ROWS, N + LD_EXTRA), float('nan'), device=DEV, dtype=dtype)
    win = big[PAD_ROWS:PAD_ROWS + M, PAD_COLS:PAD_COLS + N]
    if init is not None:
        win.copy_(init)
    ptr = ctypes.c_void_p(big.data_ptr() + (PAD_ROWS * (N + LD_EXTRA) + PAD_COLS) * big.element_size())
    return big, win, ptr, N + LD_EXTRA


def _outside_is_nan(big, M, N):
    inside = torch.zeros(big.shape, dtype=torch.bool, device=DEV)
    inside[PAD_ROWS:PAD_ROWS + M, PAD_COLS:PAD_COLS + N] = True
    return bool(torch.isnan(big[~inside]).all())


def _check(win, ref, K, epi, what):
    """The project's bound (module docstring).  A NaN inside the window fails: the comparison is `not (err <= tol)`."""
    rtol, atol = (0.0, 3e-6 * np.sqrt(K) * 4) if epi == 'none' else (2e-6, 3e-6 * np.sqrt(K) * 4 + 1e-5)
    err = (win.double() - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())
    nbad = int(bad.sum())
    worst = float(torch.nan_to_num(err, nan=float('inf')).max())
    print(f'{what}: max err {worst:.3e}, atol {atol:.3e}, max |ref| {float(ref.abs().max()):.3e}')
    assert nbad == 0, f'{what}: {nbad}/{bad.numel()} mismatches, max err {worst:.3e} (atol {atol:.3e}, rtol {rtol:g})'


def _epilogue(hip, epi, M, N, seed, addend=True):
    """-> bias, addend (ldadd = N + 8), C0, flags for one of EPILOGUES"""
    bias = _randn((N,), seed) if epi != 'none' else None
    add = _randn((M, N + 8), seed + 1) if epi == 'full' and addend else None
    C0 = _randn((M, N), seed + 2) if epi == 'full' else None
    flags = hip.DM_GEMM_ACCUM | hip.DM_GEMM_ELU if epi == 'full' else 0
    return bias, add, C0, flags


def _reference(prod, bias, add, C0, N):
    ref = prod
    if bias is not None:
        ref = ref + bias.double()
    if add is not None:
        ref = ref + add[:, :N].double()
    if C0 is not None:
        ref = F.elu(ref + C0.double())
    return ref


def _f32_call(hip, ws, al, bl, M, N, K, a_ptr, lda, B, bias, add, C0, flags):
    """One dm_gemm_f32 into a fresh NaN window -> (who answered, buffer, window)"""
    big, win, c_ptr, ldc = _nan_window(M, N, init=C0)
    got = GP.pinned(hip, lambda: hip.call('dm_gemm_f32', al, bl, M, N, K, a_ptr, lda, hip.fptr(B), B.shape[1], c_ptr, ldc, hip.fptr(bias),
                                          hip.fptr(add), N + 8, flags, hip.ptr(ws), ws.numel(), hip.stream()), M, N, K)
    return got, big, win


def _operands(al, bl, M, N, K, seed):
    """A (m,k), B (n,k) and the arrays the call reads (layout 1: the transposed copy)"""
    A, B = _randn((M, K), seed), _randn((N, K), seed + 1)
    return A, B, (A if al == 0 else A.t().contiguous()), (B if bl == 0 else B.t().contiguous())


# ------------------------------------------------------------------------------------------------------------- (a) fp32 cells
@pytest.mark.gpu
@pytest.mark.parametrize('al,bl,M,N,K,epi,reg,dflt,dma', F32_CASES, ids=_ids(F32_CASES))
def test_f32_cells(hip, ws, al, bl, M, N, K, epi, reg, dflt, dma):
    """One shape under dm_gemm_dma_enable(0), (2) and the default (1): each run pinned to its cell and checked against fp64.  The
    two loops share the tiles, the k -> MFMA-step map and the epilogue, so runs whose rows name the same tile and split count
    are asserted BIT-IDENTICAL; the default run is identical to whichever forced run took the same kernel."""
    A, B, Ad, Bd = _operands(al, bl, M, N, K, 100)
    bias, add, C0, flags = _epilogue(hip, epi, M, N, 110)
    ref = _reference(A.double() @ B.double().t(), bias, add, C0, N)
    runs = {}
    try:
        for mode, expected in ((0, reg), (2, dma), (1, dflt)):
            assert hip.lib().dm_gemm_dma_enable(mode) == mode
            got, big, win = _f32_call(hip, ws, al, bl, M, N, K, hip.fptr(Ad), Ad.shape[1], Bd, bias, add, C0, flags)
            what = f'fp32 {al}{bl} {M}x{N}x{K} {epi}, switch {mode}'
            print(f'{what}: {got}')
            assert got == GP.cell(al, bl, expected), f'{what}: {got} answered, the table names {expected}'
            assert _outside_is_nan(big, M, N), f'{what}: wrote outside the {M}x{N} window'
            _check(win, ref, K, epi, what)
            runs[mode] = (got, win)
    finally:
        hip.lib().dm_gemm_dma_enable(1)
    if runs[0][0][1] == runs[2][0][1] and runs[0][0][4] == runs[2][0][4]:
        assert torch.equal(runs[0][1], runs[2][1]), f'{int((runs[0][1] != runs[2][1]).sum())} elements differ between the two loops'
    for mode in (0, 2):
        if runs[1][0] == runs[mode][0]:
            assert torch.equal(runs[1][1], runs[mode][1]), f'the default run differs from the same kernel under switch {mode}'


# --------------------------------------------------------------------------------------------------- (a) bf16-operand cells
@pytest.mark.gpu
@pytest.mark.parametrize('al,bl,M,N,K,epi,expected', BF16_CASES, ids=_ids(BF16_CASES))
def test_bf16_operand_cells(hip, ws, al, bl, M, N, K, epi, expected):
    """DM_GEMM_BF16: fp32 operands rounded to bf16 (RNE) on the way into LDS (gemm_pipe_kernel), fp32 accumulation; reference =
    fp64 product of the bf16-rounded operands, so only the fp32 summation order is left: the fp32 bound."""
    A, B, Ad, Bd = _operands(al, bl, M, N, K, 200)
    bias, add, C0, flags = _epilogue(hip, epi, M, N, 210)
    ref = _reference(A.bfloat16().double() @ B.bfloat16().double().t(), bias, add, C0, N)
    got, big, win = _f32_call(hip, ws, al, bl, M, N, K, hip.fptr(Ad), Ad.shape[1], Bd, bias, add, C0, flags | hip.DM_GEMM_BF16)
    what = f'bf16 operands {al}{bl} {M}x{N}x{K} {epi}'
    print(f'{what}: {got}')
    assert got == GP.cell(al, bl, expected), f'{what}: {got} answered, the table names {expected}'
    assert _outside_is_nan(big, M, N), f'{what}: wrote outside the {M}x{N} window'
    _check(win, ref, K, epi, what)


# ---------------------------------------------------------------------------------------------------- (a) bf16-storage cells
@pytest.mark.gpu
@pytest.mark.parametrize('al,bl,M,N,K,epi,expected', H_CASES, ids=_ids(H_CASES))
def test_bf16_storage_cells(hip, ws, al, bl, M, N, K, epi, expected):
    """dm_gemm_bf16h (gemm_h_kernel, 64-k tiles): operands stored as bf16, fp32 accumulation; reference = fp64 product of the
    same bf16 values.  The entry point has no addend: 'full' is bias + DM_GEMM_ACCUM + DM_GEMM_ELU.  With a bias the call also
    writes the bf16 twin (same ldc), which must be exactly RNE(C) inside its window and untouched outside."""
    A, B, Ad, Bd = _operands(al, bl, M, N, K, 300)
    Ad, Bd = Ad.bfloat16(), Bd.bfloat16()
    bias, _, C0, flags = _epilogue(hip, epi, M, N, 310, addend=False)
    ref = _reference(A.bfloat16().double() @ B.bfloat16().double().t(), bias, None, C0, N)
    big, win, c_ptr, ldc = _nan_window(M, N, init=C0)
    hbig, hwin, h_ptr, _ = _nan_window(M, N, dtype=torch.bfloat16)
    got = GP.pinned(hip, lambda: hip.call('dm_gemm_bf16h', al, bl, M, N, K, hip.ptr(Ad), Ad.shape[1], hip.ptr(Bd), Bd.shape[1], c_ptr, ldc,
                                          h_ptr if epi != 'none' else None, hip.fptr(bias), flags, hip.ptr(ws), ws.numel(),
                                          hip.stream()), M, N, K)
    what = f'bf16 storage {al}{bl} {M}x{N}x{K} {epi}'
    print(f'{what}: {got}')
    assert got == GP.cell(al, bl, expected), f'{what}: {got} answered, the table names {expected}'
    assert _outside_is_nan(big, M, N), f'{what}: wrote outside the {M}x{N} window'
    _check(win, ref, K, epi, what)
    assert _outside_is_nan(hbig, M, N), f'{what}: the twin was written outside its window'
    if epi != 'none':
        assert torch.equal(hwin, win.bfloat16()), f'{what}: the bf16 twin is not RNE(C)'
    else:
        assert bool(torch.isnan(hbig).all()), f'{what}: a twin was written though none was asked for'


# -------------------------------------------------------------------------------------------------------- (c) skinny kernel
# N * K >= 65 536 and K % 4 == 0 throughout.  Row-block variants (rows per workgroup) and grids by gemm_skinny.hip's rule, with
# strips = ceil(N / 16): M <= 16 -> 16 rows; 17..64 rows -> `quarters` (16-row workgroups, ceil(M / 16) per strip) while
# ceil(M / 16) * strips <= 256, else for 33..64 rows `halves` (two 32-row workgroups) while 2 * strips <= 256, else one 32- or
# 64-row workgroup per strip; above 64 rows 64-row workgroups walk M in chunks.  N = 1001 (63 strips, the last one ragged)
# takes quarters up to 64 rows, 1800 (113) quarters up to 32 and halves above, 2064 (129) and 4112 (257) neither.
SKINNY_M = (1, 16, 17, 32, 33, 48, 64, 65, 350, 512)
SKINNY_NK = ((1001, 68), (1001, 1000), (1001, 1024), (1800, 600), (2064, 68), (4112, 16))
SKINNY_NK_ONE_CHUNK = ((2064, 1024), (1800, 8192), (4112, 600))      # above 64 rows the kernel keeps K <= 1024, N * K <= 1100 Ki
SKINNY_CASES = [(bl, M, N, K, EPILOGUES[i % 3], i % 2 == 1) for i, (M, (N, K), bl) in enumerate(
    [(M, nk, bl) for M in SKINNY_M for nk in SKINNY_NK + (SKINNY_NK_ONE_CHUNK if M <= 64 else ()) for bl in (0, 1)])]


def _skinny_case(hip, ws, bl, M, N, K, epi, strided, flags=0):
    """Layout-0 A, optionally an offset view with lda > K (a feature-matrix slice) -> (who answered, buffer, window, fp64 ref)"""
    lda = K + 64 if strided else K
    Abig = _randn((M, lda), 400)
    A = Abig[:, 60:60 + K] if strided else Abig                  # 60 floats = 240 bytes: the base stays 16-byte aligned
    a_ptr = ctypes.c_void_p(Abig.data_ptr() + (60 * 4 if strided else 0))
    B = _randn((N, K), 401)
    Bd = B if bl == 0 else B.t().contiguous()
    bias, add, C0, eflags = _epilogue(hip, epi, M, N, 410)
    ref = _reference(A.double() @ B.double().t(), bias, add, C0, N)
    got, big, win = _f32_call(hip, ws, 0, bl, M, N, K, a_ptr, lda, Bd, bias, add, C0, eflags | flags)
    return got, big, win, ref


@pytest.mark.gpu
@pytest.mark.parametrize('bl,M,N,K,epi,strided', SKINNY_CASES)
def test_skinny_kernel(hip, ws, bl, M, N, K, epi, strided):
    """gemm_skinny.hip, pinned by "DM_OK and no profiler row": every row-block variant and grid, both B layouts, the ragged
    last strip, the epilogue and lda / ldc / ldadd handling, 64-row chunks of M up to 512."""
    got, big, win, ref = _skinny_case(hip, ws, bl, M, N, K, epi, strided)
    what = f'skinny 0{bl} {M}x{N}x{K} {epi}{" lda>K" if strided else ""}'
    assert got == GP.SKINNY, f'{what}: {got} answered, not the skinny kernel'
    assert _outside_is_nan(big, M, N), f'{what}: wrote outside the {M}x{N} window'
    _check(win, ref, K, epi, what)


@pytest.mark.gpu
@pytest.mark.parametrize('bl,M,N,K,expected', [
    # 512 rows are the skinny kernel's last, 513 go to a tile (N = 1001 as a row-contiguous B has no 16-byte loads: scalar 64x64)
    (0, 512, 1001, 1000, GP.SKINNY), (1, 512, 1001, 1000, GP.SKINNY),
    (0, 513, 1001, 1000, ('dma', '64x64', 1)), (1, 513, 1001, 1000, ('regstaged', '64x64', 1)),
    # N * K = 65 704 >= 64 Ki is skinny, 65 532 is not
    (0, 50, 382, 172, GP.SKINNY), (1, 50, 382, 172, GP.SKINNY),
    (0, 50, 381, 172, ('regstaged', '64x64', 1)), (1, 50, 381, 172, ('regstaged', '64x64', 1)),
    # above 64 rows K = 1024 is the longest skinny reduction (N * K stays under 1100 Ki on both sides)
    (0, 65, 1001, 1024, GP.SKINNY), (1, 65, 1001, 1024, GP.SKINNY),
    (0, 65, 1001, 1028, ('regstaged', '64x64', 7)), (1, 65, 1001, 1028, ('regstaged', '64x64', 7)),
])
def test_skinny_boundaries(hip, ws, bl, M, N, K, expected):
    """Each limit of the skinny kernel's shape test from both sides: the neighbours take different kernels and both are right."""
    got, big, win, ref = _skinny_case(hip, ws, bl, M, N, K, 'none', False)
    what = f'boundary 0{bl} {M}x{N}x{K}'
    print(f'{what}: {got}')
    assert got == GP.cell(0, bl, expected), f'{what}: {got} answered, the table names {expected}'
    assert _outside_is_nan(big, M, N), f'{what}: wrote outside the {M}x{N} window'
    _check(win, ref, K, 'none', what)


@pytest.mark.gpu
@pytest.mark.parametrize('bl', [0, 1])
def test_skinny_keeps_fp32_operands_under_the_bf16_flag(hip, ws, bl):
    """DM_GEMM_BF16 on a skinny-eligible shape: the skinny kernel still answers and it keeps fp32 operands (the flag asks for
    bf16 OPERAND ROUNDING only where a tile kernel runs; the chains' <= 64-row products stay fp32 under conf.amp).  So the
    result meets the fp32 bound against the fp64 product of the UNROUNDED operands, which a bf16-rounded product misses by
    two orders of magnitude."""
    M, N, K = 50, 1000, 1024
    got, big, win, ref = _skinny_case(hip, ws, bl, M, N, K, 'none', False, flags=hip.DM_GEMM_BF16)
    assert got == GP.SKINNY, f'{got} answered, not the skinny kernel'
    assert _outside_is_nan(big, M, N)
    _check(win, ref, K, 'none', f'skinny 0{bl} {M}x{N}x{K} with DM_GEMM_BF16')


# ----------------------------------------------------------------------------------------- (d) one-hot rows on the tiled loops
@pytest.mark.gpu
@pytest.mark.parametrize('N,expected', [(1000, ('dma', '64x64', 1)), (3588, ('dma', '128x96', 1)), (4100, ('dma', '128x128', 1))])
def test_onehot_rows_on_tiles(hip, ws, N, expected):
    """test_gpu_primitives.py::test_gemm_onehot_rows_exact's construction at the imagination batch's 2 500 rows, where a tile
    kernel answers: one-hot A rows (32 groups of 32) against the fp64 sum of the selected weight columns."""
    M, S, C = 2500, 32, 32
    K = S * C
    g = torch.Generator().manual_seed(10)
    idx = torch.randint(0, C, (M, S), generator=g)
    A = F.one_hot(idx, C).float().reshape(M, K).to(DEV)
    W = _randn((N, K), 500)
    cols = (idx + torch.arange(S) * C).to(DEV)          # (M,S) selected columns, ascending in k
    ref = torch.zeros(M, N, device=DEV, dtype=torch.float64)
    Wt = W.double().t().contiguous()
    for s in range(S):
        ref += Wt[cols[:, s]]
    got, big, win = _f32_call(hip, ws, 0, 0, M, N, K, hip.fptr(A), K, W, None, None, None, 0)
    what = f'one-hot {M}x{N}x{K}'
    print(f'{what}: {got}')
    assert got == GP.cell(0, 0, expected), f'{what}: {got} answered, the table names {expected}'
    assert _outside_is_nan(big, M, N), f'{what}: wrote outside the {M}x{N} window'
    _check(win, ref, K, 'none', what)
