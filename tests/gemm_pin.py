"""Which kernel answered a dm_gemm_f32 / dm_gemm_bf16h call: the per-launch rows of dm_prof_begin / dm_prof_rows / dm_prof_end,
decoded.  Shared by test_gpu_primitives.py and test_gpu_gemm_menu.py.  Not a test module.

dm_gemm_launch records one row per tiled launch: kind = tile * 4 + a_layout * 2 + b_layout (+ 24 on the LDS-DMA loop), M, N, K,
split count, flags (8 = bf16 operands, 32 = bf16 storage).  The skinny kernel (gemm_skinny.hip) records none, so "the call
returned DM_OK with M, N > 0 and no row was recorded" is its pin.  The row does not say whether the 16-byte-load or the scalar-load
instantiation of the 64x64 tile ran: that follows from the alignment of the call, which the caller knows.
"""
import ctypes

import torch

TILES = ('128x128', '128x64', '64x64', '128x96', '96x128')
LOOPS = ('regstaged', 'dma', 'bf16', 'bf16store')
SKINNY = 'skinny'
FLAG_BF16, FLAG_BF16_STORAGE = 8, 32
NKINDS = 44


def profiled_rows(hip, fn, cap=64):
    """Run fn() with the per-launch profiler armed; return its rows as (kind, M, N, K, splits, flags) tuples of ints.
    Profiling is switched off again whatever fn does."""
    hip.call('dm_prof_begin', cap)
    try:
        fn()
        torch.cuda.synchronize()
        rows = (ctypes.c_double * (8 * cap))()
        n = hip.lib().dm_prof_rows(rows, cap)
    finally:
        out = (ctypes.c_double * (4 * NKINDS))()
        hip.lib().dm_prof_end(out, NKINDS)
    assert 0 <= n < cap, f'dm_prof_rows returned {n} (capacity {cap})'
    return [tuple(int(rows[8 * i + j]) for j in range(6)) for i in range(n)]


def decode(row):
    """(kind, M, N, K, splits, flags) -> (loop, tile, a_layout, b_layout, splits, flags)"""
    kind, _, _, _, splits, flags = row
    dma = kind >= 24
    k = kind - 24 if dma else kind
    assert 0 <= k < 20 and kind < NKINDS, f'row {row}: kind {kind} is not a GEMM tile kernel'
    if flags & FLAG_BF16_STORAGE:
        loop = 'bf16store'
    elif flags & FLAG_BF16:
        loop = 'bf16'
    else:
        loop = 'dma' if dma else 'regstaged'
    assert not (dma and loop != 'dma'), f'row {row}: the LDS-DMA loop serves fp32 products only'
    return (loop, TILES[k // 4], (k >> 1) & 1, k & 1, splits, flags)


def pinned(hip, fn, M, N, K):
    """Run ONE product of M x N x K (fn makes exactly one hip.call of dm_gemm_f32 / dm_gemm_bf16h, which raises unless it
    returns DM_OK) and say who answered: SKINNY, or the decoded row of the tile kernel."""
    assert M > 0 and N > 0
    rows = profiled_rows(hip, fn)
    if not rows:
        return SKINNY
    assert len(rows) == 1, f'one product, {len(rows)} rows: {rows}'
    assert rows[0][1:4] == (M, N, K), f'row {rows[0]} is not the {M}x{N}x{K} product'
    return decode(rows[0])


def cell(al, bl, expected):
    """Expected kernel of a table, ('loop', 'tile', splits) or SKINNY, in the form pinned() returns for layouts (al, bl): a plain
    dense call sets no other flag than its precision's (dm_gemm_bf16h runs in bf16 mode: 8 | 32)."""
    if expected == SKINNY:
        return SKINNY
    loop, tile, splits = expected
    assert loop in LOOPS and tile in TILES
    flags = {'regstaged': 0, 'dma': 0, 'bf16': FLAG_BF16, 'bf16store': FLAG_BF16 | FLAG_BF16_STORAGE}[loop]
    return (loop, tile, al, bl, splits, flags)
