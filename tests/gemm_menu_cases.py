"""The case tables of tests/test_gpu_gemm_menu.py, shared with tests/test_gemm_plan_cpu.py.  Not a test module.

Every row names the kernel that answers its shape: (main loop, tile, split count) in the names of tests/gemm_pin.py.
"""
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
EPILOGUES = ('none', 'full', 'bias')      # full: bias + addend (ldadd > N) + DM_GEMM_ACCUM + DM_GEMM_ELU

# ---- (a) fp32 operands.  Every case runs three times: dm_gemm_dma_enable(0) (register-staged loop for every product), the
# default (1: the LDS-DMA loop from 14 k-tiles per work item) and 2 (the LDS-DMA loop for every k extent).  The switch also
# feeds the cost model (with the LDS-DMA loop on, a row-contiguous B is steered off the 128x128 tile and split (1,1) products
# towards 64x64), so the tile may differ between the runs.  K = 36 / 28 are two / one k-tiles: fewer than the 3-stage ring of
# 128x64 holds, as many as / fewer than the 2-stage rings of 128x96 and 96x128 hold (128x128 is not chosen below K = 260).
F32_CASES = [
    # (al, bl, M, N, K, epilogue, kernel with the switch at 0, at 1 (default), at 2)
    (0, 0, 2564, 3588, 452, 'none', ('regstaged', '128x128', 1), ('dma', '128x128', 1), ('dma', '128x128', 1)),
    (0, 1, 2564, 3588, 452, 'full', ('regstaged', '128x128', 1), ('dma', '64x64', 1), ('dma', '64x64', 1)),
    (1, 0, 2564, 3588, 452, 'bias', ('regstaged', '128x128', 1), ('dma', '128x128', 1), ('dma', '128x128', 1)),
    (1, 1, 2564, 3588, 452, 'none', ('regstaged', '128x128', 1), ('dma', '128x128', 1), ('dma', '128x128', 1)),
    (0, 0, 100, 16388, 1028, 'full', ('regstaged', '128x128', 3), ('regstaged', '128x128', 3), ('dma', '128x128', 3)),
    (0, 1, 100, 16388, 1028, 'bias', ('regstaged', '128x128', 3), ('regstaged', '128x96', 4), ('dma', '128x96', 4)),
    (1, 0, 100, 16388, 1028, 'none', ('regstaged', '128x128', 3), ('regstaged', '128x128', 3), ('dma', '128x128', 3)),
    (1, 1, 100, 16388, 1028, 'full', ('regstaged', '128x128', 3), ('regstaged', '128x128', 3), ('dma', '128x128', 3)),
    (0, 0, 2052, 3588, 36, 'bias', ('regstaged', '128x64', 1), ('regstaged', '128x64', 1), ('dma', '128x64', 1)),
    (0, 1, 2052, 3588, 36, 'none', ('regstaged', '128x64', 1), ('regstaged', '128x64', 1), ('dma', '128x64', 1)),
    (1, 0, 2052, 3588, 36, 'full', ('regstaged', '128x64', 1), ('regstaged', '128x64', 1), ('dma', '128x64', 1)),
    (1, 1, 2052, 3588, 36, 'bias', ('regstaged', '128x64', 1), ('regstaged', '128x64', 1), ('dma', '128x64', 1)),
    (0, 0, 2052, 3588, 28, 'none', ('regstaged', '128x64', 1), ('regstaged', '128x64', 1), ('dma', '128x64', 1)),
    (0, 1, 2052, 3588, 28, 'full', ('regstaged', '128x64', 1), ('regstaged', '128x64', 1), ('dma', '128x64', 1)),
    (1, 0, 2052, 3588, 28, 'bias', ('regstaged', '128x64', 1), ('regstaged', '128x64', 1), ('dma', '128x64', 1)),
    (1, 1, 2052, 3588, 28, 'none', ('regstaged', '128x64', 1), ('regstaged', '128x64', 1), ('dma', '128x64', 1)),
    (0, 0, 2052, 260, 4100, 'full', ('regstaged', '128x64', 8), ('dma', '128x64', 8), ('dma', '128x64', 8)),
    (0, 1, 2052, 260, 4100, 'bias', ('regstaged', '128x64', 8), ('dma', '128x64', 8), ('dma', '128x64', 8)),
    (1, 0, 2052, 260, 4100, 'none', ('regstaged', '128x64', 8), ('dma', '128x64', 8), ('dma', '128x64', 8)),
    (1, 1, 2052, 260, 4100, 'full', ('regstaged', '128x64', 8), ('dma', '64x64', 7), ('dma', '64x64', 7)),
    (0, 0, 100, 100, 36, 'bias', ('regstaged', '64x64', 1), ('regstaged', '64x64', 1), ('dma', '64x64', 1)),
    (0, 1, 100, 100, 36, 'none', ('regstaged', '64x64', 1), ('regstaged', '64x64', 1), ('dma', '64x64', 1)),
    (1, 0, 100, 100, 36, 'full', ('regstaged', '64x64', 1), ('regstaged', '64x64', 1), ('dma', '64x64', 1)),
    (1, 1, 100, 100, 36, 'bias', ('regstaged', '64x64', 1), ('regstaged', '64x64', 1), ('dma', '64x64', 1)),
    (0, 0, 1028, 132, 452, 'none', ('regstaged', '64x64', 1), ('dma', '64x64', 1), ('dma', '64x64', 1)),
    (0, 1, 1028, 132, 452, 'full', ('regstaged', '64x64', 1), ('dma', '64x64', 1), ('dma', '64x64', 1)),
    (1, 0, 1028, 132, 452, 'bias', ('regstaged', '64x64', 1), ('dma', '64x64', 1), ('dma', '64x64', 1)),
    (1, 1, 1028, 132, 452, 'none', ('regstaged', '64x64', 1), ('dma', '64x64', 1), ('dma', '64x64', 1)),
    (0, 0, 100, 516, 8196, 'full', ('regstaged', '64x64', 43), ('regstaged', '64x64', 43), ('dma', '64x64', 43)),
    (0, 1, 100, 516, 8196, 'bias', ('regstaged', '64x64', 43), ('regstaged', '64x64', 43), ('dma', '64x64', 43)),
    (1, 0, 100, 516, 8196, 'none', ('regstaged', '64x64', 43), ('regstaged', '64x64', 43), ('dma', '64x64', 43)),
    (1, 1, 100, 516, 8196, 'full', ('regstaged', '64x64', 43), ('regstaged', '64x64', 43), ('dma', '64x64', 43)),
    (0, 0, 2564, 3076, 36, 'bias', ('regstaged', '128x96', 1), ('regstaged', '128x96', 1), ('dma', '128x96', 1)),
    (0, 1, 2564, 3076, 36, 'none', ('regstaged', '128x96', 1), ('regstaged', '128x96', 1), ('dma', '128x96', 1)),
    (1, 0, 2564, 3076, 36, 'full', ('regstaged', '128x96', 1), ('regstaged', '128x96', 1), ('dma', '128x96', 1)),
    (1, 1, 2564, 3076, 36, 'bias', ('regstaged', '128x96', 1), ('regstaged', '128x96', 1), ('dma', '128x96', 1)),
    (0, 0, 2564, 3076, 28, 'none', ('regstaged', '128x96', 1), ('regstaged', '128x96', 1), ('dma', '128x96', 1)),
    (0, 1, 2564, 3076, 28, 'full', ('regstaged', '128x96', 1), ('regstaged', '128x96', 1), ('dma', '128x96', 1)),
    (1, 0, 2564, 3076, 28, 'bias', ('regstaged', '128x96', 1), ('regstaged', '128x96', 1), ('dma', '128x96', 1)),
    (1, 1, 2564, 3076, 28, 'none', ('regstaged', '128x96', 1), ('regstaged', '128x96', 1), ('dma', '128x96', 1)),
    (0, 0, 2564, 260, 2052, 'full', ('regstaged', '128x96', 4), ('dma', '128x96', 4), ('dma', '128x96', 4)),
    (0, 1, 2564, 260, 2052, 'bias', ('regstaged', '128x96', 4), ('dma', '128x96', 4), ('dma', '128x96', 4)),
    (1, 0, 2564, 260, 2052, 'none', ('regstaged', '128x96', 4), ('dma', '128x96', 4), ('dma', '128x96', 4)),
    (1, 1, 2564, 260, 2052, 'full', ('regstaged', '128x96', 4), ('dma', '64x64', 4), ('dma', '64x64', 4)),
    (0, 0, 644, 12292, 36, 'bias', ('regstaged', '96x128', 1), ('regstaged', '96x128', 1), ('dma', '96x128', 1)),
    (0, 1, 644, 12292, 36, 'none', ('regstaged', '96x128', 1), ('regstaged', '96x128', 1), ('dma', '96x128', 1)),
    (1, 0, 644, 12292, 36, 'full', ('regstaged', '96x128', 1), ('regstaged', '96x128', 1), ('dma', '96x128', 1)),
    (1, 1, 644, 12292, 36, 'bias', ('regstaged', '96x128', 1), ('regstaged', '96x128', 1), ('dma', '96x128', 1)),
    (0, 0, 644, 12292, 28, 'none', ('regstaged', '96x128', 1), ('regstaged', '96x128', 1), ('dma', '96x128', 1)),
    (0, 1, 644, 12292, 28, 'full', ('regstaged', '96x128', 1), ('regstaged', '96x128', 1), ('dma', '96x128', 1)),
    (1, 0, 644, 12292, 28, 'bias', ('regstaged', '96x128', 1), ('regstaged', '96x128', 1), ('dma', '96x128', 1)),
    (1, 1, 644, 12292, 28, 'none', ('regstaged', '96x128', 1), ('regstaged', '96x128', 1), ('dma', '96x128', 1)),
    (0, 0, 260, 2564, 2052, 'full', ('regstaged', '96x128', 4), ('dma', '96x128', 4), ('dma', '96x128', 4)),
    (0, 1, 260, 2564, 2052, 'bias', ('regstaged', '96x128', 4), ('dma', '96x128', 4), ('dma', '96x128', 4)),
    (1, 0, 260, 2564, 2052, 'none', ('regstaged', '96x128', 4), ('dma', '96x128', 4), ('dma', '96x128', 4)),
    (1, 1, 260, 2564, 2052, 'full', ('regstaged', '96x128', 4), ('dma', '64x64', 4), ('dma', '64x64', 4)),
]

# ---- (a) bf16 operands (DM_GEMM_BF16) and bf16 storage (dm_gemm_bf16h: extents in multiples of 8).  Their tile choice does not
# depend on the layouts, so a shape is listed once and runs with all four layout pairs; the epilogue rotates over
# (shape, layout) as in the fp32 table.
BF16_SHAPES = [
    # ((M, N, K), (tile, splits))
    ((2564, 3588, 452), ('128x128', 1)), ((100, 16388, 1028), ('128x128', 3)),
    ((2052, 3588, 36), ('128x64', 1)), ((2052, 3588, 28), ('128x64', 1)), ((2052, 260, 4100), ('128x64', 8)),
    ((100, 100, 36), ('64x64', 1)), ((1028, 132, 452), ('64x64', 1)), ((100, 516, 8196), ('64x64', 43)),
    ((2564, 3076, 36), ('128x96', 1)), ((2564, 3076, 28), ('128x96', 1)), ((2564, 260, 2052), ('128x96', 4)),
    ((644, 12292, 36), ('96x128', 1)), ((644, 12292, 28), ('96x128', 1)), ((260, 2564, 2052), ('96x128', 4)),
]
H_SHAPES = [
    ((2568, 3592, 456), ('128x128', 1)), ((104, 16392, 1032), ('128x128', 3)),
    ((2056, 3592, 40), ('128x64', 1)), ((2056, 3592, 24), ('128x64', 1)), ((2056, 264, 4104), ('128x64', 8)),
    ((104, 104, 40), ('64x64', 1)), ((1032, 136, 456), ('64x64', 1)), ((104, 520, 8200), ('64x64', 43)),
    ((2568, 3080, 40), ('128x96', 1)), ((2568, 3080, 24), ('128x96', 1)), ((2568, 264, 2056), ('128x96', 4)),
    ((648, 12296, 40), ('96x128', 1)), ((648, 12296, 24), ('96x128', 1)), ((264, 2568, 2056), ('96x128', 4)),
]


def _cross(shapes, loop):
    return [(al, bl, M, N, K, EPILOGUES[(si + li) % 3], (loop, tile, splits))
            for si, ((M, N, K), (tile, splits)) in enumerate(shapes) for li, (al, bl) in enumerate(LAYOUTS)]


BF16_CASES = _cross(BF16_SHAPES, 'bf16')
H_CASES = _cross(H_SHAPES, 'bf16store')

# Cells that no shape reaches.  tests/test_gemm_plan_cpu.py::test_sweep_never_reaches_an_unreachable_cell asks the planner itself
# (dm_gemm_plan_query) for every (M, N, K) of a grid of 24 x 24 x 18 ragged extents (36 .. 16388 rows, K up to 131076, up to 4.5 G
# multiply-adds) with the switch at 1 and at 2.
UNREACHABLE = {
    ('dma', '128x128', 0, 1): 'with the LDS-DMA loop on, the cost model charges 128x128 1.3x for a row-contiguous B: another tile always wins',
}
