"""The convolution launch plan as the host states it, without a GPU: rows of the BatchNorm statistics tables of the forward
(fva_conv_stat_blocks) and of the data gradient (fva_conv_dgrad_stat_rows), and the sizes of the packed weights
(fva_conv_packed_elems), for one descriptor per branch of the plan in both dtypes.  Python sizes the tables from these numbers and
the kernels fill them, so they are pinned here as literals (taken from the library before the plan became one function)."""
import ctypes as C

import pytest

F32, BF16 = 0, 1


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def plan(built, dtype, B, H, W, Cin, Cout, k, s):
    lib = built.load()
    d = built.ConvDesc(dtype, B, H, W, Cin, Cout, k, s, 1, 1)
    return (lib.fva_conv_stat_blocks(C.byref(d)), lib.fva_conv_dgrad_stat_rows(C.byref(d)),
            lib.fva_conv_packed_elems(C.byref(d), 0), lib.fva_conv_packed_elems(C.byref(d), 1))


# (B, H, W, Cin, Cout, k, stride) -> {dtype: (forward rows, dgrad rows, packed forward elements, packed dgrad elements)}
# Forward: M = B * OH * OW rows, N = Cout columns.  dgrad: M = B * H * W (stride 1) or B * H/2 * W/2 per parity launch, N = Cin.
# Tile rows BM: 128 for N >= 128, 256 for thinner outputs and for the 8-phase kernel.  Patch tiles: 8 x 32 pixels, 8 x 64 at stride 2.
TABLE = [
    # stride-1 patch kernel (bf16, map >= 64 x 64), the patches overhang: 70 = 8 * 8 + 6, 72 = 2 * 32 + 8
    ((1, 70, 72, 64, 128, 3, 1), {
        BF16: (27,           # 1 * cdiv(70, 8) * cdiv(72, 32) = 9 * 3 patch tiles
               27,           # dgrad 128 -> 64 is a patch layer too: the same tiles
               73728,        # 9 * 128 * 64
               73728),
        F32: (40,            # cdiv(5040, 128): N = 128
              20,            # cdiv(5040, 256): N = 64
              73728, 73728)}),
    ((1, 70, 72, 128, 64, 3, 1), {
        BF16: (27, 27, 73728, 73728),      # both directions on the patch kernel: 9 * 3 tiles; 9 * 64 * 128
        F32: (20, 40, 73728, 73728)}),     # cdiv(5040, 256): N = 64; cdiv(5040, 128): N = 128
    # 8-phase 256 x 256 kernel in bf16 (128 tiles, 36 / 72 k-tiles); 128 x 128 tiles in fp32
    ((8, 64, 64, 256, 512, 3, 1), {
        BF16: (128,          # cdiv(32768, 256)
               128,          # dgrad N = 256, one column block: cdiv(32768, 256)
               1179648,      # 9 * 512 * 256
               1179648),
        F32: (256, 256, 1179648, 1179648)}),   # cdiv(32768, 128) both ways
    # wide and thin tile with a row tail: M = 240
    ((2, 12, 10, 64, 128, 3, 1), {
        BF16: (2,            # cdiv(240, 128): N = 128
               1,            # cdiv(240, 256): N = 64
               73728, 73728),
        F32: (2, 1, 73728, 73728)}),
    # half-row k-tiles: Cin = 32 in bf16 pads the nine forward taps with a zero tap
    ((2, 40, 36, 32, 64, 3, 1), {
        BF16: (12,           # cdiv(2880, 256): N = 64
               12,           # cdiv(2880, 256): N = 32
               20480,        # 10 * 64 * 32
               18432),       # 9 * 32 * 64: the dgrad reduces over Cout = 64
        F32: (12, 12, 18432, 18432)}),
    # stride 2, thin: the stride-2 patch kernel in bf16, two paired launches (N' = 2 * Cin, two table rows per block) in fp32
    ((2, 40, 36, 32, 64, 3, 2), {
        BF16: (3,            # cdiv(720, 256): M = 2 * 20 * 18, N = 64
               10,           # 2 * cdiv(40, 8) * cdiv(36, 64) patch tiles
               20480,        # 10 * 64 * 32: pad tap
               18432),       # 9 * 32 * 64: plain layout
        F32: (3,
              12,            # 2 launches x 2 rows x cdiv(720, 256): N' = 64
              18432,
              24576)}),      # 12 * 64 * 32: paired layout
    ((2, 40, 36, 64, 128, 3, 2), {
        BF16: (6,            # cdiv(720, 128): N = 128
               10,           # 2 * 5 * 1 patch tiles
               73728, 73728),
        F32: (6,
              24,            # 2 launches x 2 rows x cdiv(720, 128): N' = 128
              73728,
              98304)}),      # 12 * 128 * 64
    # stride 2 paired in both dtypes
    ((2, 40, 36, 64, 64, 3, 2), {
        BF16: (3,            # cdiv(720, 256): N = 64
               24,           # 2 launches x 2 rows x cdiv(720, 128): N' = 128
               36864,        # 9 * 64 * 64
               49152),       # 12 * 64 * 64
        F32: (3, 24, 36864, 49152)}),
    # stride 2, four parity launches
    ((3, 8, 12, 128, 128, 3, 2), {
        BF16: (1,            # cdiv(72, 128)
               4,            # 4 launches x cdiv(72, 128)
               147456, 147456),      # 9 * 128 * 128
        F32: (1, 4, 147456, 147456)}),
    # ... of which the one-tap class (4 k-tiles) stays on 128 x 128 tiles and the others (8, 8, 16 k-tiles) take the 8-phase kernel
    ((8, 128, 128, 256, 256, 3, 2), {
        BF16: (128,          # cdiv(32768, 256): 8-phase forward, 36 k-tiles
               640,          # cdiv(32768, 128) + 3 * cdiv(32768, 256)
               589824, 589824),      # 9 * 256 * 256
        F32: (256,           # cdiv(32768, 128)
              1024,          # 4 launches x cdiv(32768, 128)
              589824, 589824)}),
    # 1 x 1
    ((1, 13, 13, 256, 128, 1, 1), {
        BF16: (2,            # cdiv(169, 128), N = 128
               2,            # cdiv(169, 128), N = 256
               32768, 32768),        # 128 * 256
        F32: (2, 2, 32768, 32768)}),
]


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', TABLE, ids=lambda c: 'x'.join(map(str, c[0])))
def test_plan_rows_and_packed_sizes(built, case, dtype):
    desc, want = case
    assert plan(built, dtype, *desc) == want[dtype]


def test_patch_layers_fall_to_the_implicit_gemm_when_the_patch_kernel_is_off(built):
    lib = built.load()
    prev = lib.fva_conv_patch_kernel(0)
    try:
        # as fp32: cdiv(5040, 128) for N = 128, cdiv(5040, 256) for N = 64
        assert plan(built, BF16, 1, 70, 72, 64, 128, 3, 1) == (40, 20, 73728, 73728)
        assert plan(built, BF16, 1, 70, 72, 128, 64, 3, 1) == (20, 40, 73728, 73728)
    finally:
        lib.fva_conv_patch_kernel(prev)
    assert plan(built, BF16, 1, 70, 72, 64, 128, 3, 1) == (27, 27, 73728, 73728)
