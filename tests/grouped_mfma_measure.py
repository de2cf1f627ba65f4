"""The limits of the matrix-unit grouped 3x3 convolution (fva_gconv_mfma_*: bf16 tensors, stride 1), derived and not observed; the host
side of tests/test_grouped_mfma_measure_cpu.py and tests/test_gpu_grouped_mfma.py.  Not a test module (pytest does not collect it).

The reference is always resnext_restatement.gconv_reference in float64 on the operands as uploaded (bf16-rounded on the host).  The
kernels multiply bf16 by bf16 -- exact in fp32 -- and add in fp32, so the only errors are those of the additions and of the one rounding of
a bf16 output.  Any order of n fp32 additions of exact terms stays inside (n - 1) * 2^-24 * sum |term|; streaming_measure.sum_limit(n, S)
is (n + 2) * 2^-24 * S.  With S = gconv_reference(|x|, |w|, |dy|, float64), the sum of the magnitudes of an element's terms:

    bf16 y and dx   |got - ref64| <= 0.5 * bf16_ulp(ref64) + sum_limit(9 * Cg, S)
    fp32 dw         |got - ref64| <= sum_limit(B * H * W, S['dw'])

Statistics: the formulas of ``_compare`` in tests/test_gpu_grouped.py with e1 = sum of L, e2 = sum of (2 |y| L + L^2), L the fp32 part of
y's limit, n the positions per block plus the number of blocks."""
import torch

import resnext_restatement as xr
import streaming_measure as sm

RUN = 256                    # padded positions per block of the forward kernel = per row of its statistics table

# (B, H, W, C, Cg): where runs of padded positions can go wrong, not the workload
CASES = [(3, 10, 34, 128, 4), (3, 10, 34, 64, 64),        # runs straddle rows and both image boundaries
         (1, 16, 18, 64, 8), (2, 5, 7, 64, 16),            # even and odd maps
         (2, 2, 2, 128, 32),                               # shifts longer than the map
         (3, 26, 2, 256, 32),                              # two-pixel rows
         (6, 7, 7, 128, 32),                               # several images per run
         (2, 14, 14, 64, 16)                               # mid-size map
         ] + [(2, 4, 4, 32 * Cg, Cg) for Cg in (4, 8, 16, 32, 64)]      # the five widths, C = 2048 among them


def case_id(c):
    return 'x'.join(map(str, c))


def operands(B, H, W, Cc, Cg, seed):
    """x [B, H, W, C], w [C, Cg, 3, 3], dy [B, H, W, C] in fp32 holding bf16 values: what is uploaded."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cc, generator=g)
    w = torch.randn(Cc, Cg, 3, 3, generator=g) * (9 * Cg) ** -0.5
    dy = torch.randn(B, H, W, Cc, generator=g)
    return tuple(t.bfloat16().float() for t in (x, w, dy))


def references(x, w, dy, groups):
    """(ref64, S): the float64 reference and the same evaluation of the magnitudes."""
    return (xr.gconv_reference(x, w, dy, groups, 1, torch.float64),
            xr.gconv_reference(x.abs(), w.abs(), dy.abs(), groups, 1, torch.float64))


def limits(x, groups, ref64, S):
    """{'y', 'dx', 'dw'}: the element-wise limits; 'L': the fp32 part of y's."""
    B, H, W, Cc = x.shape
    Cg = Cc // groups
    L = sm.sum_limit(9 * Cg, S['y'])
    return {'y': 0.5 * sm.bf16_ulp(ref64['y']) + L, 'dx': 0.5 * sm.bf16_ulp(ref64['dx']) + sm.sum_limit(9 * Cg, S['dx']),
            'dw': sm.sum_limit(B * H * W, S['dw']), 'L': L}


def worst(got, ref, lim):
    """Largest err / limit (<= 1 passes; inf where something is not finite)."""
    return sm.worst_f32(got, ref, lim)


def stat_blocks(B, H, W):
    return (B * (H + 2) * (W + 2) + RUN - 1) // RUN


def stat_limits(ref64, L, nblk, eps=1e-5):
    """(mean64, var64, lim_mean, lim_var) per channel for the statistics folded by fva_bn_finalize."""
    y = ref64['y']
    M = y.numel() // y.shape[-1]
    n = RUN + nblk
    e1 = L.sum((0, 1, 2))
    e2 = (2 * y.abs() * L + L * L).sum((0, 1, 2))
    mean64 = ref64['s1'] / M
    var64 = ref64['s2'] / M - mean64 ** 2
    lim_mean = sm.sum_limit(n, ref64['s1_abs'], e1) / M + sm.EPS32 * mean64.abs()
    lim_var = sm.sum_limit(n, ref64['s2_abs'], e2) / M + 2 * mean64.abs() * lim_mean + lim_mean ** 2 + 4 * sm.EPS32 * (var64 + eps)
    return mean64, var64, lim_mean, lim_var


def compare(x, w, dy, groups, got, what):
    """got = (y [B, H, W, C] bf16, dx bf16, dw fp32, fin or None) on the host; fin = (mean, rstd, nblk) in float64.  Prints every figure,
    then asserts."""
    ref64, S = references(x, w, dy, groups)
    lim = limits(x, groups, ref64, S)
    y, dx, dw, fin = got
    figs = {}
    for k, g in (('y', y), ('dx', dx), ('dw', dw)):
        assert g.shape == ref64[k].shape, (what, k, g.shape)
        figs[k] = worst(g.float(), ref64[k], lim[k])
    if fin is not None:
        mean, rstd, nblk = fin
        mean64, var64, lim_mean, lim_var = stat_limits(ref64, lim['L'], nblk)
        figs['mean'] = ((mean - mean64).abs() / lim_mean).max().item()
        figs['var'] = ((1.0 / rstd ** 2 - 1e-5 - var64).abs() / lim_var).max().item()
    print(f'  {what}: worst err / limit ' + ', '.join(f'{k} {v:.3f}' for k, v in figs.items()))
    assert all(v <= 1.0 for v in figs.values()), (what, figs)
    return figs


def unpack(table, Cc, Cg, dgrad):
    """The packed table (bf16 [C / 16][steps][64][8], include/fastvision_amd.h) back to OIHW fp32 [C][Cg][3][3], and the number of table
    elements that are non-zero without being the image of a weight (0 for a well-formed table)."""
    steps = 9 * (Cg // 32) if Cg >= 32 else 5
    t = table.float().reshape(-1)
    assert t.numel() == (Cc // 16) * steps * 512, (t.numel(), Cc, Cg)
    i = torch.arange(t.numel())
    j, lane, step, slab = i % 8, (i // 8) % 64, (i // 512) % steps, i // (512 * steps)
    m, k = lane % 16, 8 * (lane // 16) + j
    c = 16 * slab + m
    if Cg >= 32:
        tap, kc, gb = step // (Cg // 32), 32 * (step % (Cg // 32)) + k, (c // Cg) * Cg
        live = torch.ones_like(i, dtype=torch.bool)
        co, ci, tp = (gb + kc, c - gb, 8 - tap) if dgrad else (c, kc, tap)
    else:
        tap, kc = 2 * step + k // 16, k % 16
        live = (tap < 9) & (kc // Cg == m // Cg)
        co, ci, tp = (16 * slab + kc, m % Cg, 8 - tap) if dgrad else (c, kc % Cg, tap)
    w = torch.full((Cc * Cg * 9,), float('nan'))
    flat = (co * Cg + ci) * 9 + tp
    assert flat[live].unique().numel() == int(live.sum()) == Cc * Cg * 9          # every weight exactly once
    w[flat[live]] = t[live]
    return w.view(Cc, Cg, 3, 3), int((t[~live] != 0).sum())
