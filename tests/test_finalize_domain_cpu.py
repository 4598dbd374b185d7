"""The finalize domain tests' own footing, without a GPU: the reference stays inside the condition the GPU tests hold the kernels
to, and a numpy emulation of the MFMA x2 kernels' hi + lo split shows why those kernels have an absolute error floor
(``tests/_finalize_domain.py`` states the contracts; ``tests/test_gpu_finalize_domain.py`` holds the kernels to them)."""
import numpy as np
import pytest

import _finalize_domain as fd
from oracle import heatmap_oracle as ho


@pytest.mark.parametrize('variant', fd.VARIANTS)
@pytest.mark.parametrize('sides', fd.SIDES, ids=lambda s: 'x'.join(map(str, s)))
def test_f32_oracle_within_the_condition(sides, variant):
    """The f32 numpy oracle -- the arithmetic an exact-f32 kernel mirrors -- is within 2^-21 of the row maximum of the float64 one
    on levelled f32 planes, for every class / side of the GPU matrix and every k (the exact routes' list with 40, and 17, the
    largest exponent the earlier side-32 survey covered): a kernel held to 2^-19 is not asked for more than f32 can give."""
    out_side = fd.out_side_of(sides)
    base = fd.draw_planes(sides, variant)
    want0 = fd.reference64([fd.round_to(b, 'float32') for b in base], sides, out_side)
    worst = 0.0
    for k in sorted(set(fd.K_EXACT + fd.K_MFMA + [17, 40])):
        planes, homogeneous = fd.scaled_planes(base, k, 'float32')
        assert homogeneous                                        # f32 holds every level at every k of the matrix
        got = ho.global_heat_map(fd.raw_keys(planes, sides, out_side), out_side * out_side, dtype=np.float32)
        err, rowmax = fd.row_errors(got, want0 * 2.0 ** k)
        assert (rowmax > 0).all()
        assert (err <= fd.ORACLE_F32_REL * rowmax).all(), (k, float((err / rowmax).max()))
        worst = max(worst, float((err / rowmax).max()))
    print(f'{sides} {variant}: f32 oracle vs float64, worst err_t / rowmax_t = 2^{np.log2(worst):.2f}')


@pytest.mark.parametrize('variant', fd.VARIANTS)
@pytest.mark.parametrize('dtype', fd.DTYPES)
def test_split_emulation_meets_the_mfma_contract(dtype, variant):
    """hi = fp16(v), lo = fp16(v - hi) on the plane (f32 sums) and on T (every dtype), nothing else inexact: inside |v| <= 2^15 the
    result is within 2^-19 * rowmax_t + 2^-23 of the float64 reference at every k of the MFMA routes."""
    base = fd.draw_planes((32,), variant)
    for k in fd.K_MFMA:
        k = fd.scale_exp(base, k, fd.DOMAIN_MAX)
        planes, _ = fd.scaled_planes(base, k, dtype)
        assert max(float(np.abs(p.astype(np.float64)).max()) for p in planes) <= fd.DOMAIN_MAX
        want = fd.reference64(planes, (32,), 64)
        rel, ab = fd.assert_contract(fd.emulate_mfma_x2(planes[0], dtype), want, True, f'emulated split, {dtype} {variant} k={k}')
        print(f'{dtype} {variant} k={k}: emulated split, worst err_t / rowmax_t = {rel:.3e}, worst err_t = 2^{np.log2(max(ab, 1e-300)):.1f}')


@pytest.mark.parametrize('variant', fd.VARIANTS)
@pytest.mark.parametrize('dtype', fd.DTYPES)
def test_split_emulation_needs_the_floor(dtype, variant):
    """Why the floor exists: at k = 0 every token row at level 2^-21 breaks the PURE relative contract under the split alone (lo is an
    fp16 subnormal there: half an ulp of it, 2^-25, against a row maximum of about 2^-17), while the rows at level 1 keep it."""
    base = fd.draw_planes((32,), variant)
    planes, _ = fd.scaled_planes(base, 0, dtype)
    want = fd.reference64(planes, (32,), 64)
    err, rowmax = fd.row_errors(fd.emulate_mfma_x2(planes[0], dtype), want)
    level = np.arange(fd.TOKENS) % fd.N_LEVELS
    low, high = level == fd.N_LEVELS - 1, level == 0
    assert (err[low] > fd.REL * rowmax[low]).all(), (err[low] / rowmax[low]).min()
    assert (err[high] <= fd.REL * rowmax[high]).all(), (err[high] / rowmax[high]).max()
    assert (err <= fd.contract_bound(rowmax, True)).all()


def test_generator_levels_and_domain():
    """Token rows 8 x apart per level, the unconditional half zero, the signed variant really signed; the domain clamp divides by a power
    of two only."""
    for variant in fd.VARIANTS:
        (p,) = fd.draw_planes((16,), variant)
        assert p.shape == (2 * fd.HEADS, 256, fd.TOKENS) and not p[:fd.HEADS].any()
        med = np.median(np.abs(p[fd.HEADS:]), axis=(0, 1))
        np.testing.assert_allclose(np.log2(med), -fd.LEVEL_STEP * (np.arange(fd.TOKENS) % fd.N_LEVELS), atol=0.35)
        assert (p.min() < 0) == (variant == 'signed')
        top = float(np.abs(p).max())
        k = fd.scale_exp([p], 12, fd.DOMAIN_MAX)
        assert k < 12 and top * 2.0 ** k <= fd.DOMAIN_MAX < top * 2.0 ** (k + 1)      # the largest power of two that fits
        assert fd.scale_exp([p], -10, fd.DOMAIN_MAX) == -10 and fd.scale_exp([p], 40) == 40
    # fp16 sums: the low levels at k = -20 leave the normal range, and the generator says so
    _, homogeneous = fd.scaled_planes(fd.draw_planes((16,), 'nonneg'), -20, 'float16')
    assert not homogeneous
