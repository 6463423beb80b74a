"""The folded next-event estimate adds what the three-array form adds, bit for bit: the argument of the comment at the fold in shade_body, restated
in float32 numpy over edge values (no GPU).

Three-array form (k_nee_resolve): ld = 0 [+ A if the shadow ray is unoccluded]; L += pbeta * (ld / A.w).
Folded form: shade_body stores add = pbeta * ((0 + A) / A.w); k_nee_resolve does L += add if unoccluded and nothing otherwise.
  - unoccluded: the same operations in the same order on the same operands;
  - occluded: the three-array form adds pbeta * (0 / A.w).  A.w is a selection pdf > 0, so the quotient is +0; with pbeta finite the
    product is +0 or -0; and L is never -0 (it starts as +0 and every write is a sum, which is -0 only if both terms are), so L + (+-0) = L.
Non-finite pbeta, A or A.w keep the three-array form: inf * 0 is NaN and would reach L."""
import itertools

import numpy as np

f32 = np.float32
TINY = np.finfo(f32).tiny
DENORM = f32(1e-45)                       # the smallest denormal
BIG = np.finfo(f32).max
FINITE = [f32(0.0), f32(-0.0), DENORM, -DENORM, f32(TINY), f32(1.0), f32(-0.73), BIG, -BIG]
NONFINITE = [f32(np.inf), f32(-np.inf), f32(np.nan)]
PDFS = [DENORM, f32(TINY), f32(0.25), f32(1.0), BIG]             # light_pdf > 0, the only way into the block
L_VALUES = [f32(0.0), DENORM, -DENORM, f32(3.5), f32(-2.0), BIG, -BIG]       # every value but -0


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


def fold_ok(pb, a, aw):
    """shade_body's condition for folding."""
    return bool(np.isfinite(pb) and np.isfinite(a) and np.isfinite(aw))


def three_array(L, pb, a, aw, occluded):
    ld = f32(0.0)
    if not occluded:
        ld = f32(ld + a)
    return f32(L + f32(pb * f32(ld / aw)))


def folded(L, pb, a, aw, occluded):
    add = f32(pb * f32(f32(f32(0.0) + a) / aw))          # in shade_body
    return L if occluded else f32(L + add)               # in k_nee_resolve


def test_a_sum_is_minus_zero_only_if_both_terms_are():
    vals = FINITE + NONFINITE
    with np.errstate(all="ignore"):
        for a, b in itertools.product(vals, vals):
            s = f32(a + b)
            if bits(s) == 0x80000000:
                assert bits(a) == 0x80000000 and bits(b) == 0x80000000, (a, b)
    assert bits(f32(-0.0) + f32(-0.0)) == 0x80000000                  # the one way there, and L's first term is +0


def test_folded_equals_three_array_on_finite_inputs():
    n = 0
    with np.errstate(all="ignore"):
        for L, pb, a, aw, occ in itertools.product(L_VALUES, FINITE, FINITE, PDFS, (False, True)):
            assert fold_ok(pb, a, aw)
            want, got = three_array(L, pb, a, aw, occ), folded(L, pb, a, aw, occ)
            assert bits(want) == bits(got), (L, pb, a, aw, occ, want, got)
            n += 1
    assert n == len(L_VALUES) * len(FINITE) ** 2 * len(PDFS) * 2


def test_occluded_add_is_a_signed_zero():
    with np.errstate(all="ignore"):
        for pb, aw in itertools.product(FINITE, PDFS):
            z = f32(pb * f32(f32(0.0) / aw))
            assert bits(z) in (0x00000000, 0x80000000), (pb, aw, z)


def test_non_finite_inputs_take_the_fallback():
    differs = 0
    with np.errstate(all="ignore"):
        for bad in NONFINITE:
            for pb, a, aw in ((bad, f32(1.0), f32(1.0)), (f32(1.0), bad, f32(1.0)), (f32(1.0), f32(1.0), bad)):
                assert not fold_ok(pb, a, aw)
                for occ in (False, True):
                    if bits(three_array(f32(2.0), pb, a, aw, occ)) != bits(folded(f32(2.0), pb, a, aw, occ)):
                        differs += 1
    assert differs > 0                      # and the condition is needed: an infinite pbeta on an occluded ray adds NaN in the three-array form
    with np.errstate(all="ignore"):
        assert np.isnan(three_array(f32(2.0), f32(np.inf), f32(1.0), f32(1.0), True)) and folded(f32(2.0), f32(np.inf), f32(1.0), f32(1.0), True) == f32(2.0)


def test_the_mark_cannot_be_a_selection_pdf():
    """pendA.w = +0 marks a folded entry; a stored selection pdf passed `light_pdf > 0`, denormals included."""
    for aw in PDFS:
        assert aw > 0 and bits(aw) != 0
