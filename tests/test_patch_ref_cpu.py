"""The inputs of tests/test_gpu_patch_edges.py can carry what that file asserts - shown without a GPU, for every (graph, D, dirty rows)
it uses (patch_ref.CASES and the forced walks' case):

  * the numpy mirror of the staging rule calls the matrix "wide" at guard levels 2 and 3 and not at level 1, with exactly the intended
    dirty rows;
  * the TF32-mode oracle alone stays within walks.NOISE_SHARE of the bound the GPU test applies to a patched score (4 x TIGHT of the
    edge's own sum of |terms|), measured from an fp64 evaluation on the same rounded operands;
  * the emulated UNPATCHED result - the fp64 product of the emulated fp16 images - is outside that bound on at least 99 % of the touched
    edges of covered rows (the cap is a condition the reference alone meets: a dot product of random signs that happens to cancel to
    1.6e-5 of its terms would pass unpatched; it is no tolerance of the kernel), and
  * bit-equal to the rounded-operand product on every untouched edge: the image loses nothing outside the dirty rows.

Measured over the 36 inputs (the FIG lines of this file, `-s`): the oracle's noise is at most 8.1e-7 of an edge's sum of |terms| (D = 200),
a share of 0.05 of the bound; unpatched edges outside the bound, of the touched edges of covered rows: short_metadata_n4100 670 / 670
at D = 5 / 41 / 64 / 200 and 668 / 670 at D = 128, the uniform 4 000 x 100 graph 48 773 / 48 779 with 256 dirty rows at D = 64, every one
on the identity graph, the clique, the rings and the hub rows (40 282); untouched edges: distance 0 everywhere."""
import numpy as np
import pytest

import patch_ref as P
import walks as W

ALL = P.CASES + [P.WALK_CASE]


def test_the_mirror_of_the_scale_exponent_and_the_image():
    assert P.scale_exp_from_bits(P.bits(1.0)) == 14 and P.scale_exp_from_bits(P.bits(65536.0)) == -2 and P.scale_exp_from_bits(P.bits(3.0e4)) == 0
    assert P.scale_exp_from_bits(0) == 0 and P.scale_exp_from_bits(0x7f800000) == 0 and P.scale_exp_from_bits(P.bits(1e-38)) == 126
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26], np.float32)
    img = P.image(x, 1.0).astype(np.float64)
    # (ties away from zero at 10 bits; below fp16's subnormal step the cast rounds to nearest even: 2^-25 -> 0, 1.5 x 2^-25 -> 2^-24)
    assert list(img) == [1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -10, 2.0 ** -24, 0.0, 2.0 ** -24, 0.0]
    assert list(P.is_tiny(np.array([0.0, 6.0e-5, 6.2e-5, -1e-30], np.float32), 1.0)) == [False, True, False, True]


def test_the_clique_and_the_rings_are_what_the_gpu_file_takes_them_for():
    rp, col = P.graph("clique17_n700")
    assert P.is_symmetric(rp, col)
    for r in P.CLIQUE_ROWS:
        assert sorted(col[rp[r]: rp[r + 1]]) == sorted(set(P.CLIQUE_ROWS) - {r})
    assert len(set(P.CLIQUE_ROWS // 16)) >= 3 and len(col) >= 8
    for n in (491519, 491520):
        rp, col = P.graph("ring_n%d" % n)
        assert P.is_symmetric(rp, col) and (np.diff(rp) == 2).all()
        # the patch keeps its bitmap (N + 1 bits) in LDS up to kPatchBitmapWords = 15 360 words
        assert ((n + 1 + 31) >> 5 <= 15360) == (n == 491519)
    assert P.is_symmetric(*P.graph("uniform_n4000")) and P.is_symmetric(*P.graph("hub_rows_n2500")) and not P.is_symmetric(*P.graph("directed_n4000"))
    n = 4100
    assert P.finding_rows(n)[-1] >= P.covered_rows("short_metadata_n4100", n) > P.finding_rows(n)[1]
    assert sorted(set(P.finding_rows(n) >> 5)) == [18, 64, 128]
    assert {k for g, _, k in P.CASES if g == "uniform_n4000"} == {1, 3, 256, 257}


@pytest.mark.parametrize("case", ALL, ids=[P.case_id(c) for c in ALL])
def test_inputs_make_a_missing_patch_visible(case):
    name, D, k = case
    rp, col = P.graph(name)
    n = len(rp) - 1
    rows = P.case_rows(name, k)
    assert len(rows) == k == len(set(rows))
    for salt in (0, 1):                         # X of the forward calls, dY of the backward call
        X = P.wide_matrix(n, D, rows, salt)
        assert np.array_equal(P.dirty_rows(X), np.sort(rows))
        assert [P.range_mode(X, D, lv) for lv in (1, 2, 3)] == [0, 2, 1]
        assert P.range_mode(P.ordinary_matrix(n, D, salt)[0], D, 2) == 0
    X = P.wide_matrix(n, D, rows)
    ref, r64, s64, _ = P.score_refs(name, X)
    covered = np.arange(len(col)) < rp[P.covered_rows(name, n)]
    touched = P.touched_edges(rp, col, rows)
    noise = P.ratio(ref, r64, s64).max()
    unp = P.unpatched_scores(name, X)
    judged = touched & covered
    outside = P.ratio(unp, ref, s64)[judged] > P.SCORE_BOUND
    print("FIG %-34s oracle noise %.2e (share %.3f) unpatched outside %d / %d" % (P.case_id(case), noise, noise / P.SCORE_BOUND, outside.sum(), judged.sum()))
    assert noise <= W.NOISE_SHARE * P.SCORE_BOUND
    assert judged.sum() >= k and outside.sum() >= 0.99 * judged.sum()
    assert np.array_equal(unp[~touched], r64[~touched])
    assert not ref[~covered].any() and not unp[~covered].any()
