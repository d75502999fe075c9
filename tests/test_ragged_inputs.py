"""CPU checks of the ragged-shape cases (tests/ragged_cases.py) that test_gpu_ragged.py runs on the GPU.

* The table against the planner mirror: every case's stated branch and K splits follow from
  `ragged_cases.plan` (plan_wproj / make_plan and the v2 / s8 / sc conditions re-written in Python).
* The determinacy screen, oracle alone: the GPU comparison is on the sign-aligned leading half of U
  and V at 1e-4, which means something only if those vectors are determined well past that bar.
  The oracle runs on the case's A and Omega and again on A (1 + 1e-7 N), N standard normal -- an
  fp32-sized relative perturbation.  Required: leading-half U and V within 1e-5 relative Frobenius
  (10x inside the bar), S within 1e-6 (100x inside) and S[l/2 - 1] >= 10 S[l - 1].  A case that fails
  gets another decay / seed / weights in the table, never a shorter comparison.
  Measured: the screen takes about 50 s for the 31 cases before the f64n row, which adds under a
  second (the four l = 512 cases 8 - 9 s each, two oracle runs of 4 s; the others 2 s or less), the
  whole file about 55 s.
* The builder's point, oracle alone: a dropped last row or column of A moves S by > 1e-2.
"""
import numpy as np
import pytest

import oracle
import ragged_cases as rc
from conftest import rel_fro, sign_align

IDS = [c.id for c in rc.CASES]


def test_table_shape():
    assert len(set(IDS)) == len(IDS) == 32
    assert sorted(c.id for c in rc.CASES if c.l == 512) == ["b512f", "b512v", "e512f", "e512n"]
    for c in rc.CASES:
        assert c.l <= min(c.m, c.n) and c.q >= 1  # legal under check_desc_msg; q >= 1 runs NN hi / lo and TN
        assert 0.5 < c.decay < 1.0
    assert set(rc.OUT_CASES) <= set(IDS) and {p.case for p in rc.PITCH_CASES} <= set(IDS)


@pytest.mark.parametrize("pc", rc.PITCH_CASES, ids=[p.id for p in rc.PITCH_CASES])
def test_pitch_cases_leave_the_dma_kernels(pc):
    """An unaligned base or an lda off the 16-byte chunk: the fallback kernel, with these splits."""
    c = rc.BY_ID[pc.case]
    esz = 1 if c.dtype == "e4m3" else 2
    p = rc.plan(c.dtype, c.m, c.n, c.l, lda=c.m + pc.pad, a_aligned=(pc.off * esz) % 16 == 0)
    assert rc.plan(c.dtype, c.m, c.n, c.l)["v2"] and not p["v2"]
    assert (p["sketch"], p["nn"], p["tn"]) == ("wproj", "wproj", "wproj")
    assert (p["splits_nn"], p["splits_tn"]) == pc.splits
    assert pc.off + c.m <= c.m + pc.pad


@pytest.mark.parametrize("cid", IDS)
def test_branch_follows_from_planner_mirror(cid):
    c = rc.BY_ID[cid]
    p = rc.plan(c.dtype, c.m, c.n, c.l)
    assert c.branch, "every case names the branch it is there for"
    for key, want in c.branch.items():
        assert p[key] == want, (cid, key, p[key], want)
    assert (p["splits_nn"], p["splits_tn"]) == c.splits


def test_mirror_hand_derived_plans():
    """Plans worked out by hand from csrc/wide_plan.cpp and csrc/proj.hip, independent of the table."""
    # e4m3 1024 x 1152, LP 256, v2: NN 4 row blocks of 256, target 256 -> 64 splits, capped by
    # K / 256 = 4; chunk 288 is no multiple of 128, so the sketch takes the K = 32 form
    p = rc.plan_wproj(1024, 1152, 256, True, True, True)
    assert (p["blocks"], p["splits"], p["chunk"]) == (4, 4, 288)
    # tn2 (bf16 LP 256 TN): K = 1032 -> 4 splits of 258, rounded to whole 64-row pairs: 320; last chunk 72
    p = rc.plan_wproj(701, 1032, 256, True, False, False)
    assert p["tn2"] and (p["splits"], p["chunk"]) == (4, 320) and 1032 - 3 * 320 == 72
    # tn4 (e4m3 LP 256 TN): K = 1040 -> 4 splits of 260, rounded to 128-row slots: 384; 3 splits, last slot 16
    p = rc.plan_wproj(1000, 1040, 256, True, False, True)
    assert p["tn4"] and (p["splits"], p["chunk"]) == (3, 384) and (1040 - 2 * 384) % 128 == 16
    # ds needs K % 64 == 0
    assert rc.plan_wproj(701, 1088, 128, True, False, False)["ds"]
    assert not rc.plan_wproj(702, 1000, 128, True, False, False)["ds"]
    # the aligned shapes of the existing tests give the block-scaled sketch (the gap this suite closes)
    assert rc.plan("e4m3", 4096, 2048, 256)["sc"] and rc.plan("e4m3", 4096, 2048, 512)["sc"]
    # v2 needs the base, lda and m aligned to the 16-byte chunk
    assert not rc.plan("bf16", 1000, 702, 128, a_aligned=False)["v2"]
    assert not rc.plan("bf16", 1000, 702, 128, lda=1001)["v2"]
    assert not rc.plan("e4m3", 1024, 1056, 256, lda=1032)["v2"]
    # fp32 513 x 257 narrow: NN 9 blocks of 64 rows, K / 128 = 2 splits; TN 9 blocks, K / 512 = 1
    p = rc.plan("f32", 513, 257, 10)
    assert (p["engine"], p["LP"], p["splits_nn"], p["splits_tn"]) == ("narrow", 16, 2, 1)


def test_tail_weighting():
    c = rc.BY_ID["b128f"]
    A = rc.tail_weighted(c.m, c.n, 2 * c.l, c.decay, c.seed)
    from conftest import gapped_matrix

    A0 = gapped_matrix(c.m, c.n, 2 * c.l, decay=c.decay, seed=c.seed)
    W = A / A0
    assert np.allclose(W[:-3, :-3], 1.0)
    assert np.allclose(W[-3:, 0], rc.ROW_W) and np.allclose(W[0, -3:], rc.COL_W)
    assert len(set(rc.ROW_W + rc.COL_W)) == 6 and all(3 <= w <= 8 for w in rc.ROW_W + rc.COL_W)
    # the oracle's inputs are exactly representable in the case's storage type
    stored, scale, exact, Om = rc.inputs("e256n")
    assert np.array_equal(stored.float().double().numpy() * scale, exact)
    assert np.array_equal(rc._round_to(Om, "e4m3"), Om)


@pytest.mark.parametrize("cid", ["b256v", "e256t", "f32c", "f64a"])
def test_tail_mistake_would_show(cid):
    """What the weighting is for: a kernel that dropped the last row of A (the K tail of A^T Q) or
    its last column (the K tail of A X) moves S by far more than the 1e-4 the GPU test allows."""
    c = rc.BY_ID[cid]
    _, _, A, Om = rc.inputs(cid)
    _, So, _ = rc.oracle_result(cid)
    for cut in (np.s_[-1:, :], np.s_[:, -1:]):
        Ad = np.array(A)
        Ad[cut] = 0.0
        _, Sd, _ = oracle.rsvd(Ad, c.l, q=c.q, Omega=Om)
        assert rel_fro(Sd, So) > 1e-2, rel_fro(Sd, So)


@pytest.mark.parametrize("cid", IDS)
def test_determinacy_screen(cid):
    c = rc.BY_ID[cid]
    _, _, A, Om = rc.inputs(cid)
    Uo, So, Vo = rc.oracle_result(cid)
    rng = np.random.default_rng(7)
    Ap = A * (1.0 + 1e-7 * rng.standard_normal(A.shape))
    Up, Sp, Vp = oracle.rsvd(Ap, c.l, q=c.q, Omega=Om)
    k = c.l // 2
    eu = rel_fro(sign_align(Up[:, :k], Uo[:, :k]), Uo[:, :k])
    ev = rel_fro(sign_align(Vp[:, :k], Vo[:, :k]), Vo[:, :k])
    es = rel_fro(Sp, So)
    print(f"{cid}: U {eu:.2e} V {ev:.2e} S {es:.2e} S[k-1]/S[-1] {So[k - 1] / So[-1]:.1f}")
    assert eu < 1e-5 and ev < 1e-5, (eu, ev)
    assert es < 1e-6, es
    assert So[k - 1] >= 10 * So[-1], (So[k - 1], So[-1])
