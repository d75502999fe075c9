"""CPU checks of tests/batched_cases.py: every row takes the fused kernel in both types, the table reaches
every (type, LP, panel location) combination the kernel can be launched with, and the two budget pairs sit
on the two sides of the first n whose panels leave LDS -- all from rsvd_batched_is_fused and
rsvd_batched_workspace_bytes, which are host arithmetic and need no device.  A table edit that loses an
instantiation fails here."""
import pytest

import batched_cases as bc
import rsvd_kamaneh_raganato_terrana_amd as R


@pytest.fixture(scope="module", autouse=True)
def _lib():
    R.build(force=False)


def test_rows_are_unique_and_inside_the_limits():
    assert len(set(bc.CASES)) == len(bc.CASES)
    for m, n, l, q in bc.CASES:
        assert 1 <= l <= min(m, n, 64) and max(m, n) <= 256 and q >= 0
    assert set(bc.COMPRESS_CASES) <= set(bc.CASES)
    for _, inside, past in bc.BUDGET_PAIRS:
        assert inside in bc.CASES and past in bc.CASES


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("c", bc.CASES, ids=[bc.case_id(c) for c in bc.CASES])
def test_every_case_is_fused(c, f32):
    assert bc.is_fused(*c, f32) == 1
    t, LP, loc = bc.placement(*c, f32)
    print(f"BATCHED case {bc.case_id(c)} {t}: LP {LP}, panels in {loc}, workspace {bc.workspace_bytes(*c, f32)}")
    assert (t, LP, loc) in bc.REACHABLE


def test_table_covers_every_reachable_instantiation():
    have = {bc.placement(*c, f32) for c in bc.CASES for f32 in (False, True)}
    assert have == set(bc.REACHABLE), set(bc.REACHABLE) ^ have
    # and the compress rows reach every width the tail is compiled for, in both types and both locations
    comp = {bc.placement(*c, f32) for c in bc.COMPRESS_CASES for f32 in (False, True)}
    assert {(t, LP) for t, LP, _ in comp} == {(t, LP) for t in ("f64", "f32") for LP in (32, 48, 64)}
    assert {("f64", 48, "lds"), ("f64", 48, "ws"), ("f64", 64, "lds"), ("f64", 64, "ws"), ("f32", 64, "lds"),
            ("f32", 64, "ws")} <= comp


def test_placement_does_not_depend_on_q_or_batch():
    for c in bc.CASES:
        m, n, l, q = c
        for f32 in (False, True):
            assert bc.placement(m, n, l, q, f32, batch=2) == bc.placement(m, n, l, 0, f32, batch=1)


@pytest.mark.parametrize("t,inside,past", bc.BUDGET_PAIRS, ids=[p[0] for p in bc.BUDGET_PAIRS])
def test_budget_pairs_straddle_the_boundary(t, inside, past):
    f32 = t == "f32"
    m, n0, l, q = inside
    assert past == (m, n0 + 1, l, q)
    first = next((n for n in range(l, 257) if bc.workspace_bytes(m, n, l, q, f32) > bc.LDS_FLOOR), None)
    assert first is not None, "no n <= 256 leaves LDS at this (m, l, type)"
    # the budget is monotone in n: nothing past `first` comes back
    assert all(bc.workspace_bytes(m, n, l, q, f32) > bc.LDS_FLOOR for n in range(first, 257))
    assert first == past[1], (first, past)
    assert bc.workspace_bytes(*inside, f32) == bc.LDS_FLOOR < bc.workspace_bytes(*past, f32)
    # two slices for a batch of two, each the 256-byte-rounded panels
    es = 4 if f32 else 8
    assert bc.workspace_bytes(*past, f32, batch=2) == 2 * ((es * (m + past[1]) * l + 255) // 256 * 256)
