"""The real projection planner (csrc/wide_plan.cpp) against its Python mirror (tests/ragged_cases.py).

tests/cpp/plan_dump.cpp is built with the host compiler from wide_plan.cpp alone (no library, no
GPU) and answers queries `rows K LP v2 nn fp8` with `blocks splits chunk merge s8_scaled` and the
kernel of the hi / lo and of the single-panel product.  Compared with the mirror -- plan_wproj,
_nn_kernel / _tn_kernel and plan()'s s8 / sc rule -- on a full grid and on the wnn / wtn pair of every
low-precision row of ragged_cases.CASES.  The mirror keeps its own flag names; the map from the
engine's kernel names to the mirror's is written here.  Each A/B switch of the environment is read
once per process, so each is checked in a process of its own.
"""
import itertools
import os
import subprocess

import pytest

import ragged_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
SWITCHES = ("RSVD_TN128", "RSVD_NN8", "RSVD_NN3_128")

SIZES = [140, 150, 300, 701, 702, 1000, 1024, 1032, 1040, 1056, 1088, 1152, 2048, 4096, 8192, 65536, 131072, 2 ** 20]
LPS = [16, 32, 64, 128, 256, 512]

# wproj_kernel_name (csrc/wide_plan.cpp) -> the mirror's name: the double-step and the two-half forms
# of wproj2_kernel are both its "wproj2", and it calls wproj3_kernel's NN at LP = 128 "wproj3nn128"
MIRROR_NAME = {"wproj": "wproj", "wproj2": "wproj2", "wproj2_ds": "wproj2", "wproj2_half": "wproj2",
               "wproj3": "wproj3", "wproj3tn2": "wproj3tn2", "wproj3tn128": "wproj3tn128",
               "wproj3tn4": "wproj3tn4", "wproj3nn8": "wproj3nn8"}
# the e4m3 sketch (launch_wproj_s8) beside the plan's NN kernel: wproj2_kernel's S8 form, whole at
# LP = 256 and as halves at LP = 512, whichever kernel the hi / lo products take there
S8_NAME = {"wproj2": "wproj2_s8", "wproj2_half": "wproj2_half_s8", "wproj3nn8": "wproj2_half_s8"}


def mirror_name(kernel, LP, nn):
    return "wproj3nn128" if (kernel == "wproj3" and nn and LP == 128) else MIRROR_NAME[kernel]


@pytest.fixture(scope="module")
def plan_dump():
    subprocess.run(["make", "-C", CPP, "-s", "plan_dump"], check=True, capture_output=True)
    exe = os.path.join(CPP, "plan_dump")

    def ask(queries, **switches):
        """The planner's answers to (rows, K, LP, v2, nn, fp8) queries, all in one process."""
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(switches)
        text = "".join("%d %d %d %d %d %d\n" % tuple(int(x) for x in q) for q in queries)
        out = subprocess.run([exe], input=text, env=env, check=True, capture_output=True, text=True).stdout.split("\n")
        assert len(out) == len(queries) + 1 and out[-1] == ""
        ans = []
        for line in out[:-1]:
            f = line.split()
            ans.append(dict(blocks=int(f[0]), splits=int(f[1]), chunk=int(f[2]), merge=bool(int(f[3])),
                            s8_scaled=bool(int(f[4])), split=f[5], single=f[6]))
        return ans

    return ask


def check_against_mirror(q, got, p, sketch, sc):
    """One answer of the planner against the mirror's plan p, its single-panel / sketch kernel and
    (where the e4m3 sketch runs on the fp8 MFMA) its block-scaled flag sc, else None."""
    rows, K, LP, v2, nn, fp8 = q
    for key in ("blocks", "splits", "chunk", "merge"):
        assert got[key] == p[key], (q, key, got, p)
    want = rc._nn_kernel(p, LP, fp8, True) if nn else rc._tn_kernel(p, LP, fp8)
    assert mirror_name(got["split"], LP, nn) == want, (q, got, want)
    if sc is None:
        assert not got["s8_scaled"], (q, got)
        assert mirror_name(got["single"], LP, nn) == sketch, (q, got, sketch)
    else:
        assert got["s8_scaled"] == sc, (q, got, sc)
        assert S8_NAME[got["split"]] + ("_sc" if got["s8_scaled"] else "") == sketch, (q, got, sketch)


def test_grid_against_mirror(plan_dump):
    queries = [(rows, K, LP, v2, nn, fp8) for LP in LPS for v2, nn, fp8 in itertools.product((0, 1), repeat=3)
               for rows, K in itertools.product(SIZES, SIZES)]
    answers = plan_dump(queries)
    kernels = set()
    for q, got in zip(queries, answers):
        rows, K, LP, v2, nn, fp8 = q
        p = rc.plan_wproj(rows, K, LP, bool(v2), bool(nn), bool(fp8))
        # plan()'s rule for the sketch: e4m3 x e4m3 on an LDS-DMA NN plan at LP 256 / 512, block-scaled
        # when K = n and the chunk are whole 128-deep stages; else the NN kernel of a single panel
        if nn and fp8 and p["v2"] and LP in (256, 512):
            sc = K % 128 == 0 and p["chunk"] % 128 == 0
            sketch = ("wproj2_half_s8" if p["half"] else "wproj2_s8") + ("_sc" if sc else "")
        else:
            sc = None
            sketch = rc._nn_kernel(p, LP, fp8, False) if nn else rc._tn_kernel(p, LP, fp8)
        check_against_mirror(q, got, p, sketch, sc)
        kernels.add(got["split"])
    # the grid reaches every kernel the default switches allow
    assert kernels == set(MIRROR_NAME) - {"wproj2_ds", "wproj2_half"}


def test_case_table_against_mirror(plan_dump):
    lowp = [c for c in rc.CASES if c.dtype in ("bf16", "e4m3")]
    assert len(lowp) == 24
    queries, wants = [], []
    for c in lowp:
        P = rc.plan(c.dtype, c.m, c.n, c.l)
        fp8 = c.dtype == "e4m3"
        queries.append((c.m, c.n, P["LP"], P["v2"], 1, fp8))
        wants.append((P["wnn"], P["sketch"], P.get("sc")))
        queries.append((c.n, c.m, P["LP"], P["v2"], 0, fp8))
        wants.append((P["wtn"], P["tn"], None))
        assert P["nn"] == rc._nn_kernel(P["wnn"], P["LP"], fp8, True) and (P["s8"] or "sc" not in P)
    for q, got, (p, sketch, sc) in zip(queries, plan_dump(queries), wants):
        check_against_mirror(q, got, p, sketch, sc)


def _query(cid, nn):
    c = rc.BY_ID[cid]
    P = rc.plan(c.dtype, c.m, c.n, c.l)
    assert P["v2"]
    return (c.m, c.n, P["LP"], 1, 1, c.dtype == "e4m3") if nn else (c.n, c.m, P["LP"], 1, 0, c.dtype == "e4m3")


@pytest.mark.parametrize("switch, cid, nn, on, off", [
    ("RSVD_TN128", "b128d", False, ("wproj3tn128", "wproj3tn128"), ("wproj2_ds", "wproj2_ds")),
    ("RSVD_NN8", "e512n", True, ("wproj3nn8", "wproj3nn8"), ("wproj2_half", "wproj2_half")),
    ("RSVD_NN3_128", "b128v", True, ("wproj3", "wproj2"), ("wproj2", "wproj2")),
])
def test_switch_off_takes_the_older_kernel(plan_dump, switch, cid, nn, on, off):
    """<switch>=0 moves the case's product to the kernel it replaced and leaves the rest of the plan."""
    q = _query(cid, nn)
    (dflt,), (sw,) = plan_dump([q]), plan_dump([q], **{switch: "0"})
    assert (dflt["split"], dflt["single"]) == on
    assert (sw["split"], sw["single"]) == off
    for key in ("blocks", "splits", "chunk", "merge", "s8_scaled"):
        assert sw[key] == dflt[key], (key, sw, dflt)
