"""CPU: the POD C ABI (include/rsvd_c.h ABI 9: rsvd_pod, rsvd_pod_workspace_bytes, rsvd_pod_plan,
rsvd_pod_host_f64) -- exports, the host-only planning calls with the status codes rsvd_pod returns, and
pod_rank against a literal transcription of the reference's rank rule (POD.cpp:203-216)."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest

import rsvd_kamaneh_raganato_terrana_amd as R
from conftest import REPO
from rsvd_kamaneh_raganato_terrana_amd import _capi

OK, INVALID, UNSUPPORTED = 0, 1, 2
NEW = ("rsvd_pod", "rsvd_pod_workspace_bytes", "rsvd_pod_plan", "rsvd_pod_host_f64")


@pytest.fixture(scope="module")
def lib():
    R.build(force=False)
    return _capi.lib()


def _desc(**kw):
    d = dict(nh=1000, ns=40, lds=1000, r=10, dtype=_capi.F32, svd_type=4, q=2, flags=0, reserved=0, seed=0, tol=0.05)
    d.update(kw)
    return _capi.PodDesc(**d)


def _bytes(lib, has_xh=0, **kw):
    d, nb = _desc(**kw), ctypes.c_size_t(0)
    return lib.rsvd_pod_workspace_bytes(ctypes.byref(d), has_xh, ctypes.byref(nb)), nb.value


def _plan(lib, **kw):
    d, t, c = _desc(**kw), ctypes.c_int32(0), ctypes.c_int32(0)
    return lib.rsvd_pod_plan(ctypes.byref(d), ctypes.byref(t), ctypes.byref(c)), t.value, c.value


def test_pod_desc_is_64_bytes():
    assert ctypes.sizeof(_capi.PodDesc) == 64 and ctypes.sizeof(_capi.Csr) == 32


def test_library_exports_the_pod_symbols(lib):
    assert lib.rsvd_abi_version() >= 9
    assert set(NEW) <= set(_capi.EXPORTS)
    with open(f"{REPO}/include/rsvd_c.h") as f:
        declared = set(re.findall(r"^\w[\w \*]*?\b(rsvd_\w+)\(", f.read(), re.M))
    assert set(NEW) <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


@pytest.mark.parametrize("kw,status", [
    (dict(), OK),
    (dict(dtype=_capi.F64, svd_type=1), OK), (dict(svd_type=2), OK), (dict(svd_type=5), OK),
    (dict(flags=_capi.POD_FLAG_TEXTBOOK), OK), (dict(tol=0.0), OK), (dict(tol=1.0), OK), (dict(r=40), OK),
    (dict(lds=1003), OK), (dict(nh=40, lds=40), OK),
    (dict(r=0), INVALID), (dict(r=41), INVALID), (dict(lds=999), INVALID),
    (dict(tol=-0.1), INVALID), (dict(tol=1.5), INVALID), (dict(tol=math.nan), INVALID),
    (dict(svd_type=-1), INVALID), (dict(svd_type=6), INVALID), (dict(flags=2), INVALID), (dict(q=-1), INVALID),
    (dict(nh=39, lds=39), UNSUPPORTED),                       # ns > nh: the reference's K = S S^T branch
    (dict(nh=5000, lds=5000, ns=4097, r=10), UNSUPPORTED),
    (dict(svd_type=0), UNSUPPORTED), (dict(svd_type=3), UNSUPPORTED),
    (dict(dtype=_capi.BF16), UNSUPPORTED), (dict(dtype=_capi.FP8_E4M3), UNSUPPORTED),
])
def test_status_codes_of_the_planning_calls(lib, kw, status):
    assert _bytes(lib, **kw)[0] == status
    assert _plan(lib, **kw)[0] == status


def test_null_arguments(lib):
    d, nb = _desc(), ctypes.c_size_t(0)
    assert lib.rsvd_pod_workspace_bytes(None, 0, ctypes.byref(nb)) == INVALID
    assert lib.rsvd_pod_workspace_bytes(ctypes.byref(d), 0, None) == INVALID
    assert lib.rsvd_pod_plan(ctypes.byref(d), None, None) == INVALID
    assert lib.rsvd_pod(None, ctypes.byref(d), None, None, None, None, 0, None, None, None) == INVALID


def test_workspace_grows_with_rows_and_with_xh(lib):
    st, small = _bytes(lib, nh=20000, lds=20000)
    st2, tall = _bytes(lib, nh=2000000, lds=2000000)
    st3, with_xh = _bytes(lib, 1, nh=20000, lds=20000)
    assert st == st2 == st3 == OK
    assert tall > small                          # more row chunks, more slabs
    assert with_xh >= small + 8 * 20000 * 40     # T = Xh S, kept in fp64


def test_plan_is_a_function_of_the_shape(lib):
    st, tiles, chunks = _plan(lib, nh=20011, lds=20011, ns=24, r=8)
    assert st == OK and tiles == 1 and chunks > 1
    assert _plan(lib, nh=20011, lds=20500, ns=24, r=3, svd_type=1, tol=0.5, seed=9) == (OK, tiles, chunks)
    assert _plan(lib, nh=517, lds=517, ns=130, r=16)[1] == 15   # 5 x 5 blocks of 32: 15 upper pairs
    assert _plan(lib, nh=65, lds=65, ns=1, r=1)[1:] == (1, 1)


def _literal(sigma, r, tol):
    """POD.cpp:203-216, line by line."""
    N = 0
    I = 0.0
    num = 0.0
    sigma2 = np.zeros(r)
    for i in range(r):
        sigma2[i] = math.pow(sigma[i], 2)
    den = sigma2.sum()
    while I < (1 - math.pow(tol, 2)) and (N < r):
        num += sigma2[N]
        with np.errstate(invalid="ignore"):
            I = np.float64(num) / np.float64(den)
        N += 1
    return N


def test_pod_rank_matches_the_reference_loop():
    rng = np.random.default_rng(5)
    for trial in range(200):
        r = int(rng.integers(1, 40))
        # (bounded below: Eigen's and numpy's sum() are not the sequential sum, and only a share within an
        # ulp of the threshold could tell them apart)
        sigma = np.sort(0.05 + rng.random(r) ** rng.integers(1, 8))[::-1]
        for tol in (0.0, 1.0, 0.05, float(rng.random())):
            assert R.pod_rank(sigma, tol) == _literal(sigma, r, tol), (trial, tol)
    assert R.pod_rank([3.0, 2.0, 1.0], 0.0) == 3 and R.pod_rank([3.0, 2.0, 1.0], 1.0) == 0


def test_pod_rank_zero_spectrum():
    """den == 0: rsvd_pod keeps no mode for any tol.  At tol = 1 that is the reference's loop too; below 1
    the literal loop runs once before its I turns NaN and answers 1 -- include/rsvd_c.h defines N = 0."""
    z = np.zeros(6)
    assert R.pod_rank(z, 1.0) == _literal(z, 6, 1.0) == 0
    assert R.pod_rank(z, 0.0) == 0 and R.pod_rank(z, 0.05) == 0
    assert _literal(z, 6, 0.0) == 1


def test_pod_rank_textbook_weights():
    s = np.array([4.0, 1.0, 0.25])
    assert R.pod_rank(s, 0.3, textbook=True) == R.pod_rank(np.sqrt(s), 0.3)


def test_python_argument_checks_need_no_device():
    with pytest.raises(ValueError):
        R.POD(np.ones((3, 5)), 2, 0.1)                      # ns > Nh
    with pytest.raises(ValueError):
        R.POD(np.ones((5, 3)), 2, 0.1, svd_type=0)
    with pytest.raises(ValueError):
        R.POD(np.ones((5, 3)), 2, 0.1, svd_type=6)
    with pytest.raises(ValueError):
        R.POD(np.ones((5, 3)), 2, 0.1, D=np.ones((3, 3)))   # a dense D must be diagonal
    p = R.POD()
    assert p.W is None and p.sigma is None
    rp, ci, va = R.api.dense_to_csr(np.array([[2.0, 0.0], [-1.0, 2.0]]))
    assert rp.tolist() == [0, 1, 3] and ci.tolist() == [0, 0, 1] and va.tolist() == [2.0, -1.0, 2.0]
