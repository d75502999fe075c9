"""rsvd_pod on the GPU (Engine.pod): the fp64 correlation kernel, parity of sigma / W / N with a numpy
fp64 restatement of POD.cpp:136-462, the rank rule, the textbook flag, reproducibility, layouts, edges
and status codes.

Reference (written here, not taken from oracle/): C_ref = (S^T (Xh S)) o sqrt(d d^T), symmetrised;
svd_type 1 / 2: numpy's SVD of C_ref; 4 / 5: oracle.rsvd(C_ref, r, q, Omega = Philox(seed)); then the
reference's rule and W_ref[:, i] = S D^1/2 V[:, i] / sigma_i.  fp32 cases round S first and compute the
reference in fp64 from the rounded data (Xh = tridiag(-1, 2, -1) is exact in fp32).
svd_type 2 is held to the same reference and bars as 1: rsvd_pod runs the converged Jacobi SVD for both
(rsvd_svd's ParallelJacobi, the reference's own loosely stopped iteration, measured 1.9e-9 on sigma and
2.5e-5 on W at 1037 x 37 against this reference, 7.8e-8 .. 1.8e-5 on W at the other shapes).  The textbook
test uses svd_type 1: only the SVD's V diagonalises C, an rSVD of width r leaves the reference's own
W^T Xh W 3.5e-4 from I.

Inputs: S = gapped_matrix(nh, ns, ns, decay 0.8, no noise, seed nh + ns), d_j = 0.05 + 0.1 (j mod 3).
Shapes, the smallest at which each part can go wrong: 1037 x 37 (ragged rows and columns), 517 x 130
(several column blocks, so off-diagonal block pairs), 20011 x 24 (more than one row chunk, asserted on the
plan), 48 x 48 with r = ns = nh, 65 x 1.

Bars: C 1e-10 (the error-word bar of test_gpu_compress.py; the worst-case rounding bound
nh 2^-53 || |S|^T |T| ||_F / || S^T T ||_F is computed from the reference and has to stay under a tenth
of it); sigma and W 1e-8 (fp64) / 1e-4 (fp32), test_gpu_batched.py's parity bars; W^T Xh W - I 1e-10 /
1e-4 with the textbook flag.  N is compared only after the reference's running shares are shown to stay
>= 1e-6 away from 1 - tol^2 (for the shares I_1 .. I_{r-1}: the comparison of I_r cannot change N, the
loop stops on N < r there).

test_corr_irregular_csr gives pod_spmm_kernel what the stencil never does -- empty rows, unsorted and
duplicate entries, column indices -1 and nh -- against the dense operator, at the same two bars (measured
3.8e-16 at 1037 x 37 and 3.2e-16 at 517 x 130, bounds 1.9e-13 and 9.4e-14)."""
import functools

import numpy as np
import pytest

import oracle
import padded
import ws_patterns
from conftest import gapped_matrix, rel_fro, sign_align

pytestmark = pytest.mark.gpu

SHAPES = [(1037, 37, 12), (517, 130, 16), (20011, 24, 8), (48, 48, 48), (65, 1, 1)]
SMALL_R = [s for s in SHAPES if 1 < s[2] <= 16]
TOL = 0.05
SEED = 7


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def _snap(nh, ns, f32):
    S = gapped_matrix(nh, ns, ns, decay=0.8, noise=0.0, seed=nh + ns)
    if f32:
        S = np.asfortranarray(S.astype(np.float32).astype(np.float64))
    S.setflags(write=False)
    return S


def _weights(ns):
    return 0.05 + 0.1 * (np.arange(ns) % 3)


def _tridiag_csr(nh):
    """tridiag(-1, 2, -1) as (rowptr, colind, val)."""
    rowptr, colind, val = [0], [], []
    for i in range(nh):
        for c, v in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
            if 0 <= c < nh:
                colind.append(c)
                val.append(v)
        rowptr.append(len(colind))
    return np.array(rowptr, np.int32), np.array(colind, np.int32), np.array(val)


def _apply_xh(S):
    T = 2.0 * S
    T[1:] -= S[:-1]
    T[:-1] -= S[1:]
    return T


def _shares(sig, textbook):
    w = np.asarray(sig, dtype=np.float64) if textbook else np.asarray(sig, dtype=np.float64) ** 2
    den = w.sum()
    return np.cumsum(w) / den if den > 0 else np.zeros_like(w)


def _rank(sig, tol, textbook=False):
    """POD.cpp:203-216; a zero spectrum keeps nothing (rsvd_pod's rule)."""
    w = [float(s) if textbook else float(s) ** 2 for s in sig]
    den = sum(w)
    if den == 0.0:
        return 0
    N, I, num = 0, 0.0, 0.0
    while I < 1.0 - tol * tol and N < len(w):
        num += w[N]
        I = num / den
        N += 1
    return N


def _margin(sig, tol, textbook=False):
    """Distance of the running shares that decide N (I_1 .. I_{r-1}) from 1 - tol^2."""
    sh = _shares(sig, textbook)[:-1]
    return float(np.min(np.abs(sh - (1.0 - tol * tol)))) if sh.size else 1.0


@functools.lru_cache(maxsize=None)
def _ref(nh, ns, r, f32, xh, dw, svd_type, textbook=False):
    S = _snap(nh, ns, f32)
    T = _apply_xh(S) if xh else S
    d = _weights(ns) if dw else np.ones(ns)
    C = (S.T @ T) * np.sqrt(np.outer(d, d))
    C = 0.5 * (C + C.T)
    if svd_type in (1, 2):
        _, sig, Vt = np.linalg.svd(C)
        V = Vt.T
    else:
        _, sig, V = oracle.rsvd(C, r, q=2, Omega=oracle.generate_omega(ns, r, SEED))
    sr = sig[:r]
    div = np.sqrt(sr) if textbook else sr
    W = (S * np.sqrt(d)) @ V[:, :r] / div
    absb = float(nh * 2.0 ** -53 * np.linalg.norm(np.abs(S).T @ np.abs(T)) / np.linalg.norm(S.T @ T))
    out = dict(C=C, sigma=sig, W=W, bound=absb)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _dev(S, f32):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(S.T)).cuda().t()  # column-major
    return t.float() if f32 else t


def _run(engine, nh, ns, r, f32=False, xh=False, dw=False, svd_type=4, tol=TOL, textbook=False, S=None, **kw):
    S = _dev(_snap(nh, ns, f32), f32) if S is None else S
    return engine.pod(S, r, tol, Xh=_tridiag_csr(nh) if xh else None, d=_weights(ns) if dw else None,
                      svd_type=svd_type, q=2, seed=SEED, textbook=textbook, **kw)


def _bits(t):
    """The tensor's bytes (W is a column-major view), so that NaNs would compare too."""
    torch = _torch()
    return (t.t().contiguous() if t.dim() == 2 else t.contiguous()).view(torch.uint8)


# ---- 1. the correlation kernel alone ------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("xh,dw", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "xh", "d", "xh_d"])
@pytest.mark.parametrize("nh,ns,r", SHAPES)
def test_corr(engine, nh, ns, r, xh, dw, f32):
    ref = _ref(nh, ns, r, f32, xh, dw, 4)
    if nh == 20011:
        assert engine.pod_plan(nh, ns, _torch().float32 if f32 else _torch().float64)[1] > 1
    C = _run(engine, nh, ns, r, f32, xh, dw, truncate=False, return_corr=True)[3]
    _torch().cuda.synchronize()
    assert _torch().equal(C, C.t())
    err = rel_fro(C.cpu().numpy(), ref["C"])
    print(f"C rel_fro {err:.3e}, worst-case bound {ref['bound']:.3e}")
    assert ref["bound"] < 1e-11, ref["bound"]
    assert err < 1e-10, err


# ---- 1b. the CSR product on an operator that is not a stencil -----------------------------------------------
@functools.lru_cache(maxsize=None)
def _irregular_operator(nh):
    """A symmetric nh x nh Xh, dense (the reference) and as CSR arrays made awkward on purpose.

    Dense: about 3 nh random off-diagonal pairs with values in [-1, 0); rows with i % 7 == 3 have none; the
    diagonal is 1 + the absolute row sum, except that rows 5, 16, 27, .. have a zero diagonal -- so rows that
    are both (38, 115, ..) are wholly empty.  Every value is rounded to fp32: the fp32 case is exact.
    CSR: the entries of a row in shuffled order, about a third of them split into two duplicates of half the
    value (exact), and rows with i % 5 == 0 that are not empty get two more entries with a non-zero value at
    column -1 and column nh, which pod_spmm_kernel documents that it skips."""
    rng = np.random.default_rng(4000 + nh)
    f32 = lambda x: np.float64(np.float32(x))
    X = np.zeros((nh, nh))
    for i, j, v in zip(rng.integers(0, nh, 3 * nh), rng.integers(0, nh, 3 * nh), rng.random(3 * nh) - 1.0):
        if i != j and i % 7 != 3 and j % 7 != 3:
            X[i, j] = X[j, i] = f32(v)
    for i in range(nh):
        X[i, i] = 0.0 if i % 11 == 5 else f32(1.0 + np.abs(X[i]).sum())
    assert np.array_equal(X, X.T) and np.array_equal(X, X.astype(np.float32).astype(np.float64))
    rowptr, colind, val = [0], [], []
    empty = 0
    for i in range(nh):
        ent = []
        for j in np.flatnonzero(X[i]):
            if rng.random() < 1.0 / 3.0:
                ent += [(int(j), 0.5 * X[i, j]), (int(j), 0.5 * X[i, j])]
            else:
                ent.append((int(j), X[i, j]))
        if ent and i % 5 == 0:
            ent += [(-1, 0.75), (nh, -1.5)]
        empty += not ent
        for e in rng.permutation(len(ent)):
            colind.append(ent[e][0])
            val.append(ent[e][1])
        rowptr.append(len(colind))
    val = np.array(val)
    assert empty >= 2 and np.array_equal(val, val.astype(np.float32).astype(np.float64))
    assert any(np.any(np.diff(colind[rowptr[i]:rowptr[i + 1]]) < 0) for i in range(nh))  # unsorted rows
    assert min(colind) == -1 and max(colind) == nh and len(colind) > np.count_nonzero(X) + 2
    X.setflags(write=False)
    return X, (np.array(rowptr, np.int32), np.array(colind, np.int32), val)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("nh,ns,r", [(1037, 37, 12), (517, 130, 16)])
def test_corr_irregular_csr(engine, nh, ns, r, f32):
    """pod_spmm_kernel on empty rows, unsorted and duplicate entries and out-of-range column indices, against
    the dense operator.  Only C is compared: this Xh is not meant to be a mass matrix.  The bound below does
    not count the fp64 sum of an operator row (at most about 15 terms here: 15 x 2^-53 more)."""
    torch = _torch()
    X, csr = _irregular_operator(nh)
    S, d = _snap(nh, ns, f32), _weights(ns)
    T = X @ S
    Cr = (S.T @ T) * np.sqrt(np.outer(d, d))
    Cr = 0.5 * (Cr + Cr.T)
    bound = float(nh * 2.0 ** -53 * np.linalg.norm(np.abs(S).T @ np.abs(T)) / np.linalg.norm(S.T @ T))
    C = engine.pod(_dev(S, f32), r, TOL, Xh=csr, d=d, svd_type=4, q=2, seed=SEED, truncate=False, return_corr=True)[3]
    torch.cuda.synchronize()
    assert torch.equal(C, C.t())
    err = rel_fro(C.cpu().numpy(), Cr)
    print(f"C (irregular CSR) rel_fro {err:.3e}, worst-case bound {bound:.3e}")
    assert bound < 1e-11, bound
    assert err < 1e-10, err
    engine.sync()


# ---- 2. parity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("svd_type", [1, 2, 4, 5])
@pytest.mark.parametrize("nh,ns,r", SHAPES)
def test_parity(engine, nh, ns, r, svd_type, f32):
    ref = _ref(nh, ns, r, f32, True, True, svd_type)
    W, sigma, N = _run(engine, nh, ns, r, f32, True, True, svd_type, truncate=False)
    engine.sync()
    sigma, W, N = sigma.cpu().numpy(), W.double().cpu().numpy(), int(N.item())
    bar = 1e-4 if f32 else 1e-8
    nsig = ns if svd_type in (1, 2) else r
    es = rel_fro(sigma[:r], ref["sigma"][:r])
    k = min(r, 8)
    ew = rel_fro(sign_align(W[:, :k], ref["W"][:, :k]), ref["W"][:, :k])
    margin = _margin(ref["sigma"][:r], TOL)
    print(f"sigma {es:.3e}  W[:, :{k}] {ew:.3e}  N {N}  margin {margin:.3e}")
    assert es < bar, es
    assert ew < bar, ew
    if svd_type in (1, 2):
        assert rel_fro(sigma[:nsig], ref["sigma"][:nsig]) < bar
    assert np.all(sigma[nsig:] == 0.0)
    assert margin >= 1e-6, margin
    assert N == _rank(ref["sigma"][:r], TOL)


# ---- 3. the rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("textbook", [False, True], ids=["default", "textbook"])
@pytest.mark.parametrize("nh,ns,r", [(1037, 37, 12), (20011, 24, 8)])
def test_rank_rule(engine, nh, ns, r, textbook):
    import rsvd_kamaneh_raganato_terrana_amd as R

    ref = _ref(nh, ns, r, False, True, True, 4)
    sr = ref["sigma"][:r]
    sh = _shares(sr, textbook)
    mid = float(np.sqrt(1.0 - 0.5 * (sh[2] + sh[3])))  # 1 - tol^2 midway between two consecutive shares
    for tol, want in ((0.0, r), (TOL, None), (1.0, 0), (mid, 4)):
        margin = _margin(sr, tol, textbook)
        assert margin >= 1e-6, (tol, margin)
        N = _run(engine, nh, ns, r, False, True, True, 4, tol=tol, textbook=textbook)[2]
        print(f"tol {tol:.4f}: N {N}, margin {margin:.3e}")
        assert N == R.pod_rank(sr, tol, textbook) == _rank(sr, tol, textbook)
        if want is not None:
            assert N == want


# ---- 4. the textbook flag -----------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("nh,ns,r", SMALL_R)
def test_textbook_orthonormal(engine, nh, ns, r, f32):
    ref = _ref(nh, ns, r, f32, True, True, 1, True)  # the SVD of C: an rSVD's V[:, :r] only nearly diagonalises C
    Wr = ref["W"]
    assert np.linalg.norm(Wr.T @ _apply_xh(Wr) - np.eye(r)) < 1e-13  # the reference's own W is Xh-orthonormal
    W = _run(engine, nh, ns, r, f32, True, True, 1, textbook=True, truncate=False)[0]
    engine.sync()
    W = W.double().cpu().numpy()
    dev = np.linalg.norm(W.T @ _apply_xh(W) - np.eye(r))
    print(f"|W^T Xh W - I|_F {dev:.3e}")
    assert dev < (1e-4 if f32 else 1e-10), dev


# ---- 5. reproducibility --------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_reproducible_over_workspace_fills(engine, f32):
    torch = _torch()
    nh, ns, r = 20011, 24, 8
    first = _run(engine, nh, ns, r, f32, True, True, 4, truncate=False, return_corr=True)
    engine.sync()
    first = [t.clone() for t in first]
    for fill in [None] + list(ws_patterns.PATTERNS.values()):
        if fill is not None:
            engine.workspace().fill_(fill)
        again = _run(engine, nh, ns, r, f32, True, True, 4, truncate=False, return_corr=True)
        engine.sync()
        for a, b in zip(first, again):
            assert torch.equal(_bits(a), _bits(b)), fill


# ---- 6. layout -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("nh,ns,r", [(1037, 37, 12), (517, 130, 16)])
def test_layout(engine, nh, ns, r, f32):
    torch = _torch()
    dt = torch.float32 if f32 else torch.float64
    Sp = _dev(_snap(nh, ns, f32), f32)
    packed = _run(engine, nh, ns, r, f32, True, True, 4, S=Sp, truncate=False, return_corr=True)
    engine.sync()
    lds = nh + 3
    buf = torch.zeros(1 + ns * lds, dtype=dt, device="cuda")
    So = buf[1:].view(ns, lds)[:, :nh].t()  # one element into the buffer, pitch nh + 3
    So.copy_(Sp)
    assert So.stride() == (1, lds) and So.data_ptr() == buf.data_ptr() + buf.element_size()
    out = padded._Padded(nh, r, nh + 5, dt)
    odd = _run(engine, nh, ns, r, f32, True, True, 4, S=So, truncate=False, return_corr=True, out=out.mat)
    engine.sync()
    assert out.padding_untouched()
    assert torch.equal(packed[0].contiguous(), odd[0].contiguous())
    for a, b in zip(packed[1:], odd[1:]):
        assert torch.equal(a, b)


# ---- 7. edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("svd_type", [1, 4])
def test_zero_snapshots(engine, svd_type):
    torch = _torch()
    nh, ns, r = 1037, 37, 12
    S = torch.zeros((ns, nh), dtype=torch.float64, device="cuda").t()
    W, sigma, N = _run(engine, nh, ns, r, False, True, True, svd_type, S=S, truncate=False)
    engine.sync()
    assert int(N.item()) == 0
    assert bool((sigma == 0).all()) and bool((W == 0).all())


def test_zero_last_column(engine):
    nh, ns, r = 1037, 37, 12
    S = np.array(_snap(nh, ns, False), order="F")
    S[:, -1] = 0.0
    T = _apply_xh(S)
    d = _weights(ns)
    C = (S.T @ T) * np.sqrt(np.outer(d, d))
    sig = np.linalg.svd(0.5 * (C + C.T), compute_uv=False)
    W, sigma, N = _run(engine, nh, ns, r, False, True, True, 1, S=_dev(S, False), truncate=False)
    engine.sync()
    sigma, W = sigma.cpu().numpy(), W.cpu().numpy()
    assert np.all(np.isfinite(sigma)) and np.all(np.isfinite(W))
    assert rel_fro(sigma[:r], sig[:r]) < 1e-8
    assert sigma[-1] <= 1e-12 * sigma[0]
    assert _margin(sig[:r], TOL) >= 1e-6
    assert int(N.item()) == _rank(sig[:r], TOL)


# ---- 8. status codes on the device path --------------------------------------------------------------------
def test_status_codes(engine):
    torch = _torch()
    from rsvd_kamaneh_raganato_terrana_amd import RSVDError

    S = torch.zeros((8, 32), dtype=torch.float64, device="cuda").t()  # 32 x 8
    for kw, status in ((dict(r=4, svd_type=0), 2), (dict(r=4, svd_type=3), 2), (dict(r=0), 1), (dict(r=9), 1),
                       (dict(r=4, svd_type=6), 1), (dict(r=4, tol=1.5), 1)):
        args = dict(r=4, tol=TOL, svd_type=4)
        args.update(kw)
        with pytest.raises(RSVDError) as e:
            engine.pod(S, args["r"], args["tol"], svd_type=args["svd_type"])
        assert e.value.status == status, kw
    with pytest.raises(RSVDError) as e:
        engine.pod(torch.zeros((32, 8), dtype=torch.float64, device="cuda").t(), 4, TOL)  # 8 x 32: ns > nh
    assert e.value.status == 2
    with pytest.raises(TypeError):
        engine.pod(S.half(), 4, TOL)
    # the handle still works afterwards
    assert _run(engine, 65, 1, 1)[2] in (0, 1)


# ---- 9. a non-default stream ---------------------------------------------------------------------------------
def test_non_default_stream(engine):
    torch = _torch()
    nh, ns, r = 1037, 37, 12
    S = _dev(_snap(nh, ns, False), False)
    ref = _run(engine, nh, ns, r, False, True, True, 4, S=S, truncate=False, return_corr=True)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        res = _run(engine, nh, ns, r, False, True, True, 4, S=S, truncate=False, return_corr=True)
    st.synchronize()
    for X, X0 in zip(res, ref):  # W, sigma, N, C
        assert torch.equal(_bits(X), _bits(X0))
    engine.sync()
