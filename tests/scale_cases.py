"""Cases at extreme magnitudes of A: the case table, the scaled inputs, the cached oracle results at
magnitude 1 and the checker (a plain helper module in the style of ragged_cases.py, shared by
test_scale_cases.py on the CPU and test_gpu_scale.py on the GPU).

The contract under test (include/rsvd_c.h, "dynamic range"): A 2^k has the singular values of A times
2^k and the singular vectors of A.  The oracle is bit-for-bit equivariant under that scaling
(test_scale_cases.py checks it), so the expected result of every scaled run is the oracle's result at
k = 0 with S -- or R, C, err2 -- scaled by ldexp, which is exact.

Inputs: A_k = ldexp(A_0, k) of the stored values (exact in fp32, bf16 and fp64: no stored entry comes
near the subnormals or the maximum of its type, which test_scale_cases.py asserts).  e4m3 keeps its
stored codes and takes a_scale = scale_0 2^k; the `a` variants of a case keep the stored A of k = 0
and pass a_scale = 2^k instead, which is legal for every dtype.

Windows: results delivered in fp32 (fp32, bf16 and e4m3 A) |k| <= 40; fp64 |k| <= 240.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import ragged_cases as rc

# ---- the rSVD rows ---------------------------------------------------------------------------------
# ragged: the row of ragged_cases.CASES with this shape (its inputs and oracle result are shared with
# test_gpu_ragged.py), or None for a shape of this table's own; via: "A" (A itself is scaled) or "a_scale".
Case = namedtuple("Case", "id dtype m n l q ks ragged via path")

F32_KS = (20, -20, 40, -40)
F64_KS = (40, -40, 240, -240)


def _c(id, dtype, m, n, l, q, ks, path, ragged=None, via="A"):
    return Case(id, dtype, m, n, l, q, tuple(ks), ragged, via, path)


CASES = [
    _c("n32a", "f32", 300, 200, 16, 2, F32_KS, "narrow fp32, small_svd_kernel<float, float, 16>"),
    _c("n32b", "f32", 1001, 333, 33, 2, F32_KS, "narrow fp32, small_svd_kernel<float, float, 48>", ragged="f32b"),
    _c("n64", "f64", 300, 200, 16, 2, F64_KS, "narrow fp64"),
    _c("w32", "f32", 601, 403, 65, 1, F32_KS, "wide-fp fp32, eigensolver small SVD (LP 128)"),
    _c("w64", "f64", 601, 403, 65, 1, F64_KS, "wide-fp fp64, persistent block Jacobi", ragged="f64a"),
    _c("b32", "bf16", 777, 555, 32, 2, F32_KS, "bf16, LP 32, one-workgroup fp64 Jacobi", ragged="b32"),
    _c("b128", "bf16", 1000, 702, 128, 1, F32_KS, "bf16, LP 128: split Gram, split panel products, eigensolver",
       ragged="b128v"),
    _c("b256", "bf16", 1032, 701, 256, 2, (40, -40), "bf16, LP 256, q = 2 (deferred second pass, G^-1/2 series)",
       ragged="b256v"),
    _c("e16", "e4m3", 777, 555, 16, 1, F32_KS, "e4m3 through a_scale, LP 16 fallback", ragged="e16", via="a_scale"),
    _c("e256", "e4m3", 1024, 300, 256, 1, F32_KS, "e4m3 through a_scale, LP 256 fp8-MFMA sketch", ragged="e256s",
       via="a_scale"),
    # a_scale = 2^k on a stored A of magnitude 1: one narrow fp32 case and one bf16 case
    _c("n32a_a", "f32", 300, 200, 16, 2, (40, -40), "narrow fp32, a_scale = 2^k", via="a_scale"),
    _c("b32_a", "bf16", 777, 555, 32, 2, (40, -40), "bf16 LP 32, a_scale = 2^k", ragged="b32", via="a_scale"),
]
BY_ID = {c.id: c for c in CASES}

# the range finder's Q (q = 0 and q = 1) at k = +-40
RF_CASES = [("n32a", 0), ("n32a", 1), ("b128", 0), ("b128", 1)]
# out of the window: k = +-100 must still meet the bars or end in RSVD_ERR_NUMERICAL
OUT_OF_RANGE_KS = (100, -100)

# the largest singular value of any case at k = 0 stays below this (include/rsvd_c.h states the windows
# for it; measured maximum 16.24, b256)
SIGMA_MAX = 16.3

# result type -> (largest finite value, smallest normal)
RESULT_RANGE = {"f32": (float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny)),
                "f64": (float(np.finfo(np.float64).max), float(np.finfo(np.float64).tiny))}


def result_type(dtype):
    return "f64" if dtype == "f64" else "f32"


def _base_id(cid):
    return cid[:-2] if cid.endswith("_a") else cid


@lru_cache(maxsize=None)
def inputs(cid):
    """(A stored [torch, m x n], a_scale, A exact [fp64], Omega exact [fp64]) at k = 0: the recipe of
    ragged_cases.inputs (tail_weighted, case_decay, quantise, the oracle's Philox Omega rounded to what
    the engine rounds it to), shared with it where the shape is one of its rows."""
    import oracle

    c = BY_ID[cid]
    if c.ragged:
        return rc.inputs(c.ragged)
    if cid != _base_id(cid):
        return inputs(_base_id(cid))
    seed = c.m + 3 * c.l + c.q
    A = rc.tail_weighted(c.m, c.n, 2 * c.l, rc.case_decay(c.dtype, c.l), seed)
    stored, scale, exact = rc.quantise(A, c.dtype)
    Om = np.asfortranarray(rc._round_to(oracle.generate_omega(c.n, c.l, 1000 + seed), c.dtype))
    for x in (exact, Om):
        x.setflags(write=False)
    return stored, scale, exact, Om


@lru_cache(maxsize=None)
def oracle_result(cid):
    """The fp64 oracle's (U, S, V) at k = 0: computed once, shared, read-only."""
    import oracle

    c = BY_ID[cid]
    if c.ragged:
        return rc.oracle_result(c.ragged)
    if cid != _base_id(cid):
        return oracle_result(_base_id(cid))
    _, _, A, Om = inputs(cid)
    out = oracle.rsvd(A, c.l, q=c.q, Omega=Om)
    for x in out:
        x.setflags(write=False)
    return out


def scale_stored(stored, k):
    """ldexp(stored, k) in the tensor's own type, through fp64 (exact: test_scale_cases.py)."""
    import torch

    x = np.ldexp(stored.to(torch.float64).numpy(), k)
    return torch.from_numpy(x).to(stored.dtype)


def scaled_inputs(cid, k):
    """(stored A to pass, a_scale to pass) of case `cid` at 2^k."""
    c = BY_ID[cid]
    stored, scale, _, _ = inputs(cid)
    if c.via == "a_scale":
        return stored, float(np.ldexp(scale, k))
    return scale_stored(stored, k), scale


def exact_scaled(cid, k):
    """The fp64 values A_k stands for -- what the oracle is given in the equivariance test."""
    return np.asfortranarray(np.ldexp(inputs(cid)[2], k))


# ---- the checker -----------------------------------------------------------------------------------
def sign_align(X, Xref):
    s = np.sign(np.sum(X * Xref, axis=0))
    s[s == 0] = 1.0
    return X * s


def rel_fro(X, Xref):
    den = np.linalg.norm(Xref)
    return np.linalg.norm(X - Xref) / (den if den > 0 else 1.0)


def check(cid, k, U, S, V, bounds, what=None):
    """(U, S, V): fp64 numpy arrays of a run at 2^k; bounds = (tol_s, tol_uv, orth_tol), the project's own
    for the dtype and LP.  Everything is compared at magnitude 1: ldexp(S, -k) is exact."""
    c = BY_ID[cid]
    what = what or f"{cid} k={k:+d}"
    _, _, A, _ = inputs(cid)
    Uo, So, Vo = oracle_result(cid)
    tol_s, tol_uv, orth = bounds
    l, h = c.l, c.l // 2
    finite = bool(np.isfinite(S).all() and np.isfinite(U).all() and np.isfinite(V).all())
    S1 = np.ldexp(S, -k)
    es = rel_fro(S1, So)
    eu = rel_fro(sign_align(U[:, :h], Uo[:, :h]), Uo[:, :h])
    ev = rel_fro(sign_align(V[:, :h], Vo[:, :h]), Vo[:, :h])
    ou = np.linalg.norm(U.T @ U - np.eye(l))
    ov = np.linalg.norm(V.T @ V - np.eye(l))
    e = np.linalg.norm(A - (U * S1) @ V.T)
    eo = np.linalg.norm(A - (Uo * So) @ Vo.T)
    print(f"SCALE {what}: S {es:.2e} U {eu:.2e} V {ev:.2e} orthU {ou:.2e} orthV {ov:.2e} "
          f"recon {e:.6e} oracle {eo:.6e} |A| {np.linalg.norm(A):.3e} S[0] {S[0]:.3e} S[-1] {S[-1]:.3e}")
    assert finite, what
    assert np.all(S > 0) and np.all(np.diff(S) <= 0), (what, S)
    assert es < tol_s, (what, es)
    assert eu < tol_uv and ev < tol_uv, (what, eu, ev)
    assert ou < orth and ov < orth, (what, ou, ov)
    assert abs(e - eo) <= 10 * tol_s * np.linalg.norm(A), (what, e, eo)
    return es, eu, ev


# ---- the batched rows ------------------------------------------------------------------------------
# one batch of four 70 x 45 matrices, l = 8, q = 2 (and the compress tail at rank 4); matrix b is scaled
# by 2^BATCH_KS[type][b] in ONE launch
BATCH_SHAPE = (70, 45, 8, 2)
BATCH_RANK = 4
BATCH_KS = {"f32": (0, 40, -40, 20), "f64": (0, 240, -240, 40)}
BATCH_OUT_KS = (0, 100, -100, 0)  # fp32 only: matrices 1 and 2 out of the window


# ---- the rotation test of the one-workgroup Jacobi, restated in fp32 -------------------------------
def rotation_test_f32(sigma_p, sigma_q, cosine, l):
    """(rotates, gg, tol2 ab) of `gg > tol2 * ab` as small_svd_kernel<float, float, LP> evaluated it before
    W was scaled (csrc/jacobi.hip): a, b the squared norms of two columns of norm sigma_p and sigma_q,
    g their dot product, every product in fp32."""
    f = np.float32
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a, b = f(sigma_p) * f(sigma_p), f(sigma_q) * f(sigma_q)
        g = f(cosine) * f(sigma_p) * f(sigma_q)
        tol = f(l * 1.1920928955078125e-07)
        gg, ab = g * g, a * b
        rhs = tol * tol * ab
        return bool(g != 0 and gg > rhs), float(gg), float(rhs)


def batch_matrix(t, b):
    """Matrix b of the batch at magnitude 1: the family (and the cache) of test_gpu_batched.py."""
    import test_gpu_batched as TB

    m, n, l, _ = BATCH_SHAPE
    return TB._matrix(m, n, l, b, t == "f32")


def batch_omega(t, b):
    import test_gpu_batched as TB

    _, n, l, _ = BATCH_SHAPE
    return TB._omega(n, l, b, t == "f32")


def batch_oracle(t, b):
    """The oracle's (U, S, V) of matrix b with Omega b at magnitude 1 (test_gpu_batched's cache)."""
    import test_gpu_batched as TB

    m, n, l, q = BATCH_SHAPE
    return TB._ref(m, n, l, q, b, b, t == "f32")


# ---- the dense rows ----------------------------------------------------------------------------------
DENSE_SHAPES = {"qr": (200, 60), "sv_small": (120, 60), "sv_big": (300, 130)}
DENSE_KS = {"f32": (40, -40), "f64": (40, -40, 240, -240)}


@lru_cache(maxsize=None)
def dense_matrix(name, f32=False):
    """qr: standard normal entries; sv_*: the gapped spectrum 0.97^i + 0.01 of test_gpu_dense.py."""
    m, n = DENSE_SHAPES[name]
    rng = np.random.default_rng(m * 7 + n)
    if name == "qr":
        A = rng.standard_normal((m, n))
    else:
        k = min(m, n)
        X = np.linalg.qr(rng.standard_normal((m, k)))[0]
        Y = np.linalg.qr(rng.standard_normal((n, k)))[0]
        A = (X * (0.97 ** np.arange(k) + 0.01)) @ Y.T
    if f32:
        A = A.astype(np.float32).astype(np.float64)
    A = np.asfortranarray(A)
    A.setflags(write=False)
    return A


@lru_cache(maxsize=None)
def dense_svd_oracle(name, f32=False):
    import oracle

    return oracle.jacobi_svd(dense_matrix(name, f32))


@lru_cache(maxsize=None)
def dense_qr_oracle(full, f32=False):
    import oracle

    A = dense_matrix("qr", f32)
    return oracle.givens_qr_full(A) if full else oracle.givens_qr_reduced(A)
