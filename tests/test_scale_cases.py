"""CPU checks behind tests/test_gpu_scale.py: what the GPU tests expect is mathematics the oracle
agrees with bit for bit, the scaled inputs are exact and inside the declared window, the defect the
scaled runs are there for is stated in numbers, and the checker can fail.
"""
import numpy as np
import pytest

import oracle
import scale_cases as sc

SMALL = [c.id for c in sc.CASES if c.l <= 65 and not c.id.endswith("_a")]


def _bits_equal(X, Y):
    return X.shape == Y.shape and np.array_equal(np.ascontiguousarray(X).view(np.uint64),
                                                 np.ascontiguousarray(Y).view(np.uint64))


# ---- the oracle is equivariant, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("cid", SMALL)
def test_oracle_rsvd_is_equivariant(cid):
    c = sc.BY_ID[cid]
    _, _, A, Om = sc.inputs(cid)
    Uo, So, Vo = sc.oracle_result(cid)
    Qo = oracle.intermediate_step(A, Om, q=c.q)
    for k in c.ks:
        Ak = sc.exact_scaled(cid, k)
        U, S, V = oracle.rsvd(Ak, c.l, q=c.q, Omega=Om)
        assert _bits_equal(U, Uo) and _bits_equal(V, Vo), (cid, k)
        assert _bits_equal(S, np.ldexp(So, k)), (cid, k)
        assert _bits_equal(oracle.intermediate_step(Ak, Om, q=c.q), Qo), (cid, k)


@pytest.mark.parametrize("t,k", [(t, k) for t in ("f32", "f64") for k in sc.DENSE_KS[t]])
def test_oracle_dense_is_equivariant(t, k):
    """On the matrices the GPU rows use: the fp64 ones and, for the fp32 rows, their fp32 roundings."""
    f32 = t == "f32"
    A = sc.dense_matrix("qr", f32)
    for full in (False, True):
        Q, R = sc.dense_qr_oracle(full, f32)
        Qk, Rk = (oracle.givens_qr_full if full else oracle.givens_qr_reduced)(np.ldexp(A, k))
        assert _bits_equal(Qk, Q) and _bits_equal(Rk, np.ldexp(R, k)), full
    for name in ("sv_small", "sv_big"):
        A = sc.dense_matrix(name, f32)
        U, S, V, _ = sc.dense_svd_oracle(name, f32)
        Uk, Sk, Vk, _ = oracle.jacobi_svd(np.ldexp(A, k))
        assert _bits_equal(Uk, U) and _bits_equal(Vk, V) and _bits_equal(Sk, np.ldexp(S, k)), name


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_oracle_batch_is_equivariant(t):
    """The 70 x 45 matrices of the batched and compress rows, each at the 2^k its batch position takes
    (the out-of-range positions included: the oracle is fp64)."""
    m, n, l, q = sc.BATCH_SHAPE
    for ks in (sc.BATCH_KS[t],) + ((sc.BATCH_OUT_KS,) if t == "f32" else ()):
        for b, k in enumerate(ks):
            Uo, So, Vo = sc.batch_oracle(t, b)
            U, S, V = oracle.rsvd(np.ldexp(np.array(sc.batch_matrix(t, b)), k), l, q=q, Omega=sc.batch_omega(t, b))
            assert _bits_equal(U, Uo) and _bits_equal(V, Vo) and _bits_equal(S, np.ldexp(So, k)), (t, b, k)


# ---- the stored inputs are exact -----------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in sc.CASES if c.dtype in ("f32", "bf16") and c.via == "A"])
def test_storage_is_exact(cid):
    """quantise(ldexp(A, k)) == ldexp(quantise(A), k) bit for bit, nothing stored subnormal or infinite."""
    import torch

    c = sc.BY_ID[cid]
    stored, _, exact, _ = sc.inputs(cid)
    tdt = rc_dtype(c.dtype)
    tiny = float(torch.finfo(tdt).tiny)
    A = rc_raw(cid)
    for k in c.ks:
        direct, _, _ = sc.rc.quantise(np.ldexp(A, k), c.dtype)
        scaled = sc.scale_stored(stored, k)
        assert torch.equal(direct.view(torch.int16 if c.dtype == "bf16" else torch.int32),
                           scaled.view(torch.int16 if c.dtype == "bf16" else torch.int32)), (cid, k)
        x = scaled.to(torch.float64).numpy()
        assert np.array_equal(x, np.ldexp(exact, k))
        nz = np.abs(x[x != 0])
        assert np.isfinite(x).all() and nz.min() >= tiny, (cid, k, nz.min())


def rc_dtype(dtype):
    return sc.rc._torch_dtype(dtype)


def rc_raw(cid):
    """The fp64 matrix of the case before quantisation (the builder's own output)."""
    c = sc.BY_ID[cid]
    r = sc.rc.BY_ID[c.ragged] if c.ragged else None
    decay, seed = (r.decay, r.seed) if r else (sc.rc.case_decay(c.dtype, c.l), c.m + 3 * c.l + c.q)
    return sc.rc.tail_weighted(c.m, c.n, 2 * c.l, decay, seed)


def test_storage_is_exact_f64():
    for c in sc.CASES:
        if c.dtype != "f64":
            continue
        _, _, exact, _ = sc.inputs(c.id)
        for k in c.ks:
            x = np.ldexp(exact, k)
            assert np.array_equal(np.ldexp(x, -k), exact)
            nz = np.abs(x[x != 0])
            assert np.isfinite(x).all() and nz.min() >= np.finfo(np.float64).tiny


# ---- the inputs lie inside the declared window ----------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in sc.CASES])
def test_inputs_inside_window(cid):
    """rows (S[0] 2^k)^2 below the result type's maximum and (S[l-1] 2^k)^2 above its smallest normal: the
    squares of all singular values and sums of them over the rows are ordinary numbers of the result
    type, so a GPU failure at these k cannot be excused by the inputs.  |k| within the type's window."""
    c = sc.BY_ID[cid]
    _, So, _ = sc.oracle_result(cid)
    big, tiny = sc.RESULT_RANGE[sc.result_type(c.dtype)]
    kmax = 240 if c.dtype == "f64" else 40
    assert So[0] <= sc.SIGMA_MAX  # the figure include/rsvd_c.h states the window for
    for k in c.ks:
        assert abs(k) <= kmax
        hi = max(c.m, c.n) * float(np.ldexp(So[0], k)) ** 2
        lo = float(np.ldexp(So[c.l - 1], k)) ** 2
        assert hi < big and lo > tiny, (cid, k, hi, lo)


def test_batch_inputs_inside_window():
    m, n, l, q = sc.BATCH_SHAPE
    for t in ("f32", "f64"):
        big, tiny = sc.RESULT_RANGE[t]
        for b, k in enumerate(sc.BATCH_KS[t]):
            So = sc.batch_oracle(t, b)[1]
            assert max(m, n) * float(np.ldexp(So[0], k)) ** 2 < big and float(np.ldexp(So[l - 1], k)) ** 2 > tiny


# ---- the defect, in numbers -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [40, -40])
def test_fp32_rotation_test_fails_at_the_window_edge(k):
    """The rotation test of small_svd_kernel<float, float, LP> and of the batched Jacobi, restated in
    fp32 on unscaled operands: at sigma = 2^k, two columns at |cos| = 0.5 -- far from orthogonal --
    are NOT rotated, because both sides of `gg > tol2 * ab` are fourth powers of sigma (inf > inf at
    k = +40, 0 > 0 at k = -40).  At magnitude 1 the same pair rotates.  This documents the defect the
    kernels' exact scaling of W removes and guards the window arithmetic; it does not test the kernel."""
    sigma = float(np.ldexp(1.0, k))
    rot, gg, rhs = sc.rotation_test_f32(sigma, sigma, 0.5, 16)
    assert not rot, (gg, rhs)
    assert (np.isinf(gg) and np.isinf(rhs)) if k > 0 else (gg == 0.0 and rhs == 0.0)
    assert sc.rotation_test_f32(1.0, 1.0, 0.5, 16)[0]
    # ... while the squares themselves are ordinary fp32 numbers
    assert np.isfinite(np.float32(sigma) ** 2) and np.float32(sigma) ** 2 >= np.finfo(np.float32).tiny


# ---- the checker can fail -----------------------------------------------------------------------------------
def test_checker_passes_on_the_oracle_and_fails_on_wrong_results():
    cid, k = "n32a", 40
    bounds = (1e-4, 1e-4, 1e-4)
    Uo, So, Vo = (np.array(x) for x in sc.oracle_result(cid))
    sc.check(cid, k, Uo, np.ldexp(So, k), Vo, bounds)
    with pytest.raises(AssertionError):  # S left unscaled
        sc.check(cid, k, Uo, So, Vo, bounds)
    # one rotation undone: columns 0 and 1 of U and V mixed by 1e-3 rad (the product U S V^T moves by
    # 1e-3 (S0 - S1), the vectors by 1e-3: ten times the bar)
    t = 1e-3
    G = np.eye(len(So))
    G[:2, :2] = [[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]
    with pytest.raises(AssertionError):
        sc.check(cid, k, Uo @ G, np.ldexp(So, k), Vo @ G, bounds)
    Sz = np.ldexp(So, k)
    Sz[-1] = 0.0  # a singular value written as zero
    with pytest.raises(AssertionError):
        sc.check(cid, k, Uo, Sz, Vo, bounds)
