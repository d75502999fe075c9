"""Cases of the dense drop-ins QR() and SVD<method> (rsvd_qr / rsvd_svd, csrc/dense_api.cpp and
csrc/dense_big.cpp): the case table, the matrix builder, the references and a pure-Python mirror of
the dispatch (a plain helper module in the style of ragged_cases.py, shared by test_dense_cases.py
on the CPU and test_gpu_dense_ragged.py / test_gpu_workspace.py on the GPU).

Each row is the smallest shape that still takes its branch.  `branch` names what the row is there
for; it was derived by reading the dispatch:
  dense_lp            csrc/dense_api.cpp:47     k <= 64: rup(k, 16); beyond: rup(k, 32)
  QR                  csrc/dense_api.cpp:166-167, 371   K = max(Q columns, n); K > 512 -> qr_big
                      csrc/dense_big.cpp:38, 75, 211    512-column blocks, block LP = rup(min(Q columns, 512), 32)
                      csrc/dense_api.cpp:181            a square Q (full, or m == n): the det +1 rule
  SVD<Jacobi>         csrc/dense_api.cpp:193, 408       LP = dense_lp(min(m, n)); min(m, n) > 512 -> svd_big
                      csrc/dense_api.cpp:218-221        LP <= 64: launch_small_svd, beyond: launch_block_jacobi
                      csrc/dense_api.cpp:209-212        m < n: transpose_to_panel
                      csrc/dense_big.cpp:251-252        MR = rup(max(m, n), 32), LP = rup(min(m, n), 32)
  SVD<ParallelJacobi> csrc/dense_api.cpp:197, 215-217   pjacobi_ref on A (square) or on R_P; > 512 as Jacobi
  SVD<Power>          csrc/dense_api.cpp:245, 401       LP = rup(n, 16); n > 512 -> the grid kernel
                      csrc/dense.hip:1049               B in LDS up to LP 128, in global memory beyond
`dispatch()` below is that derivation as code; test_dense_cases.py checks the table against it.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

OPS = ("qr", "qrfull", "jacobi", "pjacobi", "power")
METHOD = {"jacobi": 0, "power": 1, "pjacobi": 2}  # rsvd_c.h RSVD_SVD_*
QR_BLOCK = 512
POWER_SEED = 77  # the power method's start vectors: Philox(seed + i)


def _rup(a, b):
    return (a + b - 1) // b * b


def dense_lp(k):
    return _rup(max(k, 1), 16) if k <= 64 else _rup(k, 32)


def dispatch(op, m, n):
    """The kernel path rsvd_qr / rsvd_svd take for this op and shape, and the padded widths."""
    if op in ("qr", "qrfull"):
        kq = m if op == "qrfull" else n
        K = max(kq, n)
        out = dict(det_sign=kq == m)
        if K > 512:
            out.update(path="big", LP=_rup(min(kq, QR_BLOCK), 32), blocks=(kq + QR_BLOCK - 1) // QR_BLOCK)
        else:
            out.update(path="panel", LP=dense_lp(K), blocks=1)
        return out
    k, rows = min(m, n), max(m, n)
    if op == "power":
        if n > 512:
            return dict(path="grid", LP=0)
        LP = _rup(n, 16)
        return dict(path="power", LP=LP, b_lds=LP <= 128)
    out = dict(wide=m < n)
    if k > 512:
        out.update(path="big", LP=_rup(k, 32), MR=_rup(rows, 32))
    elif op == "pjacobi":
        out.update(path="pjacobi_ref", LP=dense_lp(k), square=m == n)
    else:
        LP = dense_lp(k)
        out.update(path="small_svd" if LP <= 64 else "block_jacobi", LP=LP)
    return out


# ---- the case table --------------------------------------------------------------------------------
# r: SVD<Power>'s triplet count (0: min(m, n)); 0 for every other op.
Case = namedtuple("Case", "id op dtype m n r branch")


def _c(op, dtype, m, n, branch, r=0):
    rid = f"{op}-{dtype}-{m}x{n}" + (f"-r{r}" if r else "")
    return Case(rid, op, dtype, m, n, r, branch)


P, B, G = "panel", "big", "grid"
SS, BJ, PJ = "small_svd", "block_jacobi", "pjacobi_ref"

CASES = [
    # -- QR, reduced --------------------------------------------------------------------------------
    _c("qr", "f64", 1, 1, dict(path=P, LP=16, det_sign=True)),
    _c("qr", "f64", 7, 1, dict(path=P, LP=16)),
    _c("qr", "f64", 20, 17, dict(path=P, LP=32)),                 # fewer rows than LP
    _c("qr", "f64", 257, 16, dict(path=P, LP=16)),                # one row past trsm_rows_kernel's 256
    _c("qr", "f64", 131, 63, dict(path=P, LP=64)),
    _c("qr", "f64", 131, 64, dict(path=P, LP=64)),
    _c("qr", "f64", 131, 65, dict(path=P, LP=96)),
    _c("qr", "f64", 515, 511, dict(path=P, LP=512)),
    _c("qr", "f64", 513, 512, dict(path=P, LP=512)),              # LP 512, no padding: the two-level factor
    _c("qr", "f64", 517, 513, dict(path=B, LP=512, blocks=2)),    # a second block of one column
    _c("qr", "f32", 20, 17, dict(path=P, LP=32)),
    _c("qr", "f32", 131, 65, dict(path=P, LP=96)),
    _c("qr", "f32", 517, 513, dict(path=B, LP=512, blocks=2)),
    # -- QR, full -----------------------------------------------------------------------------------
    _c("qrfull", "f64", 17, 17, dict(path=P, LP=32, det_sign=True)),
    _c("qrfull", "f64", 65, 65, dict(path=P, LP=96, det_sign=True)),   # det_sign_kernel with padding
    _c("qrfull", "f64", 97, 33, dict(path=P, LP=128, det_sign=True)),
    _c("qrfull", "f64", 33, 97, dict(path=P, LP=128, det_sign=True)),  # LP from n, Q 33 x 33
    _c("qrfull", "f64", 512, 40, dict(path=P, LP=512)),
    _c("qrfull", "f64", 513, 40, dict(path=B, LP=512, blocks=2)),      # identity completion crossing a block
    _c("qrfull", "f64", 40, 513, dict(path=B, LP=64, blocks=1)),       # K = 40 on the big path
    _c("qrfull", "f32", 97, 33, dict(path=P, LP=128)),
    _c("qrfull", "f32", 33, 97, dict(path=P, LP=128)),
    # -- SVD<Jacobi> --------------------------------------------------------------------------------
    _c("jacobi", "f64", 1, 1, dict(path=SS, LP=16)),
    _c("jacobi", "f64", 7, 1, dict(path=SS, LP=16, wide=False)),
    _c("jacobi", "f64", 1, 7, dict(path=SS, LP=16, wide=True)),
    _c("jacobi", "f64", 20, 17, dict(path=SS, LP=32)),
    _c("jacobi", "f64", 17, 20, dict(path=SS, LP=32, wide=True)),
    _c("jacobi", "f64", 131, 63, dict(path=SS, LP=64)),
    _c("jacobi", "f64", 131, 64, dict(path=SS, LP=64)),
    _c("jacobi", "f64", 131, 65, dict(path=BJ, LP=96)),
    _c("jacobi", "f64", 65, 131, dict(path=BJ, LP=96, wide=True)),
    _c("jacobi", "f64", 203, 97, dict(path=BJ, LP=128)),
    _c("jacobi", "f64", 520, 512, dict(path=BJ, LP=512)),
    _c("jacobi", "f64", 520, 513, dict(path=B, LP=544, MR=544)),
    _c("jacobi", "f64", 513, 520, dict(path=B, LP=544, MR=544, wide=True)),
    _c("jacobi", "f32", 20, 17, dict(path=SS, LP=32)),
    _c("jacobi", "f32", 130, 64, dict(path=SS, LP=64)),
    _c("jacobi", "f32", 131, 65, dict(path=BJ, LP=96)),
    _c("jacobi", "f32", 65, 131, dict(path=BJ, LP=96, wide=True)),
    _c("jacobi", "f32", 520, 513, dict(path=B, LP=544)),
    # -- SVD<ParallelJacobi> ------------------------------------------------------------------------
    _c("pjacobi", "f64", 65, 65, dict(path=PJ, LP=96, square=True)),
    _c("pjacobi", "f64", 131, 65, dict(path=PJ, LP=96, square=False)),
    _c("pjacobi", "f64", 65, 131, dict(path=PJ, LP=96, wide=True)),
    _c("pjacobi", "f32", 65, 65, dict(path=PJ, LP=96, square=True)),   # the square path in fp32
    _c("pjacobi", "f32", 17, 20, dict(path=PJ, LP=32, wide=True)),
    # -- SVD<Power> (fp64 only) ---------------------------------------------------------------------
    # r = 0 only at 1 x 1.  On B = A^T A the triplets below sqrt(eps) sigma_0 (2 x 0.75^i < 3e-8: i >= 63)
    # are rounding noise, and where the sigma < 1e-12 stop then falls is decided by rounding (the oracle
    # stops 90 x 70 after 63 triplets), so the other rows ask for 8 triplets as test_gpu_dense.py's
    # 150 x 120 does; the grid rows keep test_svd_power_large_n_grid's small r.
    _c("power", "f64", 1, 1, dict(path="power", LP=16, b_lds=True)),
    _c("power", "f64", 90, 70, dict(path="power", LP=80, b_lds=True), r=8),  # gram_wide's half-empty last block
    _c("power", "f64", 150, 112, dict(path="power", LP=112, b_lds=True), r=8),
    _c("power", "f64", 200, 144, dict(path="power", LP=144, b_lds=False), r=8),  # first B in global memory
    _c("power", "f64", 600, 512, dict(path="power", LP=512, b_lds=False), r=4),
    _c("power", "f64", 600, 513, dict(path=G), r=4),                        # first grid
]
BY_ID = {c.id: c for c in CASES}

# Pitch and base: at least one row per op, dtype and path (panel kernels, dense_big.cpp, the grid
# power method), each with (dA, dQ or dU, dR or dV): the pads of lda, ldq / ldu and ldr / ldv.
PITCH_CASES = [
    ("qr-f64-131x65", (1, 3, 1)), ("qr-f64-517x513", (3, 1, 3)),
    ("qr-f32-131x65", (3, 1, 3)), ("qr-f32-517x513", (1, 3, 1)),
    ("qrfull-f64-97x33", (1, 1, 3)), ("qrfull-f64-33x97", (3, 3, 1)), ("qrfull-f64-513x40", (1, 3, 1)),
    ("qrfull-f32-97x33", (3, 1, 1)),
    ("jacobi-f64-131x64", (1, 3, 1)), ("jacobi-f64-65x131", (3, 1, 3)), ("jacobi-f64-520x513", (1, 1, 3)),
    ("jacobi-f64-513x520", (3, 3, 1)),
    # 20 x 17 in fp32: a dense U whose base and pitch (80 bytes) sit on 16 bytes against one that does
    # not.  (rsvd_svd passes launch_panel_gemm no bf16 split, so U comes from panel_gemm_kernel's
    # scalar stores, csrc/wide_panel.hip:134; panel_split_kernel's 16-byte `vec` stores are rsvd_run's.)
    ("jacobi-f32-20x17", (3, 1, 3)),
    ("jacobi-f32-130x64", (1, 3, 1)), ("jacobi-f32-65x131", (3, 1, 3)), ("jacobi-f32-520x513", (1, 3, 1)),
    ("pjacobi-f64-65x65", (1, 3, 1)), ("pjacobi-f64-65x131", (3, 1, 3)),
    ("pjacobi-f32-65x65", (3, 1, 3)), ("pjacobi-f32-17x20", (1, 3, 1)),
    ("power-f64-90x70-r8", (1, 3, 1)), ("power-f64-200x144-r8", (3, 1, 3)), ("power-f64-600x513-r4", (1, 3, 1)),
]


# ---- the matrix builder ----------------------------------------------------------------------------
def case_seed(c):
    return 7 * c.m + c.n + 1000 * OPS.index(c.op) + (500 if c.dtype == "f32" else 0)


def _spectrum_matrix(m, n, sig, seed):  # as test_gpu_dense.py
    rng = np.random.default_rng(seed)
    k = len(sig)
    X = np.linalg.qr(rng.standard_normal((m, k)))[0]
    Y = np.linalg.qr(rng.standard_normal((n, k)))[0]
    return np.asfortranarray((X * sig) @ Y.T)


def spectrum(c):
    """The singular values the builder gives an SVD case (None for the Gaussian QR inputs)."""
    k = min(c.m, c.n)
    if c.op in ("qr", "qrfull"):
        return None
    if c.op == "power":
        return 2.0 * 0.75 ** np.arange(k if c.n <= 128 else min(k, 40))
    return (0.97 ** np.arange(k) + 0.01) if k <= 128 else 0.99 ** np.arange(k)


@lru_cache(maxsize=None)
def inputs(case_id):
    """The fp64 matrix the case stands for -- for an f32 row the fp32-rounded values, exactly what
    the GPU is given -- column-major and read-only."""
    c = BY_ID[case_id]
    sig = spectrum(c)
    if sig is None:
        A = np.random.default_rng(case_seed(c)).standard_normal((c.m, c.n))
    else:
        A = _spectrum_matrix(c.m, c.n, sig, case_seed(c))
    if c.dtype == "f32":
        A = A.astype(np.float32).astype(np.float64)
    A = np.asfortranarray(A)
    A.setflags(write=False)
    return A


def reference(c, A):
    """The reference's result on A: (Q, R) or (U, S, V) with V's columns the right singular vectors
    (SVD<Power>: cut to the triplets asked for and kept)."""
    import oracle

    if c.op == "qr":
        return oracle.givens_qr_reduced(A)
    if c.op == "qrfull":
        return oracle.givens_qr_full(A)
    k = min(c.m, c.n)
    if c.op == "power":
        U, S, V = oracle.power_svd(A, r=c.r, seed=POWER_SEED)
        dim = c.r or k
        # no row of the table stops early (see the table): U m x m, V n x n with v_i in ROW i
        assert U.shape == (c.m, c.m) and V.shape == (c.n, c.n) and np.all(S[:dim] > 0), (c.id, U.shape, V.shape)
        return np.asfortranarray(U[:, :dim]), S[:dim].copy(), np.asfortranarray(V[:dim, :].T)
    if c.op == "pjacobi":
        return oracle.jacobi_svd(A, parallel=True)[:3]
    if k <= 128:
        return oracle.jacobi_svd(A)[:3]
    U, S, Vt = np.linalg.svd(A, full_matrices=False)  # as test_svd_jacobi_big_f64
    return np.asfortranarray(U), S, np.asfortranarray(Vt.T)


@lru_cache(maxsize=None)
def oracle_result(case_id):
    """reference() on the case's inputs: computed once, shared, read-only."""
    out = reference(BY_ID[case_id], inputs(case_id))
    for x in out:
        x.setflags(write=False)
    return out


def perturbed(case_id):
    """The case's A moved by one ulp of its storage type, up or down by a fixed pattern: what the
    spread of the reference itself is measured with."""
    c = BY_ID[case_id]
    A = np.array(inputs(case_id))
    up = np.random.default_rng(case_seed(c) + 1).integers(0, 2, A.shape).astype(bool)
    if c.dtype == "f32":
        a = A.astype(np.float32)
        return np.asfortranarray(np.where(up, np.nextafter(a, np.float32(np.inf)),
                                          np.nextafter(a, np.float32(-np.inf))).astype(np.float64))
    return np.asfortranarray(np.where(up, np.nextafter(A, np.inf), np.nextafter(A, -np.inf)))
