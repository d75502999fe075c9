"""GPU parity of the QR() and SVD<method> drop-ins (rsvd_qr / rsvd_svd) at the dispatch edges, in
fp32, at tiny and thin shapes, and through leading dimensions and bases of their own -- the cases of
tests/dense_cases.py, whose `branch` column says what each row is there for.

a. test_dense_matches_reference: every row through Engine.qr / Engine.svd (device tensors, the
   storage dtype of the row) against the reference of dense_cases.reference on the exact values the
   GPU is given, with the assertions and bounds of the test_gpu_dense.py test of the same routine
   and dtype (`_BOUNDS` below names each source), and the shape of every output.
b. test_pitch_and_base_are_bit_identical: the rows of dense_cases.PITCH_CASES, first dense, then
   with A a view of leading dimension m + 1 or m + 3 whose base sits one element into its buffer,
   Q / R / U / V in _Padded buffers (ld = rows + 1 or + 3, offset base, guard columns) and S in a
   padded vector.  Required: bit identity with the dense run, every padding and guard element
   still holding its prefill pattern, A's buffer byte for byte unchanged.  Read from the code: no
   kernel of these paths chooses its arithmetic by a pitch or a base (rsvd_svd's panel product is
   panel_gemm_kernel, scalar stores; the MFMA GEMM of dense_big.cpp tiles by shape alone), and none
   was found by the runs: every row is held to bit identity.

Bounds that no earlier test of the routine and dtype sets (fp32: orthonormality, reconstruction, the
full-QR complement, which is checked through those two alone) are not taken from the GPU's output:
the reference's own spread was measured on the CPU -- the reference on A against the reference on A
moved by one ulp of the storage type (dense_cases.perturbed) -- and the bound is the larger of the
inherited one and four times that spread.  Measured spreads (relative Frobenius):
  fp64, every op: Q, R, S <= 5.2e-15, sign-aligned U, V <= 9.9e-14 (520 x 513)
  qr f32 20x17     Q 1.2e-7 R 8.5e-8 | qr f32 131x65   Q 1.1e-7 R 6.8e-8 | qr f32 517x513  Q 2.6e-7 R 1.2e-7
  qrfull f32 97x33 Q 1.0e-7 R 5.3e-8 | qrfull f32 33x97 Q 2.0e-7 R 2.0e-7
  jacobi f32 20x17 S 1.9e-8 U 8.2e-7 | 130x64 S 7.4e-9 U 5.4e-7 | 131x65 S 8.5e-9 U 5.4e-7
             65x131 S 8.9e-9 V 5.4e-7 | 520x513 S 3.7e-9 U 7.7e-6 (leading half 9.0e-7)
  pjacobi f32 65x65 S 1.1e-8 leading half 2.0e-5 | 17x20 S 2.7e-8 leading half 9.4e-7
Four times each stays below the inherited fp32 bounds (1e-5 on S and the QR factors, 1e-4 on the
leading half of U, V), so those hold unchanged; the fp32 bounds without an ancestor follow from them:
orthonormality of an fp32 Q 1e-5 (test_qr_f32_device), of fp32 U, V 1e-4 (the fp32 panels of
test_gpu_ragged.py); A = Q R in fp32 1e-5 and A = U S V^T in fp32 1e-4 (the factor bounds themselves:
a product of factors right to 1e-5 / 1e-4 is right to that order).

Every test prints its figures ("DENSE <case>: ...") before asserting.

Measured on an MI355X: the 74 tests of this file (51 rows, 23 pitch cases) take 4.3 s together, all
passing; the slowest is 0.4 s (the first, which loads the library), the 520 x 513 rows 0.1 s each.
Errors against the reference (relative Frobenius; orth: largest |Q^T Q - I| entry), worst per class:
  qr / qrfull f64, panel   Q 6.8e-15 (513x512)  R 2.4e-15  orth 1.6e-15  A=QR 9.8e-16
  qr / qrfull f64, big     Q 4.8e-15 (517x513)  R 2.5e-15  orth 1.8e-15  A=QR 1.1e-15
  qr / qrfull f32          Q 9.5e-8  R 3.8e-7 (517x513)  orth 5.0e-8  A=QR 3.8e-7
  jacobi f64, k <= 128     S 1.5e-14  U, V 1.5e-13 (203x97)  orth 2.2e-14  A=USV^T 1.0e-14
  jacobi f64, 520x512      S 8.7e-14  U, V 2.2e-12  orth 2.5e-13  A=USV^T 1.7e-13   (against LAPACK)
  jacobi f64, past 512     S 5.5e-14  U, V 2.3e-12  orth 2.2e-13  A=USV^T 1.1e-13
  jacobi f32               S 2.3e-8   leading half 1.9e-7 (20x17)  orth 1.4e-7  A=USV^T 1.7e-7
  pjacobi f64              S 3.3e-15  full U, V 5.1e-13 (65x65)  orth 1.3e-14
  pjacobi f32              S 2.3e-8   leading half 2.1e-7 (17x20)  orth 1.0e-7
  power                    S 7.1e-16  U 9.5e-16  V 1.3e-15; `kept` as asked in every row
  1x1, 7x1, 1x7: exact or within 5e-16.  Pitch and base: all 23 bit-identical, no padding touched.
No row missed a bound and no kernel was changed.

Checked that the tests bite, on scratch copies of the library, one run each:
  * panel_to_colmajor_kernel writing out[i + j * m]: 22 of the 23 pitch tests fail (every one but
    power-f64-600x513-r4, whose grid kernel writes U and V itself); test_gpu_dense.py stays green.
  * qr_big_typed writing its block back to Qo + c0 * m: the pitch tests of qr-f64-517x513,
    qr-f32-517x513 and qrfull-f64-513x40 fail (the three with a second block); test_gpu_dense.py
    stays green.
"""
import numpy as np
import pytest

import dense_cases as dc
from conftest import rel_fro, sign_align
from padded import _Padded

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _tdtype(c):
    torch = _torch()
    return torch.float64 if c.dtype == "f64" else torch.float32


def _orth_err(Q):
    return np.abs(Q.T @ Q - np.eye(Q.shape[1])).max()


def _dev_A(c, A, off=0, pad=0, fill=0.0):
    """A as a column-major device view with lda = m + pad whose base sits `off` elements into its
    buffer (off = pad = 0: dense, allocator-aligned).  Returns (view, buffer)."""
    torch = _torch()
    m, n = A.shape
    buf = torch.full((off + n * (m + pad),), fill, dtype=_tdtype(c))
    grid = buf[off:].view(n, m + pad)
    grid[:, :m] = torch.from_numpy(np.array(A.T, order="C")).to(_tdtype(c))  # (a copy: A is read-only)
    buf = buf.cuda()
    return buf[off:].view(n, m + pad)[:, :m].t(), buf


def _run(engine, c, A, out=None):
    if c.op in ("qr", "qrfull"):
        return engine.qr(A, full=c.op == "qrfull", out=out)
    return engine.svd(A, dc.METHOD[c.op], r=c.r, seed=dc.POWER_SEED, out=out)


# ---- the bounds ------------------------------------------------------------------------------------
def _qr_bounds(c):
    """(factors, orthonormality, A = Q R)"""
    if c.dtype == "f32":
        return 1e-5, 1e-5, 1e-5             # test_qr_f32_device; reconstruction: see the module docstring
    if c.branch["path"] == "big":
        return 1e-11, 1e-12, 1e-13          # test_qr_big_matches_givens
    return 1e-12, 1e-13, 1e-14              # test_qr_reduced_f64_matches_givens / test_qr_full_*


def _check_qr(c, Q, R):
    A = dc.inputs(c.id)
    Qo, Ro = dc.oracle_result(c.id)
    m, n, k = c.m, c.n, min(c.m, c.n)
    kq = m if c.op == "qrfull" else n
    tol, orth, recon = _qr_bounds(c)
    assert Q.shape == (m, kq) and R.shape == (kq, n)
    eq, er = rel_fro(Q[:, :k], Qo[:, :k]), rel_fro(R, Ro)
    eo, ea = _orth_err(Q), rel_fro(Q @ R, A)
    print(f"DENSE {c.id}: Q[:, :k] {eq:.2e} R {er:.2e} orth {eo:.2e} A=QR {ea:.2e}")
    assert np.isfinite(Q).all() and np.isfinite(R).all()
    assert np.all(np.tril(R, -1) == 0)
    assert np.all(np.diag(R)[: min(m - 1, n)] >= 0)  # the last pivot of a square A is never rotated
    assert er < tol and eq < tol, (er, eq)           # (a tall full Q's complement is any completion)
    assert eo < orth, eo
    assert ea < recon, ea
    if kq == m:  # a square Q: the reference's product of rotations has det +1
        assert np.linalg.slogdet(Q)[0] == 1.0
        if m <= n:
            assert rel_fro(Q, Qo) < tol


def _check_svd(c, U, S, V):
    A = dc.inputs(c.id)
    Uo, So, Vo = dc.oracle_result(c.id)
    m, n, k = c.m, c.n, min(c.m, c.n)
    big = c.branch["path"] in ("big", "grid") and c.op != "power"
    f32 = c.dtype == "f32"
    if c.op == "power":  # test_svd_power_matches_oracle / test_svd_power_large_n_grid
        kk = c.r or k
        assert S.shape == (kk,) and U.shape == (m, kk) and V.shape == (n, kk)  # `kept`
        good = S > 1e-3 * S[0]
        es = rel_fro(S[good], So[good])
        eu = rel_fro(sign_align(U[:, good], Uo[:, good]), Uo[:, good])
        ev = rel_fro(sign_align(V[:, good], Vo[:, good]), Vo[:, good])
        print(f"DENSE {c.id}: kept {S.shape[0]} good {int(good.sum())} S {es:.2e} U {eu:.2e} V {ev:.2e}")
        assert np.all(S > 0) and np.all(good == (So > 1e-3 * So[0]))
        assert es < 1e-10 and eu < 1e-8 and ev < 1e-8, (es, eu, ev)
        return
    assert U.shape == (m, k) and S.shape == (k,) and V.shape == (n, k)
    h = max(1, k // 2)
    es = rel_fro(S, So)
    eu, ev = rel_fro(sign_align(U, Uo), Uo), rel_fro(sign_align(V, Vo), Vo)
    euh = rel_fro(sign_align(U[:, :h], Uo[:, :h]), Uo[:, :h])
    evh = rel_fro(sign_align(V[:, :h], Vo[:, :h]), Vo[:, :h])
    ou, ov, ea = _orth_err(U), _orth_err(V), rel_fro((U * S) @ V.T, A)
    print(f"DENSE {c.id}: S {es:.2e} U {eu:.2e} V {ev:.2e} half U {euh:.2e} V {evh:.2e} "
          f"orthU {ou:.2e} orthV {ov:.2e} A=USV^T {ea:.2e}")
    assert np.isfinite(U).all() and np.isfinite(S).all() and np.isfinite(V).all()
    assert np.all(np.diff(S) <= 0)
    if f32:
        # test_svd_f32_device / test_svd_parallel_jacobi_f32_device / test_svd_big_parallel_jacobi_and_f32;
        # orthonormality and reconstruction: see the module docstring
        assert es < 1e-5, es
        assert euh < 1e-4 and evh < 1e-4, (euh, evh)
        assert ou < 1e-4 and ov < 1e-4, (ou, ov)
        assert ea < 1e-4, ea
    elif c.op == "pjacobi":  # test_svd_parallel_jacobi_matches_oracle
        assert es < 1e-10, es
        assert euh < 1e-4 and evh < 1e-4, (euh, evh)
        assert eu < 1e-6 and ev < 1e-6, (eu, ev)
        assert ou < 1e-12 and ov < 1e-12, (ou, ov)
    else:  # test_svd_jacobi_f64_matches_oracle; past 512: test_svd_jacobi_big_f64
        assert es < 1e-12, es
        assert eu < (1e-9 if big else 1e-10) and ev < (1e-9 if big else 1e-10), (eu, ev)
        assert ou < 1e-12 and ov < 1e-12, (ou, ov)
        assert ea < 1e-12, ea


# ---- a. parity of every row ------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in dc.CASES])
def test_dense_matches_reference(engine, cid):
    c = dc.BY_ID[cid]
    A, _ = _dev_A(c, dc.inputs(cid))
    res = _run(engine, c, A)
    assert all(x.dtype == _tdtype(c) for x in res)
    res = [x.cpu().double().numpy() for x in res]
    (_check_qr if c.op in ("qr", "qrfull") else _check_svd)(c, *res)


# ---- b. pitch and base -----------------------------------------------------------------------------
@pytest.mark.parametrize("cid,pads", dc.PITCH_CASES, ids=[p[0] for p in dc.PITCH_CASES])
def test_pitch_and_base_are_bit_identical(engine, cid, pads):
    from rsvd_kamaneh_raganato_terrana_amd.api import colmajor

    torch = _torch()
    c = dc.BY_ID[cid]
    m, n, k = c.m, c.n, min(c.m, c.n)
    da, d1, d2 = pads
    dt = _tdtype(c)
    A0, _ = _dev_A(c, dc.inputs(cid))
    dense = _run(engine, c, A0)
    A1, abuf = _dev_A(c, dc.inputs(cid), off=1, pad=da, fill=-7.25)
    before = abuf.clone()
    kept, lda = colmajor(A1)
    assert kept.data_ptr() == A1.data_ptr() == abuf.data_ptr() + abuf.element_size()  # the view itself goes in
    assert lda == (m + da if n > 1 else lda) and torch.equal(A1, A0)
    if c.op in ("qr", "qrfull"):
        kq = m if c.op == "qrfull" else n
        bufs = [_Padded(m, kq, m + d1, dt), _Padded(kq, n, kq + d2, dt)]
        out = tuple(b.mat for b in bufs)
    else:
        bufs = [_Padded(m, k, m + d1, dt), _Padded(k, 1, k + 1, dt), _Padded(n, k, n + d2, dt)]
        out = (bufs[0].mat, bufs[1].mat[:, 0], bufs[2].mat)
    got = _run(engine, c, A1, out=out)
    torch.cuda.synchronize()
    assert all(torch.isfinite(x).all() for x in dense)
    same = [bool(torch.equal(g, d)) for g, d in zip(got, dense)]
    worst = [float((g.double() - d.double()).abs().max()) if g.numel() else 0.0 for g, d in zip(got, dense)]
    clean = [b.padding_untouched() for b in bufs]
    a_same = bool(torch.equal(abuf, before))
    print(f"DENSE pitch {cid} pads {pads}: identical {same} max |diff| {worst} padding untouched {clean} "
          f"A unchanged {a_same}")
    assert all(g.shape == d.shape for g, d in zip(got, dense))
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))  # written in place
    assert all(same), (same, worst)
    assert all(clean), clean
    assert a_same
