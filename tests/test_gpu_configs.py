"""GPU parity at the BASELINE.json configurations' own kernel instantiations, and the C ABI's
error surfacing (rsvd_sync) and a_scale contract.

* C2 (configs[1]) at its full size: dense 4096 x 4096 fp32, l = 64, q = 2.
* C5's kernels (configs[4]): e4m3 A with m and lda multiples of 16 (the LDS-DMA v2 kernels,
  wide.cpp WideLayout) at l = 256 and l = 512, q = 2, and bf16 A at l = 512.
Each compares with the fp64 oracle (oracle/, test infrastructure) on the exact values the GPU sees
(bf16 / e4m3 A dequantised, the engine's own bf16 / e4m3-rounded Omega).
Tolerance: north_star's 1e-4 relative Frobenius on S and on the sign-aligned leading half of U, V
(fp32 outputs), plus U / V orthonormality and the reconstruction error against the oracle's.
"""
import numpy as np
import pytest

import oracle
from conftest import gapped_matrix, rel_fro, sign_align

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _dev_colmajor(A_np, dtype):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(A_np.T)).cuda().to(dtype).t()


def _check(U, S, V, Uo, So, Vo, A, tol, orth_tol):
    l = So.shape[0]
    k = l // 2
    assert rel_fro(S, So) < tol, rel_fro(S, So)
    eu = rel_fro(sign_align(U[:, :k], Uo[:, :k]), Uo[:, :k])
    ev = rel_fro(sign_align(V[:, :k], Vo[:, :k]), Vo[:, :k])
    assert eu < tol and ev < tol, (eu, ev)
    assert np.linalg.norm(U.T @ U - np.eye(l)) < orth_tol
    assert np.linalg.norm(V.T @ V - np.eye(l)) < orth_tol
    e = np.linalg.norm(A - (U * S) @ V.T)
    eo = np.linalg.norm(A - (Uo * So) @ Vo.T)
    assert abs(e - eo) <= 10 * tol * np.linalg.norm(A), (e, eo)


def test_c2_full_size_f32(engine):
    """BASELINE configs[1]: 4096 x 4096 fp32, rank 64, q = 2 (the narrow engine's C2 kernels)."""
    torch = _torch()
    m = n = 4096
    l = 64
    A = gapped_matrix(m, n, 128, decay=0.9, seed=2).astype(np.float32)
    Om = oracle.generate_omega(n, l, 0x5EED0002)
    Uo, So, Vo = oracle.rsvd(A.astype(np.float64), l, q=2, Omega=Om)
    U, S, V = engine.rsvd(_dev_colmajor(A, torch.float32), l, q=2, omega=torch.from_numpy(Om.astype(np.float32)))
    U, S, V = (x.cpu().double().numpy() for x in (U, S, V))
    _check(U, S, V, Uo, So, Vo, A.astype(np.float64), 1e-4, 1e-3)


@pytest.mark.parametrize("m,n,l", [(4096, 2048, 256), (4096, 2048, 512)])
def test_fp8_v2_kernels_match_oracle(engine, m, n, l):
    """e4m3 A with m, lda multiples of 16: wproj2_kernel<true, *, LP, *> (the C5 instantiations
    at l = 512), gram_sym at LP = 512, the fp32-exit block Jacobi at LP = 512."""
    torch = _torch()
    A32 = gapped_matrix(m, n, 2 * l, decay=0.985, seed=l).astype(np.float32)
    scale = float(np.abs(A32).max()) / 448.0
    A8 = _dev_colmajor(A32 / scale, torch.float8_e4m3fn)
    assert A8.stride(1) % 16 == 0 and m % 16 == 0
    A_exact = A8.float().cpu().double().numpy() * scale
    Om = engine.generate_omega(n, l, seed=321, dtype=torch.float8_e4m3fn).cpu().double().numpy()
    Uo, So, Vo = oracle.rsvd(A_exact, l, q=2, Omega=Om)
    U, S, V = engine.rsvd(A8, l, q=2, seed=321, a_scale=scale)
    U, S, V = (x.cpu().double().numpy() for x in (U, S, V))
    _check(U, S, V, Uo, So, Vo, A_exact, 1e-4, 1e-3)


def test_bf16_l512_matches_oracle(engine):
    torch = _torch()
    m, n, l = 4096, 2048, 512
    A32 = gapped_matrix(m, n, 2 * l, decay=0.985, seed=17).astype(np.float32) * 4
    Ad = _dev_colmajor(A32, torch.bfloat16)
    A_exact = Ad.float().cpu().double().numpy()
    Om = engine.generate_omega(n, l, seed=99, dtype=torch.bfloat16).cpu().double().numpy()
    Uo, So, Vo = oracle.rsvd(A_exact, l, q=2, Omega=Om)
    U, S, V = engine.rsvd(Ad, l, q=2, seed=99)
    U, S, V = (x.cpu().double().numpy() for x in (U, S, V))
    _check(U, S, V, Uo, So, Vo, A_exact, 1e-4, 1e-3)


@pytest.mark.parametrize("dt,l", [("f32", 32), ("f64", 32), ("bf16", 128)])
def test_a_scale_contract(engine, dt, l):
    """A = a_scale * (stored A) for every dtype: S scales by |a_scale|, V flips with its sign
    (include/rsvd_c.h rsvd_desc_t.a_scale), identically on the narrow and the wide engine."""
    torch = _torch()
    tdt = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}[dt]
    A = _dev_colmajor(gapped_matrix(600, 400, 2 * l, decay=0.9, seed=3).astype(np.float32), tdt)
    U1, S1, V1 = engine.rsvd(A, l, q=1, seed=5)
    U2, S2, V2 = engine.rsvd(A, l, q=1, seed=5, a_scale=-2.5)
    torch.testing.assert_close(S2, 2.5 * S1, rtol=1e-6, atol=0)
    torch.testing.assert_close(U2, U1, rtol=0, atol=0)
    torch.testing.assert_close(V2, -V1, rtol=0, atol=0)


def test_non_finite_input_raises(engine):
    """A NaN in A cannot come back as RSVD_OK: rsvd_sync reports RSVD_ERR_NUMERICAL."""
    torch = _torch()
    from rsvd_kamaneh_raganato_terrana_amd._capi import RSVDError

    A = gapped_matrix(300, 200, 40, seed=1).astype(np.float32)
    A[17, 5] = np.nan
    with pytest.raises(RSVDError, match="numerical"):
        engine.rsvd(_dev_colmajor(A, torch.float32), 16, q=1, seed=2)
    # the sticky error was reported and cleared: the next good run succeeds
    U, S, V = engine.rsvd(_dev_colmajor(np.nan_to_num(A), torch.float32), 16, q=1, seed=2)
    assert torch.isfinite(S).all()


def test_host_entry_point_reports_non_finite(engine):
    from rsvd_kamaneh_raganato_terrana_amd._capi import RSVDError

    A = gapped_matrix(200, 150, 30, seed=4)
    A[3, 3] = np.inf
    with pytest.raises(RSVDError, match="numerical"):
        engine.rsvd_host(A, 8, q=1)


def test_lowp_intermediates_flag(engine):
    """RSVD_FLAG_LOWP_INTERMEDIATES (include/rsvd_c.h): power iteration 1 of q = 2 on the bf16
    operand alone.  On a spectrum that decays across the sketch (0.985^i, l = 256) the error it
    injects is damped by the last iteration: the result stays within the 1e-4 bar of the oracle
    and within 1e-4 of the full-precision path (DESIGN.md §3.2 has the flat-spectrum limit)."""
    torch = _torch()
    m, n, l = 4096, 2048, 256
    A32 = gapped_matrix(m, n, 2 * l, decay=0.985, seed=17).astype(np.float32) * 4
    Ad = _dev_colmajor(A32, torch.bfloat16)
    A_exact = Ad.float().cpu().double().numpy()
    Om = engine.generate_omega(n, l, seed=99, dtype=torch.bfloat16).cpu().double().numpy()
    Uo, So, Vo = oracle.rsvd(A_exact, l, q=2, Omega=Om)
    U, S, V = engine.rsvd(Ad, l, q=2, seed=99, lowp_intermediates=True)
    U, S, V = (x.cpu().double().numpy() for x in (U, S, V))
    _check(U, S, V, Uo, So, Vo, A_exact, 1e-4, 1e-3)
    U2, S2, V2 = engine.rsvd(Ad, l, q=2, seed=99)
    assert rel_fro(S, S2.cpu().double().numpy()) < 1e-4


@pytest.mark.parametrize("decay,l", [(0.995, 128), (0.9, 128), (0.97, 256), (0.985, 512)])
def test_split_gram_paths(engine, decay, l):
    """The split Gram (wide_gram.hip gram_split_kernel, bf16 / e4m3 A): its factor is kept while every
    pivot stays above kSplitIllTol of its diagonal (0.995^i: cond(Y) ~ 2 at l = 128), and the fp64
    Gram + factor re-run (predicated) past it (0.9^i over 2 l columns: sigma_l / sigma_1 ~ 1e-6;
    0.97^i at l = 256; 0.985^i at l = 512) -- both must meet the 1e-4 bar against the oracle."""
    torch = _torch()
    m, n = 4096, 2048
    A32 = gapped_matrix(m, n, 2 * l, decay=decay, seed=l + 7).astype(np.float32) * 4
    Ad = _dev_colmajor(A32, torch.bfloat16)
    A_exact = Ad.float().cpu().double().numpy()
    Om = engine.generate_omega(n, l, seed=5, dtype=torch.bfloat16).cpu().double().numpy()
    Uo, So, Vo = oracle.rsvd(A_exact, l, q=2, Omega=Om)
    U, S, V = engine.rsvd(Ad, l, q=2, seed=5)
    U, S, V = (x.cpu().double().numpy() for x in (U, S, V))
    _check(U, S, V, Uo, So, Vo, A_exact, 1e-4, 1e-3)


@pytest.mark.parametrize("n,l", [(131072, 512), (393216, 256)])
def test_split_cross_gram_long_n(engine, n, l):
    """R = Q_B^T B^T on the split bf16 MFMA accumulates each row chunk in fp32; past 4096
    rows per chunk (n > 65536 at LP = 512, n > 262144 at LP = 256) the engine takes the fp64 cross
    Gram instead (launch_gram_split_cross).  bf16 A, 640 x n, rank-400 0.985^i spectrum: the leading
    l/2 singular values against the exact SVD of the bf16 A (fp64 eigenvalues of A A^T, 640 x 640),
    1e-4 relative Frobenius, and V orthonormal."""
    import torch

    m = 640
    g = torch.Generator(device="cuda").manual_seed(n + l)
    X = torch.linalg.qr(torch.randn(m, 400, generator=g, device="cuda", dtype=torch.float64))[0]
    Y = torch.linalg.qr(torch.randn(n, 400, generator=g, device="cuda", dtype=torch.float64))[0]
    sig = 0.985 ** torch.arange(400, device="cuda", dtype=torch.float64)
    Ab = ((X * sig) @ Y.t()).to(torch.bfloat16)
    Ad = Ab.t().contiguous().t()
    A64 = Ab.double()
    lam = torch.linalg.eigvalsh(A64 @ A64.t()).flip(0).clamp_min(0).sqrt().cpu().numpy()
    del X, Y, A64
    U, S, V = engine.rsvd(Ad, l, q=1, seed=9)
    torch.cuda.synchronize()
    k = l // 2
    S = S.double().cpu().numpy()
    assert rel_fro(S[:k], lam[:k]) < 1e-4, rel_fro(S[:k], lam[:k])
    Vd = V.double()
    assert torch.linalg.norm(Vd.t() @ Vd - torch.eye(l, dtype=torch.float64, device="cuda")).item() < 1e-3
