"""GPU: every engine at extreme magnitudes of A (the cases of tests/scale_cases.py).

The contract (include/rsvd_c.h, "dynamic range"): scaling A by 2^k -- or passing a_scale = 2^k --
scales S by 2^k and leaves U, V and the range finder's Q unchanged, for |k| <= 40 where results are
delivered in fp32 (fp32, bf16, e4m3 A) and |k| <= 240 for fp64 A; outside the window a run either
still meets the bars or ends in RSVD_ERR_NUMERICAL, never in RSVD_OK with wrong numbers.

Expected values: the fp64 oracle at k = 0 (bit-for-bit equivariant, tests/test_scale_cases.py), S
scaled by ldexp.  Bars: the project's own for the dtype and LP -- test_gpu_ragged._bounds for the
rSVD, test_gpu_batched._parity's for the batched kernel, test_gpu_compress's for C and err.  Per
case and k: S finite, positive and descending; ldexp(S, -k) against the oracle's S; the sign-aligned
leading half of U and V; orthonormality; the reconstruction error against the oracle's; and the path
taken (cholqr_fallbacks and the K splits of rsvd_get_info, info[b, 1] of the batched calls) equal to
the k = 0 run's.  Whether U and V are bit-identical to the k = 0 run is printed, not asserted.
Every test prints its figures ("SCALE <case> k=...") before asserting.

Found with it: the rotation test of the one-workgroup Jacobi (csrc/jacobi.hip, and its copy in
csrc/batched.hip) compared fourth powers of the singular values in the compute type, so in fp32 no
pair rotated outside sigma in about [1e-9, 4e9] and the run returned RSVD_OK with S, U, V of an
unconverged W; both kernels now hold W divided by the power of two above its largest entry.

Measured on an MI355X: see DESIGN.md, "Dynamic range".
"""
import numpy as np
import pytest

import scale_cases as sc
from test_gpu_ragged import _bounds, _dev_A, _dev_omega

pytestmark = pytest.mark.gpu

PATH_KEYS = ("cholqr_fallbacks", "splits_nn", "splits_tn")


def _torch():
    import torch

    return torch


def _np(*ts):
    return tuple(t.cpu().double().numpy() for t in ts)


# ---- the rSVD rows -----------------------------------------------------------------------------------
_BASE = {}


def _run(engine, cid, k):
    c = sc.BY_ID[cid]
    stored, a_scale = sc.scaled_inputs(cid, k)
    _, _, _, Om = sc.inputs(cid)
    U, S, V = engine.rsvd(_dev_A(stored), c.l, q=c.q, omega=_dev_omega(Om, c), a_scale=a_scale)
    info = engine.info()
    return U.cpu(), S.cpu(), V.cpu(), {key: info[key] for key in PATH_KEYS}


def _base(engine, cid):
    """The k = 0 run of the case on this engine: once, shared by every k."""
    if cid not in _BASE:
        _BASE[cid] = _run(engine, cid, 0)
    return _BASE[cid]


@pytest.mark.parametrize("cid,k", [(c.id, k) for c in sc.CASES for k in c.ks],
                         ids=[f"{c.id}{k:+d}" for c in sc.CASES for k in c.ks])
def test_rsvd_is_equivariant(engine, cid, k):
    torch = _torch()
    c = sc.BY_ID[cid]
    U0, S0, V0, path0 = _base(engine, cid)
    U, S, V, path = _run(engine, cid, k)
    same = torch.equal(U, U0) and torch.equal(V, V0)
    same_s = torch.equal(S.double(), torch.ldexp(S0.double(), torch.tensor(k)))
    print(f"SCALE {cid} k={k:+d} [{c.path}]: U, V bit-identical to k = 0: {same}; S exactly 2^k S_0: {same_s}; "
          f"path {path} (k = 0: {path0})")
    sc.check(cid, k, *_np(U, S, V), _bounds(c))
    assert path == path0, (cid, k, path, path0)


@pytest.mark.parametrize("cid", sorted({c.id for c in sc.CASES}))
def test_rsvd_base_run_meets_the_bars(engine, cid):
    """The k = 0 run the others are compared with is itself inside the bars."""
    U0, S0, V0, _ = _base(engine, cid)
    sc.check(cid, 0, *_np(U0, S0, V0), _bounds(sc.BY_ID[cid]))


# ---- the range finder's Q ----------------------------------------------------------------------------
@pytest.mark.parametrize("cid,q", sc.RF_CASES, ids=[f"{cid}-q{q}" for cid, q in sc.RF_CASES])
def test_range_finder_is_equivariant(engine, cid, q):
    """Q_k is orthonormal at the project's bar and spans what the oracle's Q spans:
    ||Q_o - Q_k Q_k^T Q_o||_F / ||Q_o||_F below the bar of the vectors."""
    import oracle

    torch = _torch()
    c = sc.BY_ID[cid]
    _, tol_uv, orth = _bounds(c)
    stored, _, A, Om = sc.inputs(cid)
    Qo = oracle.intermediate_step(A, Om, q=q)
    Q0 = engine.range_finder(_dev_A(stored), _dev_omega(Om, c), q=q).cpu()
    for k in (0, 40, -40):
        Qk = engine.range_finder(_dev_A(sc.scale_stored(stored, k)), _dev_omega(Om, c), q=q).cpu()
        Q = Qk.double().numpy()
        on = np.linalg.norm(Q.T @ Q - np.eye(c.l))
        span = np.linalg.norm(Qo - Q @ (Q.T @ Qo)) / np.linalg.norm(Qo)
        print(f"SCALE rf {cid} q={q} k={k:+d}: orth {on:.2e} span {span:.2e} bit-identical to k = 0: "
              f"{torch.equal(Qk, Q0)}")
        assert np.isfinite(Q).all()
        assert on < orth and span < tol_uv, (cid, q, k, on, span)


# ---- out of the window: the bars or RSVD_ERR_NUMERICAL -------------------------------------------------
@pytest.mark.parametrize("k", sc.OUT_OF_RANGE_KS)
def test_rsvd_out_of_range_is_reported(engine, k):
    import rsvd_kamaneh_raganato_terrana_amd as R

    cid = "n32a"
    c = sc.BY_ID[cid]
    try:
        U, S, V, _ = _run(engine, cid, k)
    except R.RSVDError as e:
        print(f"SCALE {cid} k={k:+d}: RSVDError status {e.status}")
        assert e.status == 5  # RSVD_ERR_NUMERICAL
    else:
        sc.check(cid, k, *_np(U, S, V), _bounds(c))
    U, S, V, _ = _run(engine, cid, 0)  # the handle is usable and correct afterwards
    sc.check(cid, 0, *_np(U, S, V), _bounds(c), what=f"{cid} after k={k:+d}")


# ---- the fused batched kernel and its compress tail -------------------------------------------------------
def _tdt(t):
    torch = _torch()
    return torch.float32 if t == "f32" else torch.float64


def _dev_batch(mats, t):
    x = _torch().from_numpy(np.stack(mats)).to(_tdt(t)).cuda()
    return x.transpose(1, 2).contiguous().transpose(1, 2)


def _batch(t, ks):
    m, n, l, q = sc.BATCH_SHAPE
    mats = [np.ldexp(np.array(sc.batch_matrix(t, b)), k) for b, k in enumerate(ks)]
    om = _torch().from_numpy(np.stack([sc.batch_omega(t, b) for b in range(len(ks))])).to(_tdt(t))
    return mats, om


def _batch_parity(tag, t, b, k, U, S, V):
    """test_gpu_batched._parity's bars on the run of matrix b at 2^k, S first brought back by ldexp."""
    from conftest import rel_fro, sign_align

    l = sc.BATCH_SHAPE[2]
    Uo, So, Vo = sc.batch_oracle(t, b)
    tol_s, tol_v, tol_o = (1e-4, 1e-4, 1e-4) if t == "f32" else (1e-10, 1e-8, 1e-10)
    h = l // 2
    S1 = np.ldexp(S, -k)
    es = rel_fro(S1, So)
    eu = rel_fro(sign_align(U[:, :h], Uo[:, :h]), Uo[:, :h])
    ev = rel_fro(sign_align(V[:, :h], Vo[:, :h]), Vo[:, :h])
    ou = np.linalg.norm(U.T @ U - np.eye(l))
    ov = np.linalg.norm(V.T @ V - np.eye(l))
    print(f"SCALE {tag} b{b} k={k:+d}: S {es:.2e} U {eu:.2e} V {ev:.2e} orthU {ou:.2e} orthV {ov:.2e} "
          f"S[0] {S[0]:.3e} S[-1] {S[-1]:.3e}")
    assert np.isfinite(S).all() and np.all(S > 0) and np.all(np.diff(S) <= 0), (tag, b, S)
    assert es < tol_s and eu < tol_v and ev < tol_v and ou < tol_o and ov < tol_o, (tag, b, es, eu, ev, ou, ov)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_batched_is_equivariant(engine, t):
    """bat32 / bat64: four matrices scaled by 2^(0, +40, -40, +20) (fp64: 0, +240, -240, +40) in ONE launch."""
    torch = _torch()
    m, n, l, q = sc.BATCH_SHAPE
    ks = sc.BATCH_KS[t]
    assert engine.batched_is_fused(m, n, l, _tdt(t), q=q, batch=len(ks)) == 1
    mats0, om = _batch(t, (0,) * len(ks))
    U0, S0, V0, info0 = engine.rsvd_batched(_dev_batch(mats0, t), l, q=q, omega=om, return_info=True)
    mats, _ = _batch(t, ks)
    U, S, V, info = engine.rsvd_batched(_dev_batch(mats, t), l, q=q, omega=om, return_info=True)
    print(f"SCALE bat{t[1:]}: info {info.cpu().tolist()} (k = 0: {info0.cpu().tolist()})")
    Un, Sn, Vn = _np(U, S, V)
    for b, k in enumerate(ks):
        same = torch.equal(U[b], U0[b]) and torch.equal(V[b], V0[b])
        print(f"SCALE bat{t[1:]} b{b} k={k:+d}: U, V bit-identical to k = 0: {same}")
        _batch_parity(f"bat{t[1:]}", t, b, k, Un[b], Sn[b], Vn[b])
    assert torch.equal(info[:, 1], info0[:, 1])


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_compress_is_equivariant(engine, t):
    """cmp32 / cmp64: C_b scales by 2^k, err2[2b] by exactly 2^(2k) (an fp64 sum of exactly widened
    squares in a fixed order: an identity, not a tolerance), err2[2b + 1] agrees with
    ||A_b - C_b||_F^2 recomputed on the host from the returned C at test_gpu_compress's 1e-10."""
    from conftest import rel_fro

    torch = _torch()
    m, n, l, q = sc.BATCH_SHAPE
    r = sc.BATCH_RANK
    ks = sc.BATCH_KS[t]
    tol_p = 1e-4 if t == "f32" else 1e-8
    mats0, om = _batch(t, (0,) * len(ks))
    C0, err0, info0 = engine.compress_batched(_dev_batch(mats0, t), l, k=r, q=q, omega=om, return_info=True)
    mats, _ = _batch(t, ks)
    C, err, info = engine.compress_batched(_dev_batch(mats, t), l, k=r, q=q, omega=om, return_info=True)
    Cn, errn, err0n = C.cpu().double().numpy(), err.cpu().numpy(), err0.cpu().numpy()
    for b, k in enumerate(ks):
        Uo, So, Vo = sc.batch_oracle(t, b)
        Co = (Uo[:, :r] * So[:r]) @ Vo[:, :r].T
        ep = rel_fro(np.ldexp(Cn[b], -k), Co)
        e2 = float(np.sum((mats[b] - Cn[b]) ** 2))
        exact = errn[b, 0] == np.ldexp(err0n[b, 0], 2 * k)
        print(f"SCALE cmp{t[1:]} b{b} k={k:+d}: parity {ep:.2e} err {errn[b, 0]:.17e} {errn[b, 1]:.17e} "
              f"2^(2k) err_0 {np.ldexp(err0n[b, 0], 2 * k):.17e} host {e2:.17e}; C bit-identical up to 2^k: "
              f"{np.array_equal(np.ldexp(Cn[b], -k), C0[b].cpu().double().numpy())}")
        assert np.isfinite(Cn[b]).all() and ep < tol_p, (b, k, ep)
        assert exact, (b, k, errn[b, 0], np.ldexp(err0n[b, 0], 2 * k))
        assert abs(errn[b, 1] - e2) <= 1e-10 * e2, (b, k, errn[b, 1], e2)
    assert torch.equal(info[:, 1], info0[:, 1])


def test_batched_out_of_range_is_reported(engine):
    """bat32 with matrices 1 and 2 at 2^(+100, -100): each of them either meets the bars or is marked in
    info (bit 1) and the call ends in RSVD_ERR_NUMERICAL; their neighbours are correct; the next
    ordinary run on the handle is correct (as test_gpu_batched.test_nan_in_one_matrix)."""
    import rsvd_kamaneh_raganato_terrana_amd as R

    t = "f32"
    m, n, l, q = sc.BATCH_SHAPE
    ks = sc.BATCH_OUT_KS
    mats, om = _batch(t, ks)
    U, S, V, info = engine.rsvd_batched(_dev_batch(mats, t), l, q=q, omega=om, return_info=True, check_errors=False)
    status = 0
    try:
        engine.sync()
    except R.RSVDError as e:
        status = e.status
    info = info.cpu().numpy()
    print(f"SCALE bat32 out of range: status {status} info {info.tolist()}")
    flagged = [bool(info[b, 1] & 2) for b in range(len(ks))]
    assert status == (5 if any(flagged) else 0)
    assert not flagged[0] and not flagged[3]
    Un, Sn, Vn = _np(U, S, V)
    for b, k in enumerate(ks):
        if not flagged[b]:
            _batch_parity("bat32 out of range", t, b, k, Un[b], Sn[b], Vn[b])
    mats0, _ = _batch(t, (0,) * len(ks))
    Un, Sn, Vn = _np(*engine.rsvd_batched(_dev_batch(mats0, t), l, q=q, omega=om))
    for b in range(len(ks)):
        _batch_parity("bat32 after out of range", t, b, 0, Un[b], Sn[b], Vn[b])


# ---- the dense drop-ins: rsvd_qr, rsvd_svd (Jacobi) ------------------------------------------------------
def _dev_dense(A, f32):
    torch = _torch()
    t = torch.from_numpy(np.array(A.T, order="C")).to(torch.float32 if f32 else torch.float64).cuda()
    return t.t()  # column-major


@pytest.mark.parametrize("full", [False, True], ids=["reduced", "full"])
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_qr_is_equivariant(engine, t, full):
    """qr32 / qr64: Q unchanged, R scaled by 2^k, at test_gpu_dense.py's bars (fp64 1e-12 on the factors,
    1e-13 on orthonormality, 1e-14 on A = Q R; fp32 1e-5) against the oracle's Givens QR at k = 0."""
    from conftest import rel_fro

    torch = _torch()
    f32 = t == "f32"
    tol_f, tol_o, tol_r = (1e-5, 1e-5, 1e-5) if f32 else (1e-12, 1e-13, 1e-14)
    A = sc.dense_matrix("qr", f32)
    n = A.shape[1]
    Qo, Ro = sc.dense_qr_oracle(full, f32)
    Q0, R0 = engine.qr(_dev_dense(A, f32), full=full)
    for k in (0,) + sc.DENSE_KS[t]:
        Qk, Rk = engine.qr(_dev_dense(np.ldexp(A, k), f32), full=full)
        Q, R = _np(Qk, Rk)
        R1 = np.ldexp(R, -k)
        eq, er = rel_fro(Q[:, :n], Qo[:, :n]), rel_fro(R1, Ro)
        on = np.abs(Q.T @ Q - np.eye(Q.shape[1])).max()
        rec = rel_fro(Q @ R1, A)
        print(f"SCALE qr{t[1:]} {'full' if full else 'reduced'} k={k:+d}: Q {eq:.2e} R {er:.2e} orth {on:.2e} "
              f"A=QR {rec:.2e}; Q bit-identical to k = 0: {torch.equal(Qk, Q0)}")
        assert np.isfinite(Q).all() and np.isfinite(R).all()
        assert eq < tol_f and er < tol_f and on < tol_o and rec < tol_r, (t, full, k, eq, er, on, rec)
        assert np.all(np.tril(R, -1) == 0)


@pytest.mark.parametrize("name", ["sv_small", "sv_big"])
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_svd_jacobi_is_equivariant(engine, t, name):
    """sv32 / sv64: SVD<Jacobi> of 120 x 60 (one-workgroup Jacobi, k <= 64) and 300 x 130 (block Jacobi) at
    test_gpu_dense.py's bars: fp64 S 1e-12, U and V 1e-10, orthonormality 1e-12, A = U S V^T 1e-13 / 1e-12;
    fp32 S 1e-5, the leading half of U and V 1e-4, orthonormality and A = U S V^T at the fp32 QR bar 1e-5
    (test_gpu_dense.py has no fp32 SVD bar for them)."""
    from conftest import rel_fro, sign_align

    torch = _torch()
    f32 = t == "f32"
    A = sc.dense_matrix(name, f32)
    d = min(A.shape)
    Uo, So, Vo, _ = sc.dense_svd_oracle(name, f32)
    U0, S0, V0 = engine.svd(_dev_dense(A, f32), 0)
    for k in (0,) + sc.DENSE_KS[t]:
        Uk, Sk, Vk = engine.svd(_dev_dense(np.ldexp(A, k), f32), 0)
        U, S, V = _np(Uk, Sk, Vk)
        S1 = np.ldexp(S, -k)
        h = d // 2 if f32 else d
        es = rel_fro(S1, So)
        eu = rel_fro(sign_align(U[:, :h], Uo[:, :h]), Uo[:, :h])
        ev = rel_fro(sign_align(V[:, :h], Vo[:, :h]), Vo[:, :h])
        on = max(np.abs(U.T @ U - np.eye(d)).max(), np.abs(V.T @ V - np.eye(d)).max())
        rec = rel_fro((U * S1) @ V.T, A)
        print(f"SCALE sv{t[1:]} {name} k={k:+d}: S {es:.2e} U {eu:.2e} V {ev:.2e} orth {on:.2e} A=USV^T {rec:.2e}; "
              f"U, V bit-identical to k = 0: {torch.equal(Uk, U0) and torch.equal(Vk, V0)}")
        assert np.isfinite(S).all() and np.all(S > 0) and np.all(np.diff(S) <= 0), (t, name, k)
        if f32:
            assert es < 1e-5 and eu < 1e-4 and ev < 1e-4, (t, name, k, es, eu, ev)
            assert on < 1e-5 and rec < 1e-5, (t, name, k, on, rec)  # test_qr_f32_device's bar
        else:
            assert es < 1e-12 and eu < 1e-10 and ev < 1e-10 and on < 1e-12, (t, name, k, es, eu, ev, on)
            assert rec < (1e-13 if d <= 64 else 1e-12), (t, name, k, rec)


# ---- lowrank with A and the error words -------------------------------------------------------------------
@pytest.mark.parametrize("k", [40, -40])
def test_lowrank_is_equivariant(engine, k):
    """lr: C = U_8 diag(2^k S_8) V_8^T against 2^k A, fp32, 130 x 70: C against the host product at
    test_gpu_lowrank.py's 1e-5, err[0] = 2^(2k) err_0[0] exactly (an fp64 sum of exactly widened squares in a
    fixed order), err[0] and err[1] against the host's sum over
    the returned C at its 1e-10."""
    import oracle
    from conftest import gapped_matrix, rel_fro

    torch = _torch()
    m, n, r = 130, 70, 8
    A = np.array(gapped_matrix(m, n, 24, decay=0.85, seed=1307)).astype(np.float32).astype(np.float64)
    Uo, So, Vo = oracle.rsvd(A, r, q=2, seed=5)
    f = lambda X: torch.from_numpy(np.array(X.T, order="C")).to(torch.float32).cuda().t()
    Uh, Sh, Vh = (X.astype(np.float32).astype(np.float64) for X in (Uo, So, Vo))
    U, V = f(Uh), f(Vh)
    S0 = torch.from_numpy(Sh).to(torch.float32).cuda()
    C0, err0 = engine.lowrank(U, S0, V, k=r, A=f(A))
    Sk = torch.from_numpy(np.ldexp(Sh, k)).to(torch.float32).cuda()
    Ak = np.ldexp(A, k)
    C, err = engine.lowrank(U, Sk, V, k=r, A=f(Ak))
    torch.cuda.synchronize()
    engine.sync()
    Ch, e, e0 = C.cpu().double().numpy(), err.cpu().numpy(), err0.cpu().numpy()
    ec = rel_fro(np.ldexp(Ch, -k), (Uh * Sh) @ Vh.T)
    a2, e2 = float(np.sum(Ak * Ak)), float(np.sum((Ak - Ch) ** 2))
    print(f"SCALE lr k={k:+d}: C {ec:.2e} err {e[0]:.17e} {e[1]:.17e} 2^(2k) err_0 {np.ldexp(e0[0], 2 * k):.17e} "
          f"{np.ldexp(e0[1], 2 * k):.17e} host {a2:.17e} {e2:.17e}; err[0] exactly 2^(2k) err_0[0]: "
          f"{e[0] == np.ldexp(e0[0], 2 * k)}; C bit-identical up to 2^k: "
          f"{np.array_equal(np.ldexp(Ch, -k), C0.cpu().double().numpy())}")
    assert np.isfinite(Ch).all() and ec < 1e-5, ec
    assert e[0] == np.ldexp(e0[0], 2 * k), (e[0], np.ldexp(e0[0], 2 * k))  # an identity, as in the compress tail
    assert abs(e[0] - a2) <= 1e-10 * a2 and abs(e[1] - e2) <= 1e-10 * e2, (e, a2, e2)


# ---- POD ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xh", [False, True], ids=["noXh", "Xh"])
@pytest.mark.parametrize("svd_type", [1, 4])
@pytest.mark.parametrize("t", ["f64", "f32"])
def test_pod_is_equivariant(engine, t, svd_type, xh):
    """pod64 / pod32: snapshots scaled by 2^+-40 scale C and sigma by 2^+-80 and, under the default flag,
    W = S V / sigma by 2^-+40; N is unchanged.  The reference, the inputs and the bars are test_gpu_pod.py's
    (sigma and W 1e-8 in fp64, 1e-4 in fp32), at nh = 300, ns = 24, r = 8."""
    import test_gpu_pod as TP
    from conftest import rel_fro, sign_align

    torch = _torch()
    nh, ns, r = 300, 24, 8
    f32 = t == "f32"
    bar = 1e-4 if f32 else 1e-8
    ref = TP._ref(nh, ns, r, f32, xh, False, svd_type)
    S0 = TP._snap(nh, ns, f32)
    assert TP._margin(ref["sigma"][:r], TP.TOL) >= 1e-6
    want_n = TP._rank(ref["sigma"][:r], TP.TOL)
    base = None
    for k in (0, 40, -40):
        W, sigma, N = TP._run(engine, nh, ns, r, f32, xh, False, svd_type, S=TP._dev(np.ldexp(S0, k), f32),
                              truncate=False)
        engine.sync()
        Wt, sigma, N = W.cpu(), sigma.cpu().numpy(), int(N.item())
        base = Wt if base is None else base
        W1 = np.ldexp(Wt.double().numpy(), k)
        s1 = np.ldexp(sigma, -2 * k)
        es = rel_fro(s1[:r], ref["sigma"][:r])
        ew = rel_fro(sign_align(W1[:, :r], ref["W"][:, :r]), ref["W"][:, :r])
        same = torch.equal(torch.ldexp(Wt.double(), torch.tensor(k)), base.double())
        print(f"SCALE pod{t[1:]} svd_type {svd_type} {'Xh' if xh else 'noXh'} k={k:+d}: sigma {es:.2e} W {ew:.2e} "
              f"N {N} (reference {want_n}); 2^k W bit-identical to k = 0: {same}")
        assert np.isfinite(sigma).all() and np.isfinite(W1).all()
        assert es < bar and ew < bar, (t, svd_type, xh, k, es, ew)
        assert N == want_n, (N, want_n)
