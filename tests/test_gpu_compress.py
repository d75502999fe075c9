"""GPU: the rank-k compression (Engine.compress_batched / compress_tiles / lowrank ->
rsvd_compress_batched / rsvd_lowrank) against the fp64 CPU oracle run per matrix with the same Omega:
C_o = U_o[:, :k] diag(S_o[:k]) V_o[:, :k]^T.

Inputs are the family of tests/test_gpu_batched.py (its cached matrices, Omegas and oracle runs are
shared, so every reference is computed once): gapped_matrix(m, n, min(3 l, m, n), decay=0.85,
seed=1000 m + n + l + b), Omega_b = oracle.generate_omega(n, l, 99 + b), fp32 cases round both first.
Bars (none of them taken from what the code gives):

  parity        rel_fro(C, C_o) < 1e-8 (fp64), < 1e-4 (fp32): test_gpu_batched._parity's bars for the vectors
  consistency   rel_fro(C, (U[:, :k] S[:k]) V[:, :k]^T in float64 on the host) < 1e-12 (fp64), < 1e-5 (fp32)
  error words   against ||A||_F^2 and ||A - C||_F^2 recomputed in float64 from A and the returned C, 1e-10
                relative: m n <= 65536 non-negative fp64 terms, (m n + 3) 2^-53 ~ 7e-12
  Pythagoras    |err1 - (err0 - sum_{i<k} S_i^2)| <= tol err0, tol 1e-10 (fp64), 1e-4 (fp32): C_k is an
                orthogonal projection of A; the bars are the project's orthonormality bars

test_parity_every_instantiation holds the rows of tests/batched_cases.COMPRESS_CASES to the same four checks:
the compress tail at LP 32, 48 and 64 in both types and both panel locations, at ranks whose ceil(k / 8)
does not divide the workgroup.  Measured on an MI355X over those rows: parity 2.2e-14 (fp64), 7.5e-6 (fp32,
64 x 64 x 64; 8.2e-7 elsewhere); factors 2.0e-16, 7.0e-8; Pythagoras 1.2e-14, 3.9e-7.  lowrank.hip on its own
is in tests/test_gpu_lowrank.py.
"""
import numpy as np
import pytest

import batched_cases as bc
import test_gpu_batched as TB
from conftest import rel_fro
from padded import _Padded
from ws_patterns import PATTERNS

pytestmark = pytest.mark.gpu

SHAPES = [(70, 45, 8, 2), (33, 17, 5, 1), (17, 200, 16, 2), (16, 16, 16, 0)]
_torch, _tdt, _matrix, _omega, _ref, _dev_batch = TB._torch, TB._tdt, TB._matrix, TB._omega, TB._ref, TB._dev_batch


def _ks(l):
    return sorted({1, max(1, l // 2), l})


def _c_ref(m, n, l, q, b, ob, f32, k):
    Uo, So, Vo = _ref(m, n, l, q, b, ob, f32)
    return (Uo[:, :k] * So[:k]) @ Vo[:, :k].T


def _om_batch(n, l, bs, f32):
    torch = _torch()
    return torch.from_numpy(np.stack([_omega(n, l, b, f32) for b in bs])).to(_tdt(f32))


def _np(t):
    return t.cpu().double().numpy()


def _check_err_words(tag, err, A, C, rtol=1e-10):
    """err = (||A||^2, ||A - C||^2) recomputed in float64 on the host from A and the returned C."""
    a2, e2 = float(np.sum(A * A)), float(np.sum((A - C) ** 2))
    print(f"COMPRESS {tag}: err {err[0]:.6e} {err[1]:.6e} host {a2:.6e} {e2:.6e}")
    assert abs(err[0] - a2) <= rtol * a2, (tag, err[0], a2)
    assert abs(err[1] - e2) <= rtol * e2 + 1e-300, (tag, err[1], e2)


# ---- 1-4. parity, consistency with the call's own factors, the error words, the known answer --------
def _four_checks(engine, m, n, l, q, f32, B, ks):
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, f32) for b in range(B)], f32)
    om = _om_batch(n, l, range(B), f32)
    tol_p, tol_c, tol_o = (1e-4, 1e-5, 1e-4) if f32 else (1e-8, 1e-12, 1e-10)
    for k in ks:
        C, err, (U, S, V) = engine.compress_batched(A, l, k=k, q=q, omega=om, return_factors=True)
        assert C.shape == (B, m, n) and C.dtype == _tdt(f32) and C.stride(1) == 1
        assert err.shape == (B, 2) and err.dtype == _torch().float64
        C, err, U, S, V = _np(C), _np(err), _np(U), _np(S), _np(V)
        for b in range(B):
            Ab = _matrix(m, n, l, b, f32)
            ep = rel_fro(C[b], _c_ref(m, n, l, q, b, b, f32, k))
            ec = rel_fro(C[b], (U[b][:, :k] * S[b][:k]) @ V[b][:, :k].T)
            py = abs(err[b, 1] - (err[b, 0] - np.sum(S[b][:k] ** 2))) / err[b, 0]
            print(f"COMPRESS {m}x{n} l{l} q{q} k{k} b{b}: parity {ep:.2e} factors {ec:.2e} pythagoras {py:.2e}")
            assert ep < tol_p and ec < tol_c, (k, b, ep, ec)
            _check_err_words(f"{m}x{n} k{k} b{b}", err[b], Ab, C[b])
            assert py <= tol_o, (k, b, py)
            if l == m == n == k:  # the known answer: all of a full-rank square matrix
                assert err[b, 1] <= tol_o * err[b, 0], (b, err[b])


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("m,n,l,q", SHAPES)
def test_parity_consistency_and_error_words(engine, m, n, l, q, f32):
    _four_checks(engine, m, n, l, q, f32, 3, _ks(l))


def _ks_wide(l):
    """_ks(l) and the ranks below l at which ceil(k / 8) = 3, 5, 6, 7 does not divide the workgroup: the
    round of scale_panel then leaves a spare group of threads (ch == nch) beside the working ones."""
    return sorted(set(_ks(l)) | {k for k in (17, 33, 41, 49) if k < l})


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("m,n,l,q", bc.COMPRESS_CASES, ids=[bc.case_id(c) for c in bc.COMPRESS_CASES])
def test_parity_every_instantiation(engine, m, n, l, q, f32):
    """The compress tail at LP 32, 48 and 64 in both types and both panel locations (the rows of
    tests/batched_cases.py; where each runs is checked on the CPU by tests/test_batched_cases.py), with odd
    l, more panel rows than one round of scale_panel holds (200 and 256 rows) and the ranks of _ks_wide."""
    t, LP, loc = bc.placement(m, n, l, q, f32, batch=2)
    print(f"COMPRESS {m}x{n} l{l}: {t} LP{LP} panels in {loc}, k in {_ks_wide(l)}")
    _four_checks(engine, m, n, l, q, f32, 2, _ks_wide(l))


def test_parity_panels_in_workspace(engine):
    """256 x 256, l = 64, fp64: LP = 64 and the panels (the factors of the rebuild) in the workspace."""
    m, n, l, q, B, f32 = 256, 256, 64, 2, 2, False
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, f32) for b in range(B)], f32)
    om = _om_batch(n, l, range(B), f32)
    for k in _ks(l):
        C, err, (U, S, V) = engine.compress_batched(A, l, k=k, q=q, omega=om, return_factors=True)
        C, err, U, S, V = _np(C), _np(err), _np(U), _np(S), _np(V)
        for b in range(B):
            ep = rel_fro(C[b], _c_ref(m, n, l, q, b, b, f32, k))
            ec = rel_fro(C[b], (U[b][:, :k] * S[b][:k]) @ V[b][:, :k].T)
            py = abs(err[b, 1] - (err[b, 0] - np.sum(S[b][:k] ** 2))) / err[b, 0]
            print(f"COMPRESS 256x256 l64 k{k} b{b}: parity {ep:.2e} factors {ec:.2e} pythagoras {py:.2e}")
            assert ep < 1e-8 and ec < 1e-12 and py <= 1e-10, (k, b, ep, ec, py)
            _check_err_words(f"256x256 k{k} b{b}", err[b], _matrix(m, n, l, b, f32), C[b])


# ---- 5. the factors are rsvd_batched's; C and err do not depend on asking for them ---------------------
@pytest.mark.parametrize("m,n,l,q,f32", [(70, 45, 8, 2, False), (33, 17, 5, 1, True), (256, 256, 64, 2, False),
                                         (90, 50, 33, 2, True), (200, 100, 47, 1, False)],
                         ids=["f64", "f32", "panels-in-workspace", "f32-lp48", "f64-lp48-panels-in-workspace"])
def test_factors_untouched(engine, m, n, l, q, f32):
    torch = _torch()
    B = 3 if m < 256 else 2
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, f32) for b in range(B)], f32)
    om = _om_batch(n, l, range(B), f32)
    U0, S0, V0, info0 = engine.rsvd_batched(A, l, q=q, omega=om, return_info=True)
    k = max(1, l // 2)
    C, err, (U, S, V), info = engine.compress_batched(A, l, k=k, q=q, omega=om, return_factors=True, return_info=True)
    C2, err2 = engine.compress_batched(A, l, k=k, q=q, omega=om)
    assert torch.equal(U, U0) and torch.equal(S, S0) and torch.equal(V, V0) and torch.equal(info, info0)
    assert torch.equal(C, C2) and torch.equal(err, err2)
    E = engine.compress_batched(A, l, k=k, q=q, omega=om, out=None, return_err=False)
    assert torch.equal(E, C)


# ---- 6. the tile grid, out of place and in place --------------------------------------------------------
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
def test_tile_grid_out_of_place_and_in_place(engine, f32):
    torch = _torch()
    tm, tn, l, q, gr, gc, lda, k = 37, 29, 6, 2, 3, 2, 114, 3
    assert engine.batched_is_fused(tm, tn, l, _tdt(f32), q=q, batch=gr * gc) == 1
    full = np.zeros((gr * tm, gc * tn))
    for j in range(gc):
        for i in range(gr):
            full[i * tm:(i + 1) * tm, j * tn:(j + 1) * tn] = _matrix(tm, tn, l, i + gr * j, f32)

    def grid_buffer():
        flat = torch.full((1 + lda * gc * tn,), 7.0, dtype=_tdt(f32), device="cuda")
        M = flat[1:].view(gc * tn, lda)[:, :gr * tm].t()  # base one element past the allocation, lda = 114
        assert M.shape == (111, 58) and M.stride() == (1, lda)
        return flat, M

    flat_a, A = grid_buffer()
    A.copy_(torch.from_numpy(full))
    before = flat_a.clone()
    flat_c, Cout = grid_buffer()
    om = _om_batch(tn, l, range(gr * gc), f32)
    C, err = engine.compress_tiles(A, tm, tn, l, k=k, q=q, omega=om, out=Cout)
    assert C.data_ptr() == Cout.data_ptr() and err.shape == (gr, gc, 2)
    assert torch.equal(flat_a.view(torch.uint8), before.view(torch.uint8))  # A is bit-unchanged
    pad = torch.ones_like(flat_c, dtype=torch.bool)
    pad[1:].view(gc * tn, lda)[:, :gr * tm] = False
    assert bool((flat_c[pad] == 7.0).all())  # the padding around C too
    Ch, eh = _np(C), _np(err)
    for j in range(gc):
        for i in range(gr):
            b = i + gr * j
            blk = (slice(i * tm, (i + 1) * tm), slice(j * tn, (j + 1) * tn))
            ep = rel_fro(Ch[blk], _c_ref(tm, tn, l, q, b, b, f32, k))
            print(f"COMPRESS tile ({i}, {j}): parity {ep:.2e}")
            assert ep < (1e-4 if f32 else 1e-8), (i, j, ep)
            _check_err_words(f"tile ({i}, {j})", eh[i, j], full[blk], Ch[blk])
    Cin, err_in = engine.compress_tiles(A, tm, tn, l, k=k, q=q, omega=om, in_place=True)
    assert Cin.data_ptr() == A.data_ptr()
    assert torch.equal(Cin, C) and torch.equal(err_in, err)
    rows = flat_a[1:].view(gc * tn, lda)
    assert bool((rows[:, gr * tm:] == 7.0).all()) and float(flat_a[0]) == 7.0  # rows 111..113 and the element before


# ---- 7. rank-deficient tiles ----------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_rank_deficient_tiles(engine, f32):
    m, n, l, q, B, k = 40, 24, 8, 2, 4, 8
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=B) == 1
    mats = [np.zeros((m, n)), np.ones((m, n)), np.arange(1, m * n + 1, dtype=np.float64).reshape(m, n),
            np.array(_matrix(m, n, l, 3, f32))]
    C, err = engine.compress_batched(_dev_batch(mats, f32), l, k=k, q=q, omega=_om_batch(n, l, range(B), f32))
    C, err = _np(C), _np(err)
    print(f"COMPRESS deficient: err {err.tolist()}")
    assert np.all(C[0] == 0.0) and err[0, 0] == 0.0 and err[0, 1] == 0.0
    rec_tol = 1e-5 if f32 else 1e-9  # test_rank_deficient_neighbours' reconstruction bar
    for b in (1, 2):
        assert err[b, 1] <= rec_tol ** 2 * err[b, 0], (b, err[b])
    assert rel_fro(C[3], _c_ref(m, n, l, q, 3, 3, f32, k)) < (1e-4 if f32 else 1e-8)


# ---- 8. position, grid and workspace --------------------------------------------------------------------
@pytest.mark.parametrize("m,n,l,q,f32", [(37, 29, 6, 2, True), (70, 45, 8, 2, False)], ids=["f32", "f64"])
def test_position_does_not_matter(engine, m, n, l, q, f32):
    torch = _torch()
    order = [0, 1, 2, 3, 0]
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=5) == 1
    A5 = _dev_batch([_matrix(m, n, l, b, f32) for b in order], f32)
    om5 = _om_batch(n, l, order, f32)
    C5, e5 = engine.compress_batched(A5, l, k=l // 2, q=q, omega=om5)
    C1, e1 = engine.compress_batched(A5[:1], l, k=l // 2, q=q, omega=om5[:1])
    assert torch.equal(C5[0], C5[4]) and torch.equal(e5[0], e5[4])
    assert torch.equal(C5[0], C1[0]) and torch.equal(e5[0], e1[0])
    assert not torch.equal(C5[0], C5[1])


def test_more_matrices_than_one_launch_has_workgroups(engine):
    torch = _torch()
    m, n, l, q, k = 16, 16, 4, 1, 2
    order = [0, 1, 2, 3, 0] + list(range(5, 600))
    B = len(order)
    assert engine.batched_is_fused(m, n, l, torch.float32, q=q, batch=B) == 1
    mats = [_matrix(m, n, l, b, True) for b in order]
    A = _dev_batch(mats, True)
    C, err = engine.compress_batched(A, l, k=k, q=q, omega=_om_batch(n, l, order, True))
    assert torch.equal(C[0], C[4]) and torch.equal(err[0], err[4])
    Ch, eh, Ah = _np(C), _np(err), np.stack(mats)
    a2 = np.sum(Ah * Ah, axis=(1, 2))
    e2 = np.sum((Ah - Ch) ** 2, axis=(1, 2))
    wa, we = np.max(np.abs(eh[:, 0] - a2) / a2), np.max(np.abs(eh[:, 1] - e2) / e2)
    print(f"COMPRESS 600 x 16x16: worst error-word deviation {wa:.2e} {we:.2e}")
    assert wa <= 1e-10 and we <= 1e-10


@pytest.mark.parametrize("m,n,l,q", [(70, 45, 8, 2), (256, 256, 64, 1)], ids=["panels-in-lds", "panels-in-workspace"])
def test_workspace_contents_do_not_matter(engine, m, n, l, q):
    torch = _torch()
    B = 3
    assert engine.batched_is_fused(m, n, l, torch.float64, q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, False) for b in range(B)], False)
    om = _om_batch(n, l, range(B), False)
    engine.compress_batched(A, l, k=l // 2, q=q, omega=om)  # sizes the workspace
    results = []
    for name, byte in PATTERNS.items():
        engine.workspace().fill_(byte)
        torch.cuda.synchronize()
        results.append((name, engine.compress_batched(A, l, k=l // 2, q=q, omega=om)))
    for name, res in results[1:]:
        for X, X0 in zip(res, results[0][1]):
            assert torch.equal(X, X0), name
    assert all(bool(torch.isfinite(X).all()) for X in results[0][1])


# ---- 9. a_scale -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_a_scale(engine, f32):
    """C approximates a_scale A: the kernel scales its fp64 sum and rounds to T once.  In fp64 scaling
    the stored C does the same rounding (exact); in fp32 the stored C was already rounded once: 2^-23."""
    torch = _torch()
    m, n, l, q, B, k = 37, 29, 6, 2, 3, 3
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, f32) for b in range(B)], f32)
    om = _om_batch(n, l, range(B), f32)
    C, err = engine.compress_batched(A, l, k=k, q=q, omega=om)
    C2, err2 = engine.compress_batched(A, l, k=k, q=q, omega=om, a_scale=-2.5)
    if f32:
        assert bool(((C2.double() + C.double() * 2.5).abs() <= 2.0 ** -23 * C.double().abs() * 2.5).all())
    else:
        assert torch.equal(C2, C * -2.5)
    assert bool(((err2[:, 0] - 6.25 * err[:, 0]).abs() <= 1e-12 * 6.25 * err[:, 0]).all())


# ---- 10. lowrank alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,l,dt,pad", [(300, 40, 8, "float64", 0), (128, 96, 16, "bfloat16", 0),
                                          (130, 67, 16, "float32", 3)], ids=["f64", "bf16-A", "f32-padded"])
def test_lowrank_alone(engine, m, n, l, dt, pad):
    torch = _torch()
    tdt = getattr(torch, dt)
    odt = engine.out_dtype(tdt)
    f32 = dt == "float32"
    A = torch.from_numpy(np.array(_matrix(m, n, l, 0, f32))).to(tdt).cuda().t().contiguous().t()
    U, S, V = engine.rsvd(A, l, q=1, seed=5)
    Ah, Uh, Sh, Vh = _np(A), _np(U), _np(S), _np(V)
    for k in (1, l):
        if pad:
            P = _Padded(m, n, m + pad, odt)
            C, err = engine.lowrank(U, S, V, k=k, A=A, out=P.mat)
            assert P.padding_untouched() and bool(torch.isfinite(P.mat).all())
        else:
            C, err = engine.lowrank(U, S, V, k=k, A=A)
        assert C.shape == (m, n) and C.dtype == odt and C.stride(0) == 1 and err.shape == (2,)
        Ch = _np(C)
        ec = rel_fro(Ch, (Uh[:, :k] * Sh[:k]) @ Vh[:, :k].T)
        print(f"LOWRANK {m}x{n} {dt} k{k}: against the host product {ec:.2e}")
        assert ec < (1e-12 if odt == torch.float64 else 1e-5), (k, ec)
        _check_err_words(f"lowrank {dt} k{k}", _np(err), Ah, Ch, rtol=1e-10 * max(1.0, m * n / 65536))
        assert torch.equal(engine.lowrank(U, S, V, k=k, A=A, out=False), err)  # C = NULL: the same words
        C2, err2 = engine.lowrank(U, S, V, k=k, A=A)
        assert torch.equal(C2, C) and torch.equal(err2, err)
        assert torch.equal(engine.lowrank(U, S, V, k=k), C)  # without A: C alone


def test_lowrank_in_place(engine):
    torch = _torch()
    m, n, l = 130, 67, 16
    A = torch.from_numpy(np.array(_matrix(m, n, l, 0, True))).float().cuda().t().contiguous().t()
    U, S, V = engine.rsvd(A, l, q=1, seed=5)
    C, err = engine.lowrank(U, S, V, k=8, A=A)
    W = A.clone()
    C2, err2 = engine.lowrank(U, S, V, k=8, A=W, out=W)
    assert C2.data_ptr() == W.data_ptr() and torch.equal(W, C) and torch.equal(err2, err)


# ---- 11. the looped path --------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,l,q,dt", [(300, 40, 8, 1, "float64"), (128, 96, 16, 1, "bfloat16")])
def test_looped_path_is_rsvd_then_lowrank(engine, m, n, l, q, dt):
    torch = _torch()
    tdt = getattr(torch, dt)
    B, s, k = 2, 31, l // 2
    assert engine.batched_is_fused(m, n, l, tdt, q=q, batch=B) == 0
    A = _dev_batch([_matrix(m, n, l, b, False) for b in range(B)], False).to(tdt)
    A = A.transpose(1, 2).contiguous().transpose(1, 2)
    C, err, (U, S, V), info = engine.compress_batched(A, l, k=k, q=q, seed=s, return_factors=True, return_info=True)
    C2, err2 = engine.compress_batched(A, l, k=k, q=q, seed=s)  # factors in the workspace
    assert C.dtype == engine.out_dtype(tdt) and info.shape == (B, 2) and not bool((info[:, 1] & 2).any())
    for b in range(B):
        Ub, Sb, Vb = engine.rsvd(A[b], l, q=q, seed=s + b)
        Cb, eb = engine.lowrank(Ub, Sb, Vb, k=k, A=A[b])
        assert torch.equal(U[b], Ub) and torch.equal(S[b], Sb) and torch.equal(V[b], Vb)
        for X, e in ((C, err), (C2, err2)):
            assert torch.equal(X[b], Cb) and torch.equal(e[b], eb)


# ---- 12. a non-default stream ---------------------------------------------------------------------------
def test_non_default_stream(engine):
    torch = _torch()
    m, n, l, q, B = 37, 29, 6, 2, 6
    assert engine.batched_is_fused(m, n, l, torch.float32, q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, True) for b in range(B)], True)
    om = _om_batch(n, l, range(B), True).cuda()
    ref = engine.compress_batched(A, l, k=3, q=q, omega=om)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        res = engine.compress_batched(A, l, k=3, q=q, omega=om, check_errors=False)
    st.synchronize()
    for X, X0 in zip(res, ref):
        assert torch.equal(X, X0)
    engine.sync()


# ---- 13. NaN in one matrix ------------------------------------------------------------------------------
def test_nan_in_one_matrix(engine):
    torch = _torch()
    import rsvd_kamaneh_raganato_terrana_amd as R

    m, n, l, q, B, k = 33, 17, 5, 1, 4, 2
    assert engine.batched_is_fused(m, n, l, torch.float64, q=q, batch=B) == 1
    mats = [np.array(_matrix(m, n, l, b, False)) for b in range(B)]
    mats[2][3, 4] = np.nan
    om = _om_batch(n, l, range(B), False)
    C, err, info = engine.compress_batched(_dev_batch(mats, False), l, k=k, q=q, omega=om, return_info=True,
                                           check_errors=False)
    with pytest.raises(R.RSVDError) as ei:
        engine.sync()
    assert ei.value.status == 5  # RSVD_ERR_NUMERICAL
    info = info.cpu().numpy()
    assert info[2, 1] & 2 and not any(info[b, 1] & 2 for b in (0, 1, 3))
    C = _np(C)
    for b in (0, 1, 3):
        assert rel_fro(C[b], _c_ref(m, n, l, q, b, b, False, k)) < 1e-8, b
    clean = _dev_batch([_matrix(m, n, l, b, False) for b in range(B)], False)
    C = _np(engine.compress_batched(clean, l, k=k, q=q, omega=om)[0])  # the sticky word was cleared when reported
    assert rel_fro(C[2], _c_ref(m, n, l, q, 2, 2, False, k)) < 1e-8
