"""GPU: the batched rSVD (Engine.rsvd_batched / rsvd_tiles -> rsvd_run_batched) against the fp64 CPU
oracle run per matrix with the same Omega, at the bars of tests/test_gpu_parity.py:

  fp64  rel_fro(S) < 1e-10; leading l // 2 columns of U and V, sign-aligned, < 1e-8;
        ||U^T U - I||_F and ||V^T V - I||_F < 1e-10
  fp32  1e-4 on all of those (inputs rounded to fp32 first)

Inputs: gapped_matrix(m, n, min(3 l, m, n), decay=0.85, seed=1000 m + n + l + b) and
Omega_b = oracle.generate_omega(n, l, 99 + b).  Every case asserts batched_is_fused == 1 first (the
kernel ran, not the loop) unless it is about the loop.  The shapes are the smallest at which each
thing can go wrong: l == m == n, l < 16 in a padded LP, odd sizes, one side past 64 rows (more than
one row per lane of a reflector), 256 x 256 x 64 fp64 (panels in the workspace instead of LDS), and
more matrices than one launch has workgroups' worth of compute units.

test_parity_every_instantiation runs the rows of tests/batched_cases.py (B = 2, an Omega per matrix, the
same bars): every (type, LP, panel location) the kernel can be launched with, LP = 48 (384 threads) among
them, odd l above 16, l = 1 (where the single column is compared: k = max(1, l // 2)) and both sides of the
two LDS budgets.  Measured on an MI355X over those rows: fp64 S 8.6e-15, U and V 3.4e-14, orthonormality
1.5e-13; fp32 S 7.5e-6 (64 x 64 x 64, last singular value 3.5e-5), U and V 8.9e-7, orthonormality 6.8e-6.
Found with it: Engine.rsvd_batched / compress_batched passed the stride of Omega's one-column dimension as
its leading dimension at l = 1, and 9 x 7 x 1 with an Omega per matrix was refused as an invalid argument."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import batched_cases as bc
from conftest import gapped_matrix, rel_fro, sign_align
from ws_patterns import PATTERNS

pytestmark = pytest.mark.gpu

SHAPES = [(70, 45, 8, 2), (256, 256, 32, 2), (256, 256, 64, 2), (16, 16, 16, 0), (33, 17, 5, 1), (17, 200, 16, 2),
          (37, 29, 6, 2), (16, 16, 4, 1)]


def _torch():
    import torch

    return torch


def _tdt(f32):
    torch = _torch()
    return torch.float32 if f32 else torch.float64


def _round(X, f32):
    return X.astype(np.float32).astype(np.float64) if f32 else X


@functools.lru_cache(maxsize=None)
def _matrix(m, n, l, b, f32):
    A = _round(gapped_matrix(m, n, min(3 * l, m, n), decay=0.85, seed=1000 * m + n + l + b), f32)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _omega(n, l, b, f32):
    Om = _round(oracle.generate_omega(n, l, 99 + b), f32)
    Om.setflags(write=False)
    return Om


@functools.lru_cache(maxsize=None)
def _ref(m, n, l, q, b, ob, f32):
    """The oracle's rSVD of matrix b with Omega ob (computed once, shared by every test that needs it)."""
    return oracle.rsvd(_matrix(m, n, l, b, f32), l, q=q, Omega=_omega(n, l, ob, f32))


def _dev_batch(mats, f32):
    """(B, m, n) on the device, every matrix column-major."""
    torch = _torch()
    t = torch.from_numpy(np.stack(mats)).to(_tdt(f32)).cuda()
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _host(*ts):
    return tuple(t.cpu().double().numpy() for t in ts)


def _parity(tag, U, S, V, ref, l, f32):
    Uo, So, Vo = ref
    tol_s, tol_v, tol_o = (1e-4, 1e-4, 1e-4) if f32 else (1e-10, 1e-8, 1e-10)
    k = max(1, l // 2)  # l = 1: the single column
    es = rel_fro(S, So)
    eu = rel_fro(sign_align(U[:, :k], Uo[:, :k]), Uo[:, :k])
    ev = rel_fro(sign_align(V[:, :k], Vo[:, :k]), Vo[:, :k])
    ou = np.linalg.norm(U.T @ U - np.eye(l))
    ov = np.linalg.norm(V.T @ V - np.eye(l))
    print(f"BATCHED {tag}: S {es:.2e} U {eu:.2e} V {ev:.2e} orthU {ou:.2e} orthV {ov:.2e}")
    assert es < tol_s and eu < tol_v and ev < tol_v and ou < tol_o and ov < tol_o, (tag, es, eu, ev, ou, ov)


# ---- 1. parity ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["omega-per-matrix", "omega-shared"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("m,n,l,q", SHAPES)
def test_parity(engine, m, n, l, q, f32, shared):
    torch = _torch()
    B = 6
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, f32) for b in range(B)], f32)
    if shared:
        om = torch.from_numpy(np.array(_omega(n, l, 0, f32))).to(_tdt(f32))
    else:
        om = torch.from_numpy(np.stack([_omega(n, l, b, f32) for b in range(B)])).to(_tdt(f32))
    U, S, V = engine.rsvd_batched(A, l, q=q, omega=om)
    assert U.shape == (B, m, l) and S.shape == (B, l) and V.shape == (B, n, l) and U.dtype == _tdt(f32)
    assert U.stride(1) == 1 and V.stride(1) == 1
    U, S, V = _host(U, S, V)
    for b in range(B):
        _parity(f"{m}x{n} l{l} q{q} b{b}", U[b], S[b], V[b], _ref(m, n, l, q, b, 0 if shared else b, f32), l, f32)


# ---- 1b. every reachable instantiation ------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("m,n,l,q", bc.CASES, ids=[bc.case_id(c) for c in bc.CASES])
def test_parity_every_instantiation(engine, m, n, l, q, f32):
    """The rows of tests/batched_cases.py: between them and the two types every (T, LP, panel location) the
    kernel can be launched with runs (tests/test_batched_cases.py checks that on the CPU), with odd l above
    16 (the Jacobi dummy column), l = 1, l = LP = 48 and 64, and the shapes on both sides of each LDS budget."""
    torch = _torch()
    B = 2
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=B) == 1
    t, LP, loc = bc.placement(m, n, l, q, f32, batch=B)
    for pt, inside, past in bc.BUDGET_PAIRS:
        if pt == t and (m, n, l, q) == inside:
            assert bc.workspace_bytes(m, n, l, q, f32, batch=B) == bc.LDS_FLOOR and loc == "lds"
        if pt == t and (m, n, l, q) == past:
            assert bc.workspace_bytes(m, n, l, q, f32, batch=B) > bc.LDS_FLOOR and loc == "ws"
    A = _dev_batch([_matrix(m, n, l, b, f32) for b in range(B)], f32)
    om = torch.from_numpy(np.stack([_omega(n, l, b, f32) for b in range(B)])).to(_tdt(f32))
    U, S, V, info = engine.rsvd_batched(A, l, q=q, omega=om, return_info=True)
    assert U.shape == (B, m, l) and S.shape == (B, l) and V.shape == (B, n, l) and U.dtype == _tdt(f32)
    assert not bool((info[:, 1] & 2).any())
    U, S, V = _host(U, S, V)
    for b in range(B):
        _parity(f"{t} LP{LP} {loc} {m}x{n} l{l} q{q} b{b}", U[b], S[b], V[b], _ref(m, n, l, q, b, b, f32), l, f32)


# ---- 2. Philox seeds ---------------------------------------------------------------------------
def test_philox_seed_plus_b(engine):
    m, n, l, q, B, s = 70, 45, 8, 2, 3, 4242
    assert engine.batched_is_fused(m, n, l, _tdt(False), q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, False) for b in range(B)], False)
    U, S, V = _host(*engine.rsvd_batched(A, l, q=q, seed=s))
    for b in range(B):
        _parity(f"philox b{b}", U[b], S[b], V[b], oracle.rsvd(_matrix(m, n, l, b, False), l, q=q, seed=s + b), l, False)


# ---- 3. tile grid in place ---------------------------------------------------------------------
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
def test_tile_grid_in_place(engine, f32):
    torch = _torch()
    tm, tn, l, q, gr, gc, lda = 37, 29, 6, 2, 3, 2, 114
    assert engine.batched_is_fused(tm, tn, l, _tdt(f32), q=q, batch=gr * gc) == 1
    full = np.zeros((gr * tm, gc * tn))
    for j in range(gc):
        for i in range(gr):
            full[i * tm:(i + 1) * tm, j * tn:(j + 1) * tn] = _matrix(tm, tn, l, i + gr * j, f32)
    flat = torch.full((1 + lda * gc * tn,), 7.0, dtype=_tdt(f32), device="cuda")
    A = flat[1:].view(gc * tn, lda)[:, :gr * tm].t()  # base one element past the allocation, lda = 114
    A.copy_(torch.from_numpy(full))
    assert A.shape == (111, 58) and A.stride() == (1, lda) and A.data_ptr() == flat.data_ptr() + flat.element_size()
    before = flat.clone()
    om = torch.from_numpy(np.stack([_omega(tn, l, b, f32) for b in range(gr * gc)])).to(_tdt(f32))
    U, S, V, info = engine.rsvd_tiles(A, tm, tn, l, q=q, omega=om, return_info=True)
    assert U.shape == (gr, gc, tm, l) and S.shape == (gr, gc, l) and V.shape == (gr, gc, tn, l)
    assert info.shape == (gr, gc, 2) and bool((info[..., 0] > 0).all()) and not bool((info[..., 1] & 2).any())
    assert torch.equal(flat.view(torch.uint8), before.view(torch.uint8))  # A is bit-unchanged
    U, S, V = _host(U, S, V)
    for j in range(gc):
        for i in range(gr):
            b = i + gr * j
            _parity(f"tile ({i}, {j})", U[i, j], S[i, j], V[i, j], _ref(tm, tn, l, q, b, b, f32), l, f32)


# ---- 4. padded outputs through the ctypes entry point -----------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_padded_outputs(engine, f32):
    torch = _torch()
    from rsvd_kamaneh_raganato_terrana_amd import _capi

    m, n, l, q, B = 33, 17, 5, 1, 3
    ldu, ldv = m + 3, n + 5
    us, ss, vs = ldu * l + 7, l + 1, ldv * l + 7
    idt = torch.int32 if f32 else torch.int64
    pattern = 0x7FC12345 if f32 else 0x7FF8000000012345  # the NaN patterns of tests/padded.py
    A = _dev_batch([_matrix(m, n, l, b, f32) for b in range(B)], f32)
    om = torch.from_numpy(np.stack([_omega(n, l, b, f32) for b in range(B)])).to(_tdt(f32)).cuda()
    om = om.transpose(1, 2).contiguous().transpose(1, 2)
    bufs = [torch.full((1 + B * s,), pattern, dtype=idt, device="cuda") for s in (us, ss, vs)]
    d = _capi.Desc(m=m, n=n, lda=A.stride(2), l=l, q=q, dtype=_capi.F32 if f32 else _capi.F64, method=0, qr_mode=0,
                   flags=0, seed=0, a_scale=1.0)
    bd = _capi.BatchDesc(count0=B, count1=1, a_stride0=A.stride(0), a_stride1=0, omega_stride=om.stride(0),
                         u_stride=us, s_stride=ss, v_stride=vs)
    L = _capi.lib()
    assert L.rsvd_batched_is_fused(ctypes.byref(d), ctypes.byref(bd)) == 1
    nb = ctypes.c_size_t(0)
    _capi.check(L.rsvd_batched_workspace_bytes(ctypes.byref(d), ctypes.byref(bd), ctypes.byref(nb)))
    engine._reserve_bytes(nb.value)
    engine._bind_stream()
    es = bufs[0].element_size()
    _capi.check(L.rsvd_run_batched(engine.h, ctypes.byref(d), ctypes.byref(bd), ctypes.c_void_p(A.data_ptr()),
                                   ctypes.c_void_p(om.data_ptr()), om.stride(2),
                                   ctypes.c_void_p(bufs[0].data_ptr() + es), ldu,
                                   ctypes.c_void_p(bufs[1].data_ptr() + es),
                                   ctypes.c_void_p(bufs[2].data_ptr() + es), ldv, None), engine.h)
    engine.sync()
    for buf, stride, ld, rows, cols in ((bufs[0], us, ldu, m, l), (bufs[1], ss, l, l, 1), (bufs[2], vs, ldv, n, l)):
        inside = torch.zeros_like(buf, dtype=torch.bool)
        for b in range(B):
            inside[1 + b * stride: 1 + b * stride + ld * cols].view(cols, ld)[:, :rows] = True
        assert bool((buf[~inside] == pattern).all())
        assert bool(torch.isfinite(buf.view(_tdt(f32))[inside]).all())
    for b in range(B):  # and the values landed where the strides say
        U = bufs[0][1 + b * us: 1 + b * us + ldu * l].view(_tdt(f32)).view(l, ldu)[:, :m].t()
        S = bufs[1][1 + b * ss: 1 + b * ss + l].view(_tdt(f32))
        V = bufs[2][1 + b * vs: 1 + b * vs + ldv * l].view(_tdt(f32)).view(l, ldv)[:, :n].t()
        _parity(f"padded b{b}", *_host(U, S, V), _ref(m, n, l, q, b, b, f32), l, f32)


# ---- 5. rank deficiency inside a batch ---------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_rank_deficient_neighbours(engine, f32):
    torch = _torch()
    m, n, l, q, B = 40, 24, 8, 2, 4
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=B) == 1
    mats = [np.zeros((m, n)), np.ones((m, n)), np.arange(1, m * n + 1, dtype=np.float64).reshape(m, n),
            np.array(_matrix(m, n, l, 3, f32))]
    om = torch.from_numpy(np.stack([_omega(n, l, b, f32) for b in range(B)])).to(_tdt(f32))
    U, S, V, info = engine.rsvd_batched(_dev_batch(mats, f32), l, q=q, omega=om, return_info=True)
    info = info.cpu().numpy()
    U, S, V = _host(U, S, V)
    orth, rec_tol, tail, lead = (1e-4, 1e-5, 1e-4, 1e-5) if f32 else (1e-10, 1e-9, 1e-9, 1e-10)
    for b in range(B):
        ou = np.linalg.norm(U[b].T @ U[b] - np.eye(l))
        ov = np.linalg.norm(V[b].T @ V[b] - np.eye(l))
        print(f"BATCHED deficient b{b}: S {S[b]} orthU {ou:.2e} orthV {ov:.2e} info {info[b]}")
        assert ou < orth and ov < orth, (b, ou, ov)
        assert np.all(np.diff(S[b]) <= 0) and np.all(S[b] >= 0)
    assert np.all(S[0] == 0.0)
    s1 = np.sqrt(m * n)
    assert abs(S[1][0] - s1) < (1e-5 if f32 else 1e-10) * s1 and np.max(S[1][1:]) < tail * s1
    sv = np.linalg.svd(mats[2], compute_uv=False)
    if f32:
        assert rel_fro(S[2][:2], sv[:2]) < lead
    else:
        assert abs(S[2][0] - sv[0]) < 1e-10 * sv[0] and abs(S[2][1] - sv[1]) < 1e-8 * sv[0]
    assert np.max(S[2][2:]) < tail * sv[0]
    for b in (0, 1, 2):
        rec = np.linalg.norm(mats[b] - (U[b] * S[b]) @ V[b].T)
        print(f"BATCHED deficient b{b}: reconstruction {rec:.2e} of {np.linalg.norm(mats[b]):.2e}")
        assert rec <= rec_tol * np.linalg.norm(mats[b]), (b, rec)
        assert info[b, 1] & 1, (b, info[b])
    _parity("deficient b3", U[3], S[3], V[3], _ref(m, n, l, q, 3, 3, f32), l, f32)
    if not f32:  # what the oracle itself returns for the exactly low-rank ones
        So1 = oracle.rsvd(np.asfortranarray(mats[1]), l, q=q, Omega=_omega(n, l, 1, False))[1]
        So2 = oracle.rsvd(np.asfortranarray(mats[2]), l, q=q, Omega=_omega(n, l, 2, False))[1]
        assert abs(So1[0] - s1) < 1e-10 * s1 and So1[1] < 1e-9 * s1
        assert abs(So2[0] - sv[0]) < 1e-10 * sv[0] and So2[2] < 1e-9 * sv[0]


# ---- 6. independence of position and neighbours ------------------------------------------------
@pytest.mark.parametrize("m,n,l,q,f32", [(37, 29, 6, 2, True), (70, 45, 8, 2, False)], ids=["f32", "f64"])
def test_position_and_neighbours_do_not_matter(engine, m, n, l, q, f32):
    torch = _torch()
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=5) == 1
    order = [0, 1, 2, 3, 0]
    A5 = _dev_batch([_matrix(m, n, l, b, f32) for b in order], f32)
    om5 = torch.from_numpy(np.stack([_omega(n, l, b, f32) for b in order])).to(_tdt(f32))
    U5, S5, V5 = engine.rsvd_batched(A5, l, q=q, omega=om5)
    U1, S1, V1 = engine.rsvd_batched(A5[:1], l, q=q, omega=om5[:1])
    for X5, X1 in ((U5, U1), (S5, S1), (V5, V1)):
        assert torch.equal(X5[0], X5[4])
        assert torch.equal(X5[0], X1[0])
        assert not torch.equal(X5[0], X5[1])


# ---- 7. more matrices than compute units -------------------------------------------------------
def test_more_matrices_than_compute_units(engine):
    torch = _torch()
    m, n, l, q, B = 16, 16, 4, 1, 600
    assert engine.batched_is_fused(m, n, l, torch.float32, q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, True) for b in range(B)], True)
    om = torch.from_numpy(np.stack([_omega(n, l, b, True) for b in range(B)])).float()
    S = engine.rsvd_batched(A, l, q=q, omega=om)[1].cpu().double().numpy()
    worst = max(rel_fro(S[b], _ref(m, n, l, q, b, b, True)[1]) for b in range(B))
    print(f"BATCHED 600 x 16x16: worst S error {worst:.2e}")
    assert worst < 1e-4


# ---- 8. workspace contents ---------------------------------------------------------------------
@pytest.mark.parametrize("m,n,l,q", [(70, 45, 8, 2), (256, 256, 64, 1), (150, 125, 48, 1)],
                         ids=["panels-in-lds", "panels-in-workspace", "lp48-panels-in-workspace"])
def test_workspace_contents_do_not_matter(engine, m, n, l, q):
    torch = _torch()
    B = 6
    assert engine.batched_is_fused(m, n, l, torch.float64, q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, False) for b in range(B)], False)
    om = torch.from_numpy(np.stack([_omega(n, l, b, False) for b in range(B)]))
    engine.rsvd_batched(A, l, q=q, omega=om)  # sizes the workspace
    results = []
    for name, byte in PATTERNS.items():
        engine.workspace().fill_(byte)
        torch.cuda.synchronize()
        results.append((name, engine.rsvd_batched(A, l, q=q, omega=om)))
    for name, res in results[1:]:
        for X, X0 in zip(res, results[0][1]):
            assert torch.equal(X, X0), name
    assert all(bool(torch.isfinite(X).all()) for X in results[0][1])


# ---- 9. non-finite input -----------------------------------------------------------------------
def test_nan_in_one_matrix(engine):
    torch = _torch()
    import rsvd_kamaneh_raganato_terrana_amd as R

    m, n, l, q, B = 33, 17, 5, 1, 4
    assert engine.batched_is_fused(m, n, l, torch.float64, q=q, batch=B) == 1
    mats = [np.array(_matrix(m, n, l, b, False)) for b in range(B)]
    mats[2][3, 4] = np.nan
    om = torch.from_numpy(np.stack([_omega(n, l, b, False) for b in range(B)]))
    U, S, V, info = engine.rsvd_batched(_dev_batch(mats, False), l, q=q, omega=om, return_info=True, check_errors=False)
    with pytest.raises(R.RSVDError) as ei:
        engine.sync()
    assert ei.value.status == 5  # RSVD_ERR_NUMERICAL
    info = info.cpu().numpy()
    assert info[2, 1] & 2 and not any(info[b, 1] & 2 for b in (0, 1, 3))
    U, S, V = _host(U, S, V)
    for b in (0, 1, 3):
        _parity(f"beside NaN b{b}", U[b], S[b], V[b], _ref(m, n, l, q, b, b, False), l, False)
    clean = _dev_batch([_matrix(m, n, l, b, False) for b in range(B)], False)
    U, S, V = _host(*engine.rsvd_batched(clean, l, q=q, omega=om))  # the sticky word was cleared when reported
    _parity("after NaN b2", U[2], S[2], V[2], _ref(m, n, l, q, 2, 2, False), l, False)


# ---- 10. the looped path -----------------------------------------------------------------------
@pytest.mark.parametrize("m,n,l,q,dt", [(300, 40, 8, 1, "float64"), (128, 96, 16, 1, "bfloat16")])
def test_looped_path_is_rsvd_per_matrix(engine, m, n, l, q, dt):
    torch = _torch()
    tdt = getattr(torch, dt)
    B, s = 2, 31
    assert engine.batched_is_fused(m, n, l, tdt, q=q, batch=B) == 0
    A = _dev_batch([_matrix(m, n, l, b, False) for b in range(B)], False).to(tdt)
    A = A.transpose(1, 2).contiguous().transpose(1, 2)
    U, S, V, info = engine.rsvd_batched(A, l, q=q, seed=s, return_info=True)
    assert U.dtype == engine.out_dtype(tdt) and info.shape == (B, 2)
    assert not bool((info[:, 1] & 2).any())
    U2, S2, V2 = engine.rsvd_batched(A, l, q=q, seed=s)  # without info: no per-matrix synchronisation
    for b in range(B):
        Ub, Sb, Vb = engine.rsvd(A[b], l, q=q, seed=s + b)
        for X in ((U, S, V), (U2, S2, V2)):
            assert torch.equal(X[0][b], Ub) and torch.equal(X[1][b], Sb) and torch.equal(X[2][b], Vb)


# ---- 11. stream --------------------------------------------------------------------------------
def test_non_default_stream(engine):
    torch = _torch()
    m, n, l, q, B = 37, 29, 6, 2, 6
    assert engine.batched_is_fused(m, n, l, torch.float32, q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, True) for b in range(B)], True)
    om = torch.from_numpy(np.stack([_omega(n, l, b, True) for b in range(B)])).float().cuda()
    ref = engine.rsvd_batched(A, l, q=q, omega=om)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        res = engine.rsvd_batched(A, l, q=q, omega=om, check_errors=False)
    st.synchronize()
    for X, X0 in zip(res, ref):
        assert torch.equal(X, X0)
    engine.sync()


# ---- 12. a_scale -------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_a_scale_scales_s_and_flips_v(engine, f32):
    """A = a_scale * stored A: S scales by |a_scale|, V changes sign for a_scale < 0, U stays.  The
    kernel rounds the fp64 sigma * |a_scale| to T once.  In fp64 scaling the stored S does the same
    rounding, so the comparison is exact; in fp32 the stored S was already rounded once, and the two
    roundings may differ from the one by an ulp: 2^-23 relative."""
    torch = _torch()
    m, n, l, q, B = 37, 29, 6, 2, 3
    assert engine.batched_is_fused(m, n, l, _tdt(f32), q=q, batch=B) == 1
    A = _dev_batch([_matrix(m, n, l, b, f32) for b in range(B)], f32)
    om = torch.from_numpy(np.stack([_omega(n, l, b, f32) for b in range(B)])).to(_tdt(f32))
    U, S, V = engine.rsvd_batched(A, l, q=q, omega=om)
    U2, S2, V2 = engine.rsvd_batched(A, l, q=q, omega=om, a_scale=-2.5)
    assert torch.equal(U2, U) and torch.equal(V2, -V)
    if f32:
        assert bool(((S2.double() - S.double() * 2.5).abs() <= 2.0 ** -23 * S.double() * 2.5).all())
    else:
        assert torch.equal(S2, S * 2.5)
