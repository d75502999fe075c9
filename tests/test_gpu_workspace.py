"""What a result is allowed to depend on: not on the workspace's previous contents, not on whether
runs were queued or synchronised one by one, not on the stream -- and a run leaves A and Omega alone.

The workspace contract (include/rsvd_c.h at rsvd_set_workspace): contents unspecified on entry and on
return, no state carried between runs.  A freshly mapped block reads as zeros, so a buffer the
kernels never write but do read can pass every other test by luck; here the whole workspace tensor
(Engine.workspace()) is overwritten with a byte pattern (tests/ws_patterns.py: 0x00, 0xFF = NaN in
every float type and 2^32 - 1 as a counter, 0x4B = large finite values) before each run.

a. test_results_do_not_depend_on_workspace: per case one sizing run, then runs over zero, zero
   again (the determinism control), nan and big, each into fresh outputs.  Asserted: the two zero
   runs are bit-identical, the nan and big runs are bit-identical to them, the zero result is finite;
   for the plain ragged cases the zero result also passes test_gpu_ragged.py's oracle check (_check /
   _bounds, imported unchanged) and the splits of the table (the option cases change the algorithm,
   not the layout: identity and finiteness only); the three cases past 512 columns are held to
   finiteness and the orthonormality bounds of test_gpu_big_l.py / test_gpu_dense.py instead of the
   oracle; the four rows of tests/dense_cases.py with padding columns inside LP (Power 90 x 70 in LP
   80, Jacobi 131 x 65 in LP 96, fp32 Jacobi 65 x 131, fp32 QR 517 x 513: all bit-identical on every
   pattern, 2.5 s together) are held to test_gpu_dense_ragged.py's reference check.  Every case prints "WS <case> <pattern>: identical" or the first differing index and the
   largest difference before asserting.
   test_nshard_layout_does_not_depend_on_workspace: the same on the n-side sharded layout at world
   1 (b128v: n = 702 in nfull = 704 rows), in one spawned child as test_gpu_rccl.py's library mode.
b. test_stale_data_of_real_runs: e512n, f32a, bLP, e512n on one handle (large LP, tiny LP, padded
   LP, large again; three dtypes) against each case run first on a fresh Engine.
c. test_queued_runs: four runs queued with check_errors=False, one sync().
   test_queued_calls_across_entry_points: rsvd_batched (fp64, LP 48, panels in the workspace),
   compress_batched (fp32, LP 48, k = 17), pod (with Xh: its regions and a nested solver in the tail),
   lowrank (slots) and the first again, queued on one handle with one sync(), each bit-equal to the same
   call made alone; then again over every fill of the workspace.
d. test_non_default_stream.
e. test_inputs_are_read_only: A and Omega inside guard buffers, every byte unchanged.

Sync words, counters and flags that live in the workspace, and who zeroes each before its first
wait (read from the code; the error and breakdown flags proper live in the handle's own dflags
block, not in the workspace, and reset_run_flags clears the per-run ones):
  driver.cpp Layout      ctr[64]: [0..1] cumulative arrival counters of gram_kernel (qr.hip
                         spin_until), [8..59] private counters of predicated passes, [62..63] the
                         refine words -- all 64 zeroed by run_typed's hipMemsetAsync before the first
                         launch of every run.
  wide.cpp WideLayout    sync[kBJSyncWords = 512]: words 0..383 (grid counter, abort, parity, sweep
                         flags, smax / cmax, the row-group counters) zeroed by bj_launch's
                         hipMemsetAsync (wide_svd.hip) before block_jacobi_kernel; words 448 / 449
                         (the tridiagonalisation's hand-off counter and abort) zeroed by
                         tri_zero_kernel, the first launch of launch_eig_svd after its Gram product
                         (wide_eig.hip).  colflag[LP]: written 0 for every column by the Cholesky
                         factor kernels (wide_chol.hip) before any pivot is tested.  The wide Grams
                         and projections reduce their slabs in a second launch: no in-kernel wait.
  dense_api.cpp DenseWs  sync and colflag as the wide engine's (launch_block_jacobi, launch_chol).
                PowerGridWs  sync[8]: zeroed by launch_power_grid's hipMemsetAsync (dense.hip);
                         kept: written by workgroup 0 at the end of power_grid_kernel, read after.
  dense_big.cpp SvdBigWs / BigLWs  sync[512]: bj_launch as above, or launch_power_grid_rsvd's
                         hipMemsetAsync of its 8 words; QrBigWs colflag: the Cholesky factor kernels.
Every wait is bounded by a spin count and reports through a sticky flag; a run that raises such a
timeout ends the session here (pytest.exit) instead of starting more GPU work.

Measured on an MI355X, this file alone (46 tests): 16 s.  Per test: every pattern case 0.6 s or less
(most under 0.15 s) except e512n, 4.1 s when its oracle result is not yet cached (test_gpu_ragged.py
computes it earlier in a whole-suite run); the n-shard test 6.4 s, nearly all of it the child's start
(torch import, the RCCL communicator) -- the branch needs that child; stale / queued / stream /
read-only tests under 0.2 s each.

Found with these tests, all three a padding handled by "times zero" and never written, each fixed in
the kernel that owns the buffer (every case then bit-identical on all patterns, no case needed the
determinism fallback):
  * wide_eig.hip tridiag_invit_kernel: the back substitution reads the super-diagonal scratch rows
    U1 / U2 at row n - 1, which the factorisation never wrote, and multiplies them by z = 0.  Under
    NaN every eigenvector came back NaN, the finish kernel's isfinite guard turned that into S = 0
    and a completed U_w: finite, wrong, and no error (f32d, f32f, bLP, eLP, b128v, b128d, b256v,
    e256t, e512n, their option and n-shard variants: every fp32-result run at LP >= 128).
  * dense.hip pjacobi_ref_kernel (SVD<ParallelJacobi>): Jl / Jr written only on d x d; a wide A
    multiplies the whole LP-wide Q panel by Jr (pjacobi-90x400: V NaN).
  * dense.hip power_svd_kernel, rSVD mode: U_p / V_c written only on l x l before the LP-wide panel
    products of the power stage (image-compression-512x384, l = 24 in LP = 32: U NaN; f32d+Power).
Checked that the tests bite: with the `L.mpad > L.m` memset of wide.cpp removed on a scratch copy,
b128v and b256v fail (nan: non-finite singular values raised; big: U differs by 0.7).
"""
import os
import sys

import numpy as np
import pytest

import ragged_cases as rc
from conftest import gapped_matrix
from test_gpu_ragged import _bounds, _check, _dev_A, _dev_omega, _splits
from ws_patterns import PATTERNS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = (("zero", "zero"), ("zero#2", "zero"), ("nan", "nan"), ("big", "big"))

# Cases whose two zero-fill runs differ (an order-dependent reduction): name -> the source.  For
# these alone the poisoned runs are held to the oracle bounds instead of bit identity.
ORDER_DEPENDENT = {}


def _torch():
    import torch

    return torch


# ---- the poisoning primitive ------------------------------------------------------------------------
def _host(res):
    """Host copies of a result tuple (torch tensors or numpy arrays)."""
    return tuple(np.array(x) if isinstance(x, np.ndarray) else x.detach().cpu().numpy() for x in res)


def _first_difference(a, b):
    """None when the tuples are bit-identical (np.array_equal), else (part, index, max |diff|)."""
    for k, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape:
            return k, "shape", float("inf")
        if not np.array_equal(x, y):
            bad = np.flatnonzero(~(x.ravel(order="F") == y.ravel(order="F")))
            with np.errstate(invalid="ignore"):
                d = np.abs(x.astype(np.float64) - y.astype(np.float64))
            return k, int(bad[0]), float(np.max(d))  # (NaN when either side holds one)
    return None


def _guarded_call(call):
    """Run call(); an in-kernel wait that timed out ends the session (nothing more on the GPU)."""
    from rsvd_kamaneh_raganato_terrana_amd._capi import RSVDError

    try:
        return _host(call()), None
    except RSVDError as e:
        if "timed out" in str(e):
            pytest.exit(f"an in-kernel wait timed out on a poisoned workspace: {e}", returncode=3)
        return None, str(e)


def pattern_runs(engine, what, call):
    """One sizing run, then call() over each fill of the WHOLE workspace.  Returns {tag: host result
    or None} and {tag: error text}; prints one line per pattern."""
    torch = _torch()
    call()
    ws = engine.workspace()
    assert ws is not None and ws.is_cuda and ws.dtype == torch.uint8 and ws.numel() > 0
    out, errs = {}, {}
    for tag, pat in RUNS:
        ws.fill_(PATTERNS[pat])
        out[tag], err = _guarded_call(call)
        if err:
            errs[tag] = err
        assert engine.workspace().data_ptr() == ws.data_ptr()  # nothing was reallocated
    report(what, out, errs)
    return out, errs


def report(what, out, errs):
    for tag, _ in RUNS[1:]:
        if out[tag] is None or out["zero"] is None:
            print(f"WS {what} {tag}: raised {errs.get(tag) or errs.get('zero')}")
            continue
        d = _first_difference(out["zero"], out[tag])
        print(f"WS {what} {tag}: " + ("identical" if d is None else
                                      f"differs in part {d[0]} first at flat index {d[1]}, max |diff| {d[2]:.3e}"))


def assert_independent(what, out, errs, oracle_check=None):
    assert not errs, (what, errs)
    assert all(np.isfinite(x).all() for x in out["zero"]), what
    if what in ORDER_DEPENDENT:
        assert oracle_check is not None
        for tag, _ in RUNS:
            oracle_check(out[tag])
        return
    assert _first_difference(out["zero"], out["zero#2"]) is None, (what, "the control: two zero-fill runs differ")
    for tag in ("nan", "big"):
        assert _first_difference(out["zero"], out[tag]) is None, (what, tag)
    if oracle_check is not None:
        oracle_check(out["zero"])


# ---- a. the cases -----------------------------------------------------------------------------------
def _ragged_inputs(cid):
    c = rc.BY_ID[cid]
    stored, scale, _, Om = rc.inputs(cid)
    return c, _dev_A(stored), _dev_omega(Om, c), scale


def _oracle_check(cid):
    torch = _torch()
    return lambda res: _check(cid, *(torch.from_numpy(x) for x in res), what=f"{cid} (workspace)")


def _ragged(cid):
    """The plain rSVD of a ragged case: oracle check and the table's splits."""
    def make(engine):
        c, A, om, scale = _ragged_inputs(cid)

        def call():
            res = engine.rsvd(A, c.l, q=c.q, omega=om, a_scale=scale)
            assert _splits(engine) == c.splits
            return res
        return call, _oracle_check(cid)
    return make


def _ragged_opt(cid, **opts):
    def make(engine):
        c, A, om, scale = _ragged_inputs(cid)
        return (lambda: engine.rsvd(A, c.l, q=c.q, omega=om, a_scale=scale, **opts)), None
    return make


def _range_finder(cid):
    def make(engine):
        c, A, om, _ = _ragged_inputs(cid)

        def check(res):
            Q = res[0].astype(np.float64)
            assert np.linalg.norm(Q.T @ Q - np.eye(c.l)) < _bounds(c)[2]
        return (lambda: (engine.range_finder(A, om, q=c.q),)), check
    return make


def _power_f64(engine):  # test_gpu_power.py test_rsvd_power_matches_oracle[300-200-16-f64]
    torch = _torch()
    from rsvd_kamaneh_raganato_terrana_amd.api import SVDMethod

    At = torch.from_numpy(gapped_matrix(300, 200, 32, decay=0.8, seed=500)).cuda()
    return (lambda: engine.rsvd(At, 16, q=2, method=SVDMethod.Power, seed=4321)), None


def _image_compression(engine):  # rSVD_image_compression's call, test_gpu_power.py's shape
    from rsvd_kamaneh_raganato_terrana_amd import _capi

    A = gapped_matrix(512, 384, 48, decay=0.8, seed=21)
    return (lambda: engine.rsvd_host(A, 24, q=1, method=_capi.SVD_POWER_IC, seed=99)), None


def _host_f64n(engine):
    c = rc.BY_ID["f64n"]
    _, _, A, Om = rc.inputs("f64n")
    return (lambda: engine.rsvd_host(np.array(A), c.l, q=c.q, omega=np.array(Om))), _oracle_check("f64n")


def _host_identity(engine):  # bench.py's C1
    return (lambda: engine.rsvd_host(np.eye(100), 10, q=2, seed=0)), None


def _rng_matrix(m, n, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((m, n)))


def _spectrum_matrix(m, n, sig, seed):  # as test_gpu_dense.py
    rng = np.random.default_rng(seed)
    k = len(sig)
    X = np.linalg.qr(rng.standard_normal((m, k)))[0]
    Y = np.linalg.qr(rng.standard_normal((n, k)))[0]
    return np.asfortranarray((X * sig) @ Y.T)


def _qr(m, n, full, seed, orth=None):
    def make(engine):
        A = _rng_matrix(m, n, seed)

        def check(res):
            Q = res[0]
            assert np.abs(Q.T @ Q - np.eye(Q.shape[1])).max() < orth
        return (lambda: engine.qr_host(A, full=full)), (check if orth else None)
    return make


def _svd(m, n, method, r=0, seed=0, sig=None, mseed=None, orth=None):
    def make(engine):
        k = min(m, n)
        s = (0.97 ** np.arange(k) + 0.01) if sig is None else sig
        A = _spectrum_matrix(m, n, s, seed=m * 7 + n if mseed is None else mseed)

        def check(res):
            for X in (res[0], res[2]):
                assert np.abs(X.T @ X - np.eye(X.shape[1])).max() < orth
        return (lambda: engine.svd_host(A, method, r=r, seed=seed)), (check if orth else None)
    return make


def _big_rsvd(engine):
    """Past 512 sketch columns (driver.cpp rsvd_run: d->l > 512 -> dense_big.cpp big_rsvd_run): l = 513,
    fp32 A, q = 1.  Orthonormality at test_gpu_big_l.py's fp32 bound, 1e-3 l / 512 (Frobenius)."""
    torch = _torch()
    m, n, l = 700, 600, 513
    A = torch.from_numpy(np.ascontiguousarray(gapped_matrix(m, n, 600, decay=0.99, seed=513).T)).float().cuda().t()

    def check(res):
        for X in (res[0].astype(np.float64), res[2].astype(np.float64)):
            assert np.linalg.norm(X.T @ X - np.eye(l)) < 1e-3 * l / 512
    return (lambda: engine.rsvd(A, l, q=1, seed=514)), check


def _dense_case(cid):
    """A row of tests/dense_cases.py on the device path (Engine.qr / Engine.svd, the row's storage
    dtype), held to test_gpu_dense_ragged.py's reference check."""
    def make(engine):
        import dense_cases as dc
        from test_gpu_dense_ragged import _check_qr, _check_svd, _dev_A, _run

        c = dc.BY_ID[cid]
        A, _ = _dev_A(c, dc.inputs(cid))
        check = _check_qr if c.op in ("qr", "qrfull") else _check_svd
        return (lambda: _run(engine, c, A)), (lambda res: check(c, *(x.astype(np.float64) for x in res)))
    return make


def _methods():
    from rsvd_kamaneh_raganato_terrana_amd.api import QRMode, SVDMethod

    return QRMode, SVDMethod


def _cases():
    QRMode, SVDMethod = _methods()
    cases = [(cid, _ragged(cid)) for cid in (
        "f32a", "f32b", "f64n",                                    # narrow engine (driver.cpp)
        "f32d", "f32f", "f64a",                                    # wide fp engine
        "bLP", "eLP", "b128v", "b128d", "b256v", "e256t", "e512n", "b32", "e16")]  # wide low precision
    cases += [
        ("b256v+lowp_intermediates", _ragged_opt("b256v", lowp_intermediates=True)),
        ("f32b+GS2", _ragged_opt("f32b", qr_mode=QRMode.GS2)),
        ("f32b+CholQR2", _ragged_opt("f32b", qr_mode=QRMode.CholQR2)),
        ("f32d+ParallelJacobi", _ragged_opt("f32d", method=SVDMethod.ParallelJacobi)),
        ("power-f64-300x200", _power_f64),                         # (l = LP = 16: no padding)
        ("f32d+Power", _ragged_opt("f32d", method=SVDMethod.Power)),  # the power stage with l = 65 in LP = 128
        ("image-compression-512x384", _image_compression),
        ("b128v+range_finder", _range_finder("b128v")),
        ("f64a+range_finder", _range_finder("f64a")),
        ("host-f64n", _host_f64n),
        ("host-identity-c1", _host_identity),
        # dense drop-ins at test_gpu_dense.py's shapes
        ("qr-reduced-300x40", _qr(300, 40, False, 340)),
        ("qr-full-96x30", _qr(96, 30, True, 3)),
        ("qr-full-wide-40x70", _qr(40, 70, True, 4)),
        ("jacobi-200x50", _svd(200, 50, 0)),                       # one workgroup (LP <= 64)
        ("jacobi-300x150", _svd(300, 150, 0)),                     # block Jacobi
        ("pjacobi-90x400", _svd(90, 400, 2)),
        ("power-60x40-r0", _svd(60, 40, 1, r=0, seed=77, sig=2.0 * 0.75 ** np.arange(40), mseed=60 + 3 * 40)),
        ("gridpower-700x600-r8", _svd(700, 600, 1, r=8, seed=31, sig=2.0 * 0.7 ** np.arange(40), mseed=1300)),
        # past 512 columns (dense_big.cpp), the smallest shapes the dispatch sends there:
        # rsvd_qr: max(Q columns, n) > 512; rsvd_svd Jacobi: min(m, n) > 512 (dense_api.cpp); rsvd_run: l > 512
        ("big-qr-600x513", _qr(600, 513, False, 600 * 3 + 513, orth=1e-12)),
        ("big-jacobi-600x513", _svd(600, 513, 0, sig=0.99 ** np.arange(513), mseed=600 + 2 * 513, orth=1e-12)),
        ("big-rsvd-700x600-l513", _big_rsvd),
        # padding columns inside LP that had not yet run under the 0xFF fill (tests/dense_cases.py)
        ("dense-power-90x70", _dense_case("power-f64-90x70-r8")),         # LP 80: gram_wide's half-empty block
        ("dense-jacobi-131x65", _dense_case("jacobi-f64-131x65")),        # LP 96
        ("dense-jacobi-65x131-f32", _dense_case("jacobi-f32-65x131")),    # LP 96, transpose_to_panel<float>
        ("dense-qr-517x513-f32", _dense_case("qr-f32-517x513")),          # a one-column block in LP 512
    ]
    return cases


CASES = _cases()


@pytest.mark.parametrize("what,make", CASES, ids=[c[0] for c in CASES])
def test_results_do_not_depend_on_workspace(engine, what, make):
    call, check = make(engine)
    out, errs = pattern_runs(engine, what, call)
    assert_independent(what, out, errs, check)


def _nshard_worker(q):
    """comm_init(uid, 0, 1) then force_nshard=True, as test_gpu_rccl.py's library mode; the pattern
    runs happen here and the host results go back."""
    try:
        sys.path.insert(0, REPO)
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import torch

        import rsvd_kamaneh_raganato_terrana_amd as R

        torch.cuda.set_device(0)
        c, A, om, scale = _ragged_inputs("b128v")
        eng = R.Engine(0)
        eng.comm_init(R.Engine.comm_unique_id(), 0, 1, shard_n=True)
        rows = []

        def call():
            res = eng.rsvd(A, c.l, q=c.q, omega=om, a_scale=scale, force_nshard=True)
            rows.append(eng.info()["n_shard_rows"])
            return res
        out, errs = pattern_runs(eng, "b128v+nshard", call)
        eng.comm_destroy()
        eng.close()
        q.put((True, (out, errs, rows)))
    except BaseException:
        import traceback

        q.put((False, traceback.format_exc()))


def test_nshard_layout_does_not_depend_on_workspace():
    """The rows past n of the sharded n-side panels (wide.cpp: nfull > n) at world 1: n = 702 gives
    nc = nfull = 704.  Two processes hold the GPU: this one and the child."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nshard_worker, args=(q,))
    p.start()
    ok, res = q.get(timeout=300)
    p.join(timeout=60)
    if not ok and "timed out" in res:
        pytest.exit(f"an in-kernel wait timed out in the n-shard child: {res}", returncode=3)
    assert ok, res
    out, errs, rows = res
    report("b128v+nshard", out, errs)
    assert rows and all(r == 704 for r in rows), rows
    assert_independent("b128v+nshard", out, errs, _oracle_check("b128v"))


# ---- b. stale data of real runs ---------------------------------------------------------------------
def test_stale_data_of_real_runs():
    """Every workspace region re-partitioned over live data of another dtype and LP."""
    import rsvd_kamaneh_raganato_terrana_amd as R

    order = ["e512n", "f32a", "bLP", "e512n"]
    calls, fresh = {}, {}
    for cid in sorted(set(order)):
        c, A, om, scale = _ragged_inputs(cid)
        calls[cid] = lambda e, c=c, A=A, om=om, scale=scale: e.rsvd(A, c.l, q=c.q, omega=om, a_scale=scale)
        eng = R.Engine(0)
        try:
            fresh[cid] = _host(calls[cid](eng))
        finally:
            eng.close()
    eng = R.Engine(0)
    try:
        got = [(cid, _host(calls[cid](eng))) for cid in order]
    finally:
        eng.close()
    diffs = [(cid, _first_difference(fresh[cid], res)) for cid, res in got]
    for k, (cid, d) in enumerate(diffs):
        print(f"WS stale run {k} {cid}: " + ("identical" if d is None else f"differs {d}"))
    assert all(d is None for _, d in diffs), diffs


# ---- c. queued runs ---------------------------------------------------------------------------------
def test_queued_runs(engine):
    order = ["b256v", "f32b", "e256t", "b256v"]
    inp = {cid: _ragged_inputs(cid) for cid in set(order)}

    def run(cid, **kw):
        c, A, om, scale = inp[cid]
        return engine.rsvd(A, c.l, q=c.q, omega=om, a_scale=scale, **kw)
    for cid in inp:  # the largest of the three first: nothing is reallocated while work is queued
        c, A, _, scale = inp[cid]
        engine.reserve(engine.desc(A, c.l, c.q, a_scale=scale))
    sync_res = {cid: _host(run(cid)) for cid in inp}
    ws = engine.workspace().data_ptr()
    queued = [(cid, run(cid, check_errors=False)) for cid in order]
    assert engine.workspace().data_ptr() == ws
    engine.sync()
    assert _splits(engine) == rc.BY_ID[order[-1]].splits
    diffs = [(cid, _first_difference(sync_res[cid], _host(res))) for cid, res in queued]
    for k, (cid, d) in enumerate(diffs):
        print(f"WS queued run {k} {cid}: " + ("identical" if d is None else f"differs {d}"))
    assert all(d is None for _, d in diffs), diffs


def test_queued_calls_across_entry_points(engine):
    """rsvd_batched, compress_batched, pod and lowrank share the handle's workspace (panel slices, POD's
    regions with a nested solver in the tail, low-rank slots) and need very different amounts of it.  Queued
    on one handle with nothing between them -- every input already on the device in the layout the call takes,
    so no call copies or waits -- each must return the bits of the same call made alone, whatever the
    workspace held before."""
    torch = _torch()
    import batched_cases as bc
    import test_gpu_batched as TB
    import test_gpu_lowrank as TL
    import test_gpu_pod as TP

    def batch(m, n, l, f32):
        A = TB._dev_batch([TB._matrix(m, n, l, b, f32) for b in range(2)], f32)
        om = torch.from_numpy(np.stack([TB._omega(n, l, b, f32) for b in range(2)])).to(TB._tdt(f32)).cuda()
        return A, om.transpose(1, 2).contiguous().transpose(1, 2)

    A1, om1 = batch(150, 125, 48, False)
    assert bc.placement(150, 125, 48, 1, False) == ("f64", 48, "ws")
    A2, om2 = batch(90, 50, 33, True)
    nh, ns, r = 1037, 37, 12
    Sp = TP._dev(TP._snap(nh, ns, False), False)
    csr = tuple(torch.from_numpy(x).cuda() for x in TP._tridiag_csr(nh))
    dw = torch.from_numpy(TP._weights(ns)).cuda()
    Uh, Sh, Vh, Ah = TL._inputs(130, 67, TL.D, False)
    U, V, A4 = (TL._colmajor(X, torch.float64) for X in (Uh, Vh, Ah))
    S4 = torch.from_numpy(np.array(Sh)).cuda()
    calls = [
        ("rsvd_batched", lambda: engine.rsvd_batched(A1, 48, q=1, omega=om1, check_errors=False)),
        ("compress_batched", lambda: engine.compress_batched(A2, 33, k=17, q=2, omega=om2, check_errors=False)),
        ("pod", lambda: engine.pod(Sp, r, TP.TOL, Xh=csr, d=dw, svd_type=4, q=2, seed=TP.SEED, truncate=False,
                                   return_corr=True)),
        ("lowrank", lambda: engine.lowrank(U, S4, V, k=37, A=A4)),
    ]
    calls.append(calls[0])
    alone = []
    for _, call in calls[:4]:
        torch.cuda.synchronize()
        res = call()
        torch.cuda.synchronize()
        engine.sync()
        alone.append(_host(res))
    alone.append(alone[0])
    assert all(np.isfinite(x).all() for res in alone for x in res)
    ws = engine.workspace()
    for fill in [None] + list(PATTERNS):
        if fill is not None:
            ws.fill_(PATTERNS[fill])
            torch.cuda.synchronize()
        queued = [call() for _, call in calls]
        assert engine.workspace().data_ptr() == ws.data_ptr()  # nothing was reallocated while work was queued
        engine.sync()
        diffs = [(name, _first_difference(ref, _host(res))) for (name, _), ref, res in zip(calls, alone, queued)]
        for k, (name, d) in enumerate(diffs):
            print(f"WS queued entry points, fill {fill}, call {k} {name}: " +
                  ("identical" if d is None else f"differs {d}"))
        assert all(d is None for _, d in diffs), (fill, diffs)


# ---- d. a non-default stream --------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["b128v", "f64a"])
def test_non_default_stream(engine, cid):
    torch = _torch()
    c, A, om, scale = _ragged_inputs(cid)
    ref = _host(engine.rsvd(A, c.l, q=c.q, omega=om, a_scale=scale))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res = engine.rsvd(A, c.l, q=c.q, omega=om, a_scale=scale)
        s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    d = _first_difference(ref, _host(res))
    print(f"WS stream {cid}: " + ("identical" if d is None else f"differs {d}"))
    assert d is None, d
    engine.rsvd(A, c.l, q=c.q, omega=om, a_scale=scale)  # (the handle back on the default stream)


# ---- e. inputs are read-only --------------------------------------------------------------------------
class _Guarded:
    """A copy of a rows x cols device matrix, column-major with leading dimension rows + pad, inside a
    byte buffer prefilled with 0xA5: pad elements after every column, one guard column before and
    one after.  With (rows + pad) * element size a multiple of 16 the base stays 16-byte aligned."""

    def __init__(self, src, pad):
        torch = _torch()
        rows, cols = src.shape
        esz, ld = src.element_size(), rows + pad
        self.raw = torch.full(((cols + 2) * ld * esz,), 0xA5, dtype=torch.uint8, device="cuda")
        self.raw.view(cols + 2, ld * esz)[1:cols + 1, :rows * esz] = src.t().contiguous().view(torch.uint8)
        self.mat = self.raw.view(src.dtype).view(cols + 2, ld)[1:cols + 1, :rows].t()
        assert self.mat.stride() == (1, ld) and self.mat.shape == src.shape
        self.before = self.raw.clone()

    def unchanged(self):
        return bool(_torch().equal(self.raw, self.before))


@pytest.mark.parametrize("cid", ["b128v", "e256n", "f32b", "f64a"])
def test_inputs_are_read_only(engine, cid):
    torch = _torch()
    from rsvd_kamaneh_raganato_terrana_amd.api import colmajor

    c, A, om, scale = _ragged_inputs(cid)
    # lda = m + 8 (bf16) / m + 16 (e4m3): pitch and base stay on the 16-byte chunk, the LDS-DMA kernels are kept
    Ag = _Guarded(A, {"bf16": 8, "e4m3": 16}.get(c.dtype, 1))
    Og = _Guarded(om, 1)
    if c.dtype in ("bf16", "e4m3"):
        assert Ag.mat.data_ptr() % 16 == 0 and (Ag.mat.stride(1) * Ag.mat.element_size()) % 16 == 0
    assert colmajor(Ag.mat)[0].data_ptr() == Ag.mat.data_ptr()  # the views themselves reach the engine
    assert colmajor(Og.mat)[0].data_ptr() == Og.mat.data_ptr() and Og.mat.dtype == engine.out_dtype(A.dtype)
    res = engine.rsvd(Ag.mat, c.l, q=c.q, omega=Og.mat, a_scale=scale)
    torch.cuda.synchronize()
    assert _splits(engine) == c.splits
    print(f"WS read-only {cid}: A unchanged {Ag.unchanged()}, Omega unchanged {Og.unchanged()}")
    assert Ag.unchanged() and Og.unchanged()
    assert all(np.isfinite(x).all() for x in _host(res))
