"""CPU: the batched rSVD's C ABI (rsvd_run_batched, rsvd_batched_workspace_bytes,
rsvd_batched_is_fused; include/rsvd_c.h ABI 7) -- exports, the host-only planning calls and their
status codes, and the Python argument checks that run before any device call."""
import ctypes
import subprocess

import pytest

import rsvd_kamaneh_raganato_terrana_amd as R
from rsvd_kamaneh_raganato_terrana_amd import _capi

INVALID, UNSUPPORTED = 1, 2
NEW = ("rsvd_run_batched", "rsvd_batched_workspace_bytes", "rsvd_batched_is_fused")


@pytest.fixture(scope="module")
def lib():
    R.build(force=False)
    return _capi.lib()


def _desc(m, n, l, dtype, **kw):
    d = dict(m=m, n=n, lda=m, l=l, q=2, dtype=dtype, method=_capi.SVD_JACOBI, qr_mode=_capi.QR_AUTO, flags=0, seed=0,
             a_scale=1.0)
    d.update(kw)
    return _capi.Desc(**d)


def _batch(d, count=4, **kw):
    b = dict(count0=count, count1=1, a_stride0=d.lda * d.n, a_stride1=0, omega_stride=0, u_stride=d.m * d.l,
             s_stride=d.l, v_stride=d.n * d.l)
    b.update(kw)
    return _capi.BatchDesc(**b)


def _ws(lib, d, b):
    nb = ctypes.c_size_t(0)
    return lib.rsvd_batched_workspace_bytes(ctypes.byref(d), ctypes.byref(b), ctypes.byref(nb)), nb.value


def _fused(lib, d, b=None):
    b = b or _batch(d)
    return lib.rsvd_batched_is_fused(ctypes.byref(d), ctypes.byref(b))


def test_batch_desc_is_eight_int64():
    assert ctypes.sizeof(_capi.BatchDesc) == 8 * 8


def test_library_exports_the_batched_symbols(lib):
    assert set(NEW) <= set(_capi.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NEW) <= exported
    assert lib.rsvd_abi_version() >= 7


@pytest.mark.parametrize("m,n,l,dtype", [(256, 256, 64, _capi.F64), (16, 16, 16, _capi.F32), (17, 200, 16, _capi.F64)])
def test_inside_the_fused_limits(lib, m, n, l, dtype):
    d = _desc(m, n, l, dtype)
    assert _fused(lib, d) == 1
    st, nb = _ws(lib, d, _batch(d))
    assert st == 0 and nb > 0


@pytest.mark.parametrize("m,n,l,dtype,kw", [
    (257, 64, 8, _capi.F64, {}),
    (128, 128, 65, _capi.F32, {}),
    (128, 96, 16, _capi.BF16, {}),
    (64, 64, 8, _capi.F64, dict(qr_mode=_capi.QR_GS2)),
])
def test_outside_the_fused_limits_loops(lib, m, n, l, dtype, kw):
    d = _desc(m, n, l, dtype, **kw)
    assert _fused(lib, d) == 0
    st, nb = _ws(lib, d, _batch(d))
    assert st == 0 and nb > 0
    one = ctypes.c_size_t(0)  # the loop needs what one rsvd_run needs
    assert lib.rsvd_workspace_bytes(ctypes.byref(d), ctypes.byref(one)) == 0
    assert nb == one.value


def test_tile_grid_description(lib):
    """32 x 32 tiles of 128 x 128 inside a 4096 x 4096 column-major matrix: overlapping strides are fine."""
    d = _desc(128, 128, 16, _capi.F32, lda=4096)
    b = _batch(d, count0=32, count1=32, a_stride0=128, a_stride1=128 * 4096)
    assert _fused(lib, d, b) == 1
    assert _ws(lib, d, b)[0] == 0


@pytest.mark.parametrize("bad", [
    dict(count0=0), dict(count1=0), dict(count0=-3),
    dict(a_stride0=-1), dict(a_stride1=-1), dict(omega_stride=-1), dict(u_stride=-1), dict(s_stride=-1),
    dict(v_stride=-1),
    dict(u_stride=70 * 8 - 1), dict(s_stride=7), dict(v_stride=45 * 8 - 1),
])
def test_bad_batch_arguments(lib, bad):
    d = _desc(70, 45, 8, _capi.F64)
    assert _ws(lib, d, _batch(d))[0] == 0
    assert _ws(lib, d, _batch(d, **bad))[0] == INVALID, bad
    assert _fused(lib, d, _batch(d, **bad)) == 0


def test_bad_descriptions(lib):
    d = _desc(70, 45, 8, _capi.F64, flags=_capi.FLAG_LOWP_INTERMEDIATES)
    assert _ws(lib, d, _batch(d))[0] == INVALID
    for method in (_capi.SVD_POWER, _capi.SVD_POWER_IC):
        d = _desc(70, 45, 8, _capi.F64, method=method)
        assert _ws(lib, d, _batch(d))[0] == UNSUPPORTED
        assert _fused(lib, d) == 0
    d = _desc(70, 45, 8, _capi.F64, lda=69)  # the single-matrix checks still apply
    assert _ws(lib, d, _batch(d))[0] == INVALID
    d = _desc(70, 45, 8, _capi.F64)
    assert lib.rsvd_batched_workspace_bytes(ctypes.byref(d), ctypes.byref(_batch(d)), None) == INVALID


def test_run_batched_refuses_a_null_handle(lib):
    d = _desc(70, 45, 8, _capi.F64)
    assert lib.rsvd_run_batched(None, ctypes.byref(d), ctypes.byref(_batch(d)), None, None, 0, None, 70, None, None, 45,
                                None) == INVALID


def test_rsvd_tiles_refuses_a_tile_that_does_not_divide():
    """Checked on a CPU tensor, before any device call (no handle is needed to get this far)."""
    import torch

    A = torch.zeros((111, 58), dtype=torch.float32).t().contiguous().t()
    eng = object.__new__(R.Engine)
    for tm, tn in ((36, 29), (37, 30), (0, 29)):
        with pytest.raises(ValueError):
            eng.rsvd_tiles(A, tm, tn, 6)
