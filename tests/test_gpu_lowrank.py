"""GPU: Engine.lowrank -> rsvd_lowrank (csrc/lowrank.hip) on its own, away from the rSVD that usually feeds it.

The factors are not singular vectors here: U (m x d), S (d, positive) and V (n x d) come from a seeded numpy
generator with d = 40, and A is an independent Gaussian matrix, so nothing is small by construction and every
K slice carries weight.  The reference is (U[:, :k] * S[:k]) @ V[:, :k].T in float64 on the host from the
values as stored (rounded to fp32 first in the fp32 cases).

Bars, the ones tests/test_gpu_compress.py already holds the same quantities to:
  C against the host product   rel_fro < 1e-12 (fp64), < 1e-5 (fp32)       test_lowrank_alone
  error words                  _check_err_words, rtol 1e-10 max(1, m n / 65536)   test_lowrank_alone
  a_scale                      err[0] scales by a_scale^2 to 1e-12 relative        test_a_scale

What each case is there for (lowrank_kernel walks K in slices of 16 with two barriers per slice; one
64 x 64 tile per workgroup; lowrank_err_kernel sums the tiles' slots, thread t taking t, t + 256, ..):
  K loop   k = 3 (a partial single slice), 16 (an exact slice), 17 (a second slice of one column: the
           refill of Us / Vs), 37 (three slices, k % 4 != 0), 40 (a partial last slice, a multiple of 4);
           U and V at pitches m + 3 and n + 5 from a base one element into their buffers, C in a guarded
           buffer whose padding has to stay as it was
  tiles    16385 x 1 and 3 x 16385 (257 tiles along either grid axis: the second round of the slot sum),
           200 x 16385 (4 x 257: the slot index with both block indices non-zero)
  e4m3 A   every finite code, decoded on the host from the format's definition
  a_scale  on the stand-alone call

Measured on an MI355X: C against the host product 0 (fp64: the k sum runs in the same order) and 4.5e-8 ..
1.2e-7 (fp32); each case well under a second.  Checked that the tests bite, on a scratch build with three
in-bounds changes to lowrank.hip (the refill of Us reading column kk instead of k0 + kk, subnormal e4m3 codes
decoded as m 2^-10, the slot sum stopping after 256 slots): k = 17, 37, 40, the three tile cases and both e4m3
cases fail, k = 3 and 16 pass -- as does every lowrank test of tests/test_gpu_compress.py.
"""
import functools

import numpy as np
import pytest

from conftest import rel_fro
from padded import _Padded
from test_gpu_compress import _check_err_words

gpu = pytest.mark.gpu
D = 40


def _torch():
    import torch

    return torch


def _tdt(f32):
    torch = _torch()
    return torch.float32 if f32 else torch.float64


def _round(X, f32):
    return X.astype(np.float32).astype(np.float64) if f32 else X


@functools.lru_cache(maxsize=None)
def _inputs(m, n, d, f32):
    """U, S, V and A as the device will hold them, in float64 and read-only."""
    rng = np.random.default_rng(1000 * m + n + d)
    out = (_round(rng.standard_normal((m, d)), f32), _round(rng.uniform(0.5, 2.0, d), f32),
           _round(rng.standard_normal((n, d)), f32), _round(rng.standard_normal((m, n)), f32))
    for x in out:
        x.setflags(write=False)
    return out


def _pitched(X, pad, dt):
    """X on the device, column-major at pitch rows + pad, its base one element into the buffer."""
    torch = _torch()
    rows, cols = X.shape
    ld = rows + pad
    buf = torch.zeros(1 + cols * ld, dtype=dt, device="cuda")
    view = buf[1:].view(cols, ld)[:, :rows].t()
    view.copy_(torch.from_numpy(np.array(X)))
    assert view.stride() == (1, ld) and view.data_ptr() == buf.data_ptr() + buf.element_size()
    return view


def _colmajor(X, dt):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(np.array(X).T)).to(dt).cuda().t()


def _np(t):
    return t.cpu().double().numpy()


def _rtol(m, n):
    return 1e-10 * max(1.0, m * n / 65536)  # test_lowrank_alone's


# ---- 1. the K loop ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [3, 16, 17, 37, 40])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_k_loop(engine, f32, k):
    torch = _torch()
    from rsvd_kamaneh_raganato_terrana_amd.api import colmajor

    m, n, dt = 130, 67, _tdt(f32)
    Uh, Sh, Vh, Ah = _inputs(m, n, D, f32)
    U, V = _pitched(Uh, 3, dt), _pitched(Vh, 5, dt)
    assert colmajor(U)[0].data_ptr() == U.data_ptr() and colmajor(V)[0].data_ptr() == V.data_ptr()  # the views go in
    S, A = torch.from_numpy(np.array(Sh)).to(dt).cuda(), _colmajor(Ah, dt)
    P = _Padded(m, n, m + 3, dt)
    C, err = engine.lowrank(U, S, V, k=k, A=A, out=P.mat)
    torch.cuda.synchronize()
    assert C.data_ptr() == P.mat.data_ptr() and P.padding_untouched() and bool(torch.isfinite(P.mat).all())
    Ch = _np(C)
    ec = rel_fro(Ch, (Uh[:, :k] * Sh[:k]) @ Vh[:, :k].T)
    print(f"LOWRANK k-loop {m}x{n} {'f32' if f32 else 'f64'} k{k}: against the host product {ec:.2e}")
    assert ec < (1e-5 if f32 else 1e-12), (k, ec)
    _check_err_words(f"k-loop k{k}", _np(err), Ah, Ch, rtol=_rtol(m, n))
    assert torch.equal(engine.lowrank(U, S, V, k=k), C)  # without A: the same C


# ---- 2. more than 256 tiles -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("m,n", [(16385, 1), (3, 16385), (200, 16385)])
def test_more_than_256_tiles(engine, m, n):
    torch = _torch()
    d = 5
    Uh, Sh, Vh, Ah = _inputs(m, n, d, True)
    U, V, A = _colmajor(Uh, torch.float32), _colmajor(Vh, torch.float32), _colmajor(Ah, torch.float32)
    S = torch.from_numpy(np.array(Sh)).float().cuda()
    assert -(-m // 64) * -(-n // 64) > 256
    C, err = engine.lowrank(U, S, V, k=d, A=A)
    torch.cuda.synchronize()
    Ch = _np(C)
    ec = rel_fro(Ch, (Uh * Sh) @ Vh.T)
    print(f"LOWRANK tiles {m}x{n}: against the host product {ec:.2e}")
    assert ec < 1e-5, ec
    _check_err_words(f"tiles {m}x{n}", _np(err), Ah, Ch, rtol=_rtol(m, n))
    assert torch.equal(engine.lowrank(U, S, V, k=d, A=A, out=False), err)  # C = NULL: the same words


# ---- 3. e4m3 A ----------------------------------------------------------------------------------------------
def _e4m3_value(b):
    """OCP e4m3fn from its definition: 1 sign bit, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 is
    subnormal, m 2^-9; S.1111.111 is the one NaN and there is no infinity."""
    e, mt = (b >> 3) & 15, b & 7
    if e == 15 and mt == 7:
        v = float("nan")
    elif e == 0:
        v = mt * 2.0 ** -9
    else:
        v = (1.0 + mt / 8.0) * 2.0 ** (e - 7)
    return -v if b & 0x80 else v


FINITE_CODES = [b for b in range(256) if b not in (0x7F, 0xFF)]


def test_e4m3_decode_agrees_with_torch():
    """The host decode of the e4m3 case, against torch's own conversion of all 256 codes (CPU)."""
    torch = _torch()
    mine = np.array([_e4m3_value(b) for b in range(256)])
    theirs = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).double().numpy()
    assert np.array_equal(np.isnan(mine), np.isnan(theirs)) and int(np.isnan(mine).sum()) == 2
    ok = ~np.isnan(mine)
    assert np.array_equal(mine[ok], theirs[ok]) and np.array_equal(np.signbit(mine[ok]), np.signbit(theirs[ok]))
    assert len(FINITE_CODES) == 254 and max(abs(_e4m3_value(b)) for b in FINITE_CODES) == 448.0


@gpu
@pytest.mark.parametrize("a_scale", [1.0, -0.375])
def test_e4m3_a(engine, a_scale):
    torch = _torch()
    m, n, k = 70, 67, 17
    Uh, Sh, Vh, _ = _inputs(m, n, D, True)
    codes = np.resize(np.array(FINITE_CODES, dtype=np.uint8), m * n)  # the 254 finite codes, cyclically, column by column
    Ah = np.array([_e4m3_value(int(b)) for b in codes]).reshape(n, m).T
    assert len(set(codes.tolist())) == 254 and np.all(np.isfinite(Ah))
    A = torch.from_numpy(codes.reshape(n, m)).cuda().view(torch.float8_e4m3fn).t()
    assert A.shape == (m, n) and A.stride() == (1, m)
    U, V = _colmajor(Uh, torch.float32), _colmajor(Vh, torch.float32)
    S = torch.from_numpy(np.array(Sh)).float().cuda()
    C, err = engine.lowrank(U, S, V, k=k, A=A, a_scale=a_scale)
    torch.cuda.synchronize()
    Ch = _np(C)
    ec = rel_fro(Ch, (Uh[:, :k] * Sh[:k]) @ Vh[:, :k].T)
    print(f"LOWRANK e4m3 a_scale {a_scale}: against the host product {ec:.2e}")
    assert ec < 1e-5, ec
    _check_err_words(f"e4m3 a_scale {a_scale}", _np(err), a_scale * Ah, Ch, rtol=_rtol(m, n))  # -0.375 a is exact


# ---- 4. a_scale on the stand-alone call ---------------------------------------------------------------------
@gpu
def test_a_scale(engine):
    torch = _torch()
    m, n, k, a_scale = 130, 67, 17, -2.5
    Uh, Sh, Vh, Ah = _inputs(m, n, D, False)
    U, V, A = (_colmajor(X, torch.float64) for X in (Uh, Vh, Ah))
    S = torch.from_numpy(np.array(Sh)).cuda()
    C, err = engine.lowrank(U, S, V, k=k, A=A)
    C2, err2 = engine.lowrank(U, S, V, k=k, A=A, a_scale=a_scale)
    torch.cuda.synchronize()
    assert torch.equal(C2, C)  # a_scale belongs to A: C is the factors' product either way
    assert rel_fro(_np(C), (Uh[:, :k] * Sh[:k]) @ Vh[:, :k].T) < 1e-12
    e, e2 = _np(err), _np(err2)
    assert abs(e2[0] - 6.25 * e[0]) <= 1e-12 * 6.25 * e[0], (e2[0], e[0])
    _check_err_words("a_scale -2.5", e2, a_scale * Ah, _np(C2), rtol=_rtol(m, n))
    _check_err_words("a_scale 1", e, Ah, _np(C), rtol=_rtol(m, n))
