"""Python host mirror of the reference's rSVD interface, running on the MI355X engine.

Reference signatures mirrored (AMSC22-23/rSVD_Kamaneh_Raganato_Terrana):

* ``rSVD(A, l, method=SVDMethod.Jacobi)`` -> ``(U, S, V)``
      void rSVD(Mat_m& A, Mat_m& U, Vec_v& S, Mat_m& V, int l, SVDMethod)  include/rSVD.hpp:14
* ``intermediate_step(A, Omega, l, q)`` -> ``Q``
      void intermediate_step(const Mat_m&, Mat_m& Q, const Mat_m& Omega, int l, int q)  :13
* ``generateOmega(n, l)`` -> ``Omega``                    Mat_m generateOmega(int, int)  :15
* ``SVDMethod`` (Jacobi, Power, ParallelJacobi)           include/SVD_class.hpp:28-32

numpy float64 inputs take the synchronous fp64 host path (the drop-in the reference's Eigen
callers see); torch CUDA tensors (float64 / float32 / bfloat16 / float8_e4m3fn) take the
asynchronous device path on the current torch stream, with A resident in HBM (bf16 / fp8 A return
fp32 U, S, V; fp8 A carries a per-tensor scale, A = a_scale * stored).  There is no CPU fallback: without the HIP
library or a GPU these functions raise.
"""
from __future__ import annotations

import ctypes
import enum
from typing import Optional

import numpy as np

from . import _capi
from ._capi import Desc, Info, Timing, check, lib


class SVDMethod(enum.IntEnum):
    Jacobi = 0
    Power = 1
    ParallelJacobi = 2


class QRMode(enum.IntEnum):
    Auto = 0      # CholeskyQR(2) + predicated CGS2 fallback
    GS2 = 1       # always CGS2 (robust, slow: one workgroup)
    CholQR2 = 2   # two CholeskyQR passes on every panel


def _dp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _torch():
    import torch  # plumbing only: device memory, streams, torch.distributed

    return torch


def colmajor(t):
    """A column-major (Fortran-order) view/copy of a 2-D torch tensor and its leading dim."""
    if t.dim() != 2:
        raise ValueError("expected a matrix")
    if t.stride(0) == 1 and t.stride(1) >= max(1, t.shape[0]):
        return t, t.stride(1)
    c = t.t().contiguous().t()
    return c, max(1, c.shape[0])


def empty_colmajor(rows: int, cols: int, dtype, device, pad: int = 0):
    """An uninitialised column-major rows x cols matrix; pad > 0 gives it the leading dimension
    rows + pad.  For a tall A whose row count is a large power of two, a pad of 64 elements keeps the
    columns of one k-step off a common HBM address pattern: C3's A^T Q 0.66 -> 0.54 ms per launch
    (profiles/r06_ldapad_ab.txt; no effect at C4 / C5).  Eigen callers pass lda = m."""
    torch = _torch()
    buf = torch.empty((cols, rows + max(0, pad)), dtype=dtype, device=device)
    return buf[:, :rows].t()


def make_allreduce_hook(get_buffer, group=None):
    """The C ABI's rsvd_allreduce_fn (include/rsvd_c.h) over torch.distributed.

    The engine only ever exchanges slices of its workspace (the Gram matrix of a CholeskyQR pass
    and the n x l panel Z = A^T Q); ``get_buffer()`` returns that workspace as a
    uint8 tensor and the hook sums the (pointer, count, dtype) slice in place across ranks.  It
    returns non-zero (never raises through C) for a slice outside the buffer or a failed
    collective.  With a CUDA workspace and the "nccl" backend this is an RCCL all-reduce over
    xGMI; with a CPU buffer and "gloo" it is the same code path the CPU tests exercise.
    """
    torch = _torch()
    import torch.distributed as dist

    def _hook(buf, count, dtype, stream, user):
        try:
            ws = get_buffer()
            if ws is None or buf is None:
                return 1
            base = ws.data_ptr()
            tdt = torch.float64 if dtype == _capi.F64 else torch.float32
            esz = 8 if dtype == _capi.F64 else 4
            off = buf - base
            if count < 0 or off < 0 or off % esz or off + count * esz > ws.numel():
                return 1
            view = ws[off: off + count * esz].view(tdt)
            dist.all_reduce(view, op=dist.ReduceOp.SUM, group=group)
            return 0
        except Exception:  # never unwind through C
            return 1

    return _capi.ALLREDUCE_FN(_hook)


def make_collective_hook(get_buffer, group=None):
    """The C ABI's rsvd_collective_fn (include/rsvd_c.h, ABI 5) over torch.distributed: the
    reduce-scatter of A^T Q and the all-gathers of the next skinny operand and of V that the
    n-side sharding needs.  Like the all-reduce hook it only ever touches
    slices of the handle's workspace and returns non-zero instead of raising through C.  RCCL
    ("nccl") and gloo on CPU buffers run reduce_scatter_tensor / all_gather_into_tensor, in place
    when the engine aliases recv = send + rank count (RS) or send = recv + rank count (AG) -- so the
    CPU gloo tests run the very branch RCCL runs.  gloo on CUDA buffers (two ranks sharing one GPU
    in the GPU tests) lacks those and gets the same result from one all_reduce (reduce-scatter: sum
    everything, keep this rank's chunk; all-gather: zero the other chunks, sum)."""
    torch = _torch()
    import torch.distributed as dist

    sizes = {_capi.F64: (torch.float64, 8), _capi.F32: (torch.float32, 4), _capi.BF16: (torch.bfloat16, 2)}
    # the tensor collectives (RCCL, and gloo on CPU tensors -- so the CPU tests run this same
    # branch, in-place aliasing included); gloo on CUDA tensors has only all_reduce
    legacy = {}

    def _hook(op, send, recv, count, dtype, stream, user):
        try:
            ws = get_buffer()
            if ws is None or send is None or recv is None or dtype not in sizes or count < 0:
                return 1
            tdt, esz = sizes[dtype]
            world = dist.get_world_size(group)
            rank = dist.get_rank(group)
            base = ws.data_ptr()

            def view(ptr, n):
                off = ptr - base
                if off < 0 or off % esz or off + n * esz > ws.numel():
                    raise ValueError("slice outside the workspace")
                return ws[off: off + n * esz].view(tdt)

            if "v" not in legacy:
                legacy["v"] = dist.get_backend(group) == "gloo" and ws.is_cuda
            if op == _capi.COLL_REDUCE_SCATTER:
                full, part = view(send, world * count), view(recv, count)
                if not legacy["v"]:
                    dist.reduce_scatter_tensor(part, full, op=dist.ReduceOp.SUM, group=group)
                else:
                    dist.all_reduce(full, op=dist.ReduceOp.SUM, group=group)
                    if recv != send + rank * count * esz:
                        part.copy_(full[rank * count:(rank + 1) * count])
                return 0
            if op == _capi.COLL_ALL_GATHER:
                full, part = view(recv, world * count), view(send, count)
                if not legacy["v"]:
                    dist.all_gather_into_tensor(full, part, group=group)
                else:
                    mine = full[rank * count:(rank + 1) * count]
                    if send != recv + rank * count * esz:
                        mine.copy_(part)
                    keep = mine.clone()
                    full.zero_()
                    mine.copy_(keep)
                    if tdt == torch.bfloat16:  # exact: every element is non-zero on one rank only
                        f = full.float()
                        dist.all_reduce(f, op=dist.ReduceOp.SUM, group=group)
                        full.copy_(f)
                    else:
                        dist.all_reduce(full, op=dist.ReduceOp.SUM, group=group)
                return 0
            return 1
        except Exception:  # never unwind through C
            return 1

    return _capi.COLLECTIVE_FN(_hook)


class Engine:
    """One GPU handle (HIP stream + workspace); mirrors what a C++ caller gets from librsvd_hip."""

    def __init__(self, device: int = 0):
        self.device = device
        h = ctypes.c_void_p()
        check(lib().rsvd_create(device, ctypes.byref(h)))
        self.h = h
        self._ws = None
        self._hook = None

    def close(self):
        if getattr(self, "h", None):
            lib().rsvd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing --------------------------------------------------------------------------
    def _bind_stream(self):
        torch = _torch()
        s = torch.cuda.current_stream(self.device)
        check(lib().rsvd_set_stream(self.h, ctypes.c_void_p(s.cuda_stream)), self.h)

    def reserve(self, desc: Desc):
        """Allocate the workspace from torch's allocator (outside any timed region)."""
        nbytes = ctypes.c_size_t(0)
        check(lib().rsvd_workspace_bytes(ctypes.byref(desc), ctypes.byref(nbytes)))
        return self._reserve_bytes(nbytes.value)

    def _reserve_bytes(self, nbytes: int):
        torch = _torch()
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=f"cuda:{self.device}")
            check(lib().rsvd_set_workspace(self.h, ctypes.c_void_p(self._ws.data_ptr()), nbytes), self.h)
        return self._ws

    def workspace(self):
        """The handle's current workspace as a uint8 CUDA tensor, or None before the first
        reservation.  Its contents are unspecified between runs (include/rsvd_c.h)."""
        return self._ws

    def set_comm(self, rank: int, world: int, group=None, shard_n: bool = True):
        """Row-sharded runs: bind the exchange hooks to torch.distributed over RCCL -- the
        all-reduce (m-side Grams; A^T Q when the n side is replicated) and, with shard_n, the
        reduce-scatter / all-gather hook that shards the n side across ranks as well.  At world 1
        the collective hook is still bound with shard_n, for runs with force_nshard=True (the
        sharded code path and its collectives on one GPU)."""
        self._hook = make_allreduce_hook(lambda: self._ws, group)
        check(lib().rsvd_set_comm(self.h, rank, world, self._hook, None), self.h)
        self._coll = make_collective_hook(lambda: self._ws, group) if shard_n else None
        check(lib().rsvd_set_collectives(self.h, self._coll if self._coll is not None else _capi.COLLECTIVE_FN(), None),
              self.h)

    def emulate_world(self, rank: int, world: int):
        """Diagnostics (bench.py --emulate-world): run rank `rank` of a `world`-rank row-sharded rSVD
        on this one handle -- the kernels a rank of the N-GPU job runs, at its shapes (its rows of A,
        its n shard, the fp64 Grams of sharded panels) -- with every collective a no-op.  The
        exchanged values are then not the other ranks' (the outputs are not the SVD of any matrix), so
        this only prices the per-rank kernels; the collectives are priced apart."""
        self._hook = _capi.ALLREDUCE_FN(lambda buf, count, dt, stream, user: 0)
        self._coll = _capi.COLLECTIVE_FN(lambda op, send, recv, count, dt, stream, user: 0)
        check(lib().rsvd_set_comm(self.h, rank, world, self._hook, None), self.h)
        check(lib().rsvd_set_collectives(self.h, self._coll, None), self.h)

    @staticmethod
    def comm_unique_id() -> bytes:
        """rsvd_comm_unique_id: the RCCL id one rank draws and every rank passes to comm_init."""
        buf = ctypes.create_string_buffer(_capi.COMM_ID_BYTES)
        check(lib().rsvd_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, world: int, shard_n: bool = True):
        """rsvd_comm_init: the library-owned RCCL communicator (no Python hooks on the data path;
        what a C / C++ caller uses, include/rsvd_c.h ABI 6)."""
        if len(uid) != _capi.COMM_ID_BYTES:
            raise ValueError("bad RCCL unique id")
        buf = ctypes.create_string_buffer(uid, _capi.COMM_ID_BYTES)
        # the handle may still hold set_comm's trampolines if the call fails (librccl missing):
        # drop the Python references only once the library owns the collectives
        check(lib().rsvd_comm_init(self.h, buf, rank, world, int(shard_n)), self.h)
        self._hook = self._coll = None

    def comm_destroy(self):
        check(lib().rsvd_comm_destroy(self.h), self.h)

    def set_timing(self, enable: bool = True):
        """hipEvent timing of every projection GEMM launch (benchmarking only)."""
        check(lib().rsvd_set_timing(self.h, int(enable)), self.h)

    def timing(self) -> dict:
        t = Timing()
        check(lib().rsvd_get_timing(self.h, ctypes.byref(t)), self.h)
        return {k: getattr(t, k) for k, _ in Timing._fields_}

    def sync(self):
        """rsvd_sync: wait for the queued runs and raise what they could not report at enqueue time
        (a timed-out in-kernel hand-off, an unrepairable rank deficiency, non-finite S)."""
        check(lib().rsvd_sync(self.h), self.h)

    def info(self) -> dict:
        inf = Info()
        check(lib().rsvd_get_info(self.h, ctypes.byref(inf)), self.h)
        return {k: getattr(inf, k) for k, _ in Info._fields_}

    # -- device path -----------------------------------------------------------------------
    @staticmethod
    def abi_dtype(t_dtype) -> int:
        torch = _torch()
        dt = {torch.float64: _capi.F64, torch.float32: _capi.F32, torch.bfloat16: _capi.BF16,
              torch.float8_e4m3fn: _capi.FP8_E4M3}.get(t_dtype)
        if dt is None:
            raise TypeError(f"unsupported dtype {t_dtype}")
        return dt

    @staticmethod
    def out_dtype(t_dtype):
        """Element type of U, S, V, Omega and Q for an A of this dtype (fp32 for bf16 / fp8)."""
        torch = _torch()
        return t_dtype if t_dtype in (torch.float64, torch.float32) else torch.float32

    def desc(self, A, l: int, q: int = 2, method: int = SVDMethod.Jacobi, seed: int = 0,
             qr_mode: int = QRMode.Auto, a_scale: float = 1.0, flags: int = 0) -> Desc:
        dt = self.abi_dtype(A.dtype)
        lda = A.stride(1) if A.stride(0) == 1 else None
        if lda is None:
            raise ValueError("A must be column-major (use colmajor())")
        return Desc(m=A.shape[0], n=A.shape[1], lda=max(lda, A.shape[0]), l=l, q=q, dtype=dt,
                    method=int(method), qr_mode=int(qr_mode), flags=int(flags), seed=seed, a_scale=a_scale)

    def rsvd(self, A, l: int, q: int = 2, method: int = SVDMethod.Jacobi, omega=None, seed: int = 0,
             qr_mode: int = QRMode.Auto, out=None, a_scale: float = 1.0, check_errors: bool = True,
             lowp_intermediates: bool = False, force_nshard: bool = False):
        """Device rSVD: A (m x n, CUDA, column-major f64/f32/bf16/e4m3) -> U (m x l), S (l), V (n x l).

        check_errors=True synchronises and raises on the run's device-side failures (rsvd_sync);
        False leaves the run queued (asynchronous) -- call sync() later to check.
        lowp_intermediates: RSVD_FLAG_LOWP_INTERMEDIATES (include/rsvd_c.h; bf16 / e4m3 A, q >= 2).
        force_nshard: RSVD_FLAG_FORCE_NSHARD (tests: the n-side sharded path at world 1)."""
        torch = _torch()
        A, _ = colmajor(A)
        flags = (_capi.FLAG_LOWP_INTERMEDIATES if lowp_intermediates else 0) | (
            _capi.FLAG_FORCE_NSHARD if force_nshard else 0)
        d = self.desc(A, l, q, method, seed, qr_mode, a_scale, flags)
        self.reserve(d)
        self._bind_stream()
        m, n = A.shape
        dd = min(l, n)
        odt = self.out_dtype(A.dtype)
        if out is None:
            U = empty_colmajor(m, dd, odt, A.device)
            S = torch.empty(dd, dtype=odt, device=A.device)
            V = empty_colmajor(n, dd, odt, A.device)
        else:
            U, S, V = out
        om, ldo = (None, 0)
        if omega is not None:
            om, ldo = colmajor(omega.to(device=A.device, dtype=odt))
        check(lib().rsvd_run(self.h, ctypes.byref(d), ctypes.c_void_p(A.data_ptr()),
                             ctypes.c_void_p(om.data_ptr() if om is not None else 0), ldo,
                             ctypes.c_void_p(U.data_ptr()), U.stride(1),
                             ctypes.c_void_p(S.data_ptr()),
                             ctypes.c_void_p(V.data_ptr()), V.stride(1)), self.h)
        if check_errors:
            self.sync()
        return U, S, V

    # -- batched rSVD (rsvd_run_batched, include/rsvd_c.h ABI 7) ---------------------------------
    def batched_is_fused(self, m: int, n: int, l: int, dtype, q: int = 2, method: int = SVDMethod.Jacobi,
                         qr_mode: int = QRMode.Auto, batch: int = 1) -> int:
        """rsvd_batched_is_fused: 1 when a batch of m x n matrices of this dtype (a torch dtype or an
        ABI code) takes the fused one-launch kernel, 0 when rsvd_run_batched loops rsvd_run."""
        dt = dtype if isinstance(dtype, int) else self.abi_dtype(dtype)
        d = Desc(m=m, n=n, lda=m, l=l, q=q, dtype=dt, method=int(method), qr_mode=int(qr_mode), flags=0, seed=0,
                 a_scale=1.0)
        bd = _capi.BatchDesc(count0=batch, count1=1, a_stride0=m * n, a_stride1=0, omega_stride=0,
                             u_stride=m * l, s_stride=l, v_stride=n * l)
        return int(lib().rsvd_batched_is_fused(ctypes.byref(d), ctypes.byref(bd)))

    def _run_batched(self, d: Desc, bd, A, omega, U, S, V, ldu: int, ldv: int, return_info: bool, check_errors: bool):
        """Reserve, bind the stream and enqueue one rsvd_run_batched.  omega: None, (n, l) shared or
        (B, n, l); it is brought to the result dtype, every matrix column-major."""
        torch = _torch()
        odt = self.out_dtype(A.dtype)
        batch = bd.count0 * bd.count1
        om_ptr, ldo = 0, 0
        om = None
        if omega is not None:
            om = omega.to(device=A.device, dtype=odt)
            if om.dim() == 2:
                om, ldo = colmajor(om)
                bd.omega_stride = 0
            elif om.dim() == 3 and om.shape[0] == batch:
                if not (om.stride(1) == 1 and om.stride(2) >= max(1, om.shape[1])):
                    om = om.transpose(1, 2).contiguous().transpose(1, 2)
                ldo = max(om.stride(2), d.n)  # l == 1: the stride of the one-column dimension carries no meaning
                bd.omega_stride = om.stride(0) if batch > 1 else 0
            else:
                raise ValueError("omega must be (n, l) or (batch, n, l)")
            if tuple(om.shape[-2:]) != (d.n, d.l):
                raise ValueError("omega must have n rows and l columns")
            om_ptr = om.data_ptr()
        nbytes = ctypes.c_size_t(0)
        check(lib().rsvd_batched_workspace_bytes(ctypes.byref(d), ctypes.byref(bd), ctypes.byref(nbytes)))
        self._reserve_bytes(nbytes.value)
        self._bind_stream()
        info = torch.zeros((batch, 2), dtype=torch.int32, device=A.device) if return_info else None
        check(lib().rsvd_run_batched(self.h, ctypes.byref(d), ctypes.byref(bd), ctypes.c_void_p(A.data_ptr()),
                                     ctypes.c_void_p(om_ptr), ldo, ctypes.c_void_p(U.data_ptr()), ldu,
                                     ctypes.c_void_p(S.data_ptr()), ctypes.c_void_p(V.data_ptr()), ldv,
                                     ctypes.c_void_p(info.data_ptr() if info is not None else 0)), self.h)
        if check_errors:
            self.sync()
        return info

    def rsvd_batched(self, A, l: int, q: int = 2, method: int = SVDMethod.Jacobi, omega=None, seed: int = 0,
                     out=None, return_info: bool = False, check_errors: bool = True, a_scale: float = 1.0):
        """rSVD of every matrix of a CUDA tensor A (B, m, n): U (B, m, l), S (B, l), V (B, n, l) in
        out_dtype(A.dtype), each matrix column-major.  Entry b is rsvd(A[b], l, q, seed=seed + b).

        Each A[b] is used in place when it is column-major (stride(1) == 1, stride(2) >= m, any
        stride(0)); any other layout gets one copy into that layout.  Small fp64 / fp32 matrices
        (batched_is_fused) run in ONE launch, one workgroup per matrix; everything else loops rsvd.
        omega: (n, l) shared by all, or (B, n, l).  return_info adds an int32 (B, 2) tensor: Jacobi
        sweeps, and bit 0 = rank-deficient sketch met, bit 1 = non-finite S.  a_scale as rsvd's:
        A = a_scale * stored A, S scales by |a_scale| and V takes its sign."""
        torch = _torch()
        if A.dim() != 3:
            raise ValueError("expected a (B, m, n) tensor")
        B, m, n = A.shape
        if not (A.stride(1) == 1 and A.stride(2) >= max(1, m)):
            A = A.transpose(1, 2).contiguous().transpose(1, 2)
        odt = self.out_dtype(A.dtype)
        if out is None:
            U = torch.empty((B, l, m), dtype=odt, device=A.device).transpose(1, 2)
            S = torch.empty((B, l), dtype=odt, device=A.device)
            V = torch.empty((B, l, n), dtype=odt, device=A.device).transpose(1, 2)
        else:
            U, S, V = out
            for X, rows in ((U, m), (V, n)):
                if tuple(X.shape) != (B, rows, l) or X.dtype != odt or X.stride(1) != 1 or X.stride(2) < rows:
                    raise ValueError("out: U and V must be (B, rows, l), each matrix column-major, of the result dtype")
            if tuple(S.shape) != (B, l) or S.dtype != odt or (l > 1 and S.stride(1) != 1):
                raise ValueError("out: S must be (B, l) with unit stride along l, of the result dtype")
        d = Desc(m=m, n=n, lda=max(A.stride(2), m), l=l, q=q, dtype=self.abi_dtype(A.dtype), method=int(method),
                 qr_mode=int(QRMode.Auto), flags=0, seed=seed, a_scale=a_scale)
        one = B == 1  # a stride of a one-element dimension carries no meaning
        bd = _capi.BatchDesc(count0=B, count1=1, a_stride0=0 if one else A.stride(0), a_stride1=0, omega_stride=0,
                             u_stride=U.stride(2) * l if one else U.stride(0), s_stride=l if one else S.stride(0),
                             v_stride=V.stride(2) * l if one else V.stride(0))
        info = self._run_batched(d, bd, A, omega, U, S, V, U.stride(2), V.stride(2), return_info, check_errors)
        return (U, S, V, info) if return_info else (U, S, V)

    def rsvd_tiles(self, A, tile_m: int, tile_n: int, l: int, q: int = 2, method: int = SVDMethod.Jacobi,
                   omega=None, seed: int = 0, return_info: bool = False, check_errors: bool = True):
        """One rSVD per tile_m x tile_n tile of the 2-D column-major A (any lda, any storage offset),
        read in place through strides: the block decomposition of the reference's
        Image::compress_parallel (image_compression/src/image_com.cpp:350-371).  Returns
        U (gr, gc, tile_m, l), S (gr, gc, l), V (gr, gc, tile_n, l); tile (i, j) is
        A[i*tile_m:(i+1)*tile_m, j*tile_n:(j+1)*tile_n] and draws seed + i + gr*j.
        omega: (tile_n, l) shared, or (gr*gc, tile_n, l) indexed by b = i + gr*j."""
        torch = _torch()
        if A.dim() != 2:
            raise ValueError("expected a matrix")
        m, n = A.shape
        if tile_m <= 0 or tile_n <= 0 or m % tile_m or n % tile_n:
            raise ValueError(f"tile {tile_m} x {tile_n} does not divide the {m} x {n} matrix")
        A, lda = colmajor(A)
        gr, gc = m // tile_m, n // tile_n
        odt = self.out_dtype(A.dtype)
        Ub = torch.empty((gc, gr, l, tile_m), dtype=odt, device=A.device)
        Sb = torch.empty((gc, gr, l), dtype=odt, device=A.device)
        Vb = torch.empty((gc, gr, l, tile_n), dtype=odt, device=A.device)
        d = Desc(m=tile_m, n=tile_n, lda=max(lda, m), l=l, q=q, dtype=self.abi_dtype(A.dtype), method=int(method),
                 qr_mode=int(QRMode.Auto), flags=0, seed=seed, a_scale=1.0)
        bd = _capi.BatchDesc(count0=gr, count1=gc, a_stride0=tile_m, a_stride1=tile_n * max(lda, m), omega_stride=0,
                             u_stride=tile_m * l, s_stride=l, v_stride=tile_n * l)
        info = self._run_batched(d, bd, A, omega, Ub, Sb, Vb, tile_m, tile_n, return_info, check_errors)
        U, S, V = Ub.permute(1, 0, 3, 2), Sb.permute(1, 0, 2), Vb.permute(1, 0, 3, 2)
        if return_info:
            return U, S, V, info.view(gc, gr, 2).permute(1, 0, 2)
        return U, S, V

    # -- rank-k compression (rsvd_compress_batched / rsvd_lowrank, include/rsvd_c.h ABI 8) ---------
    @staticmethod
    def _check_k(k, l: int, n: int) -> int:
        k = l if k is None else int(k)
        if not 1 <= k <= min(l, n):
            raise ValueError(f"k = {k} must be in 1 .. min(l, n) = {min(l, n)}")
        return k

    def _run_compress(self, d: Desc, bd, cd, A, omega, C, factors, return_err: bool, return_info: bool,
                      check_errors: bool):
        """Reserve, bind the stream and enqueue one rsvd_compress_batched (omega as _run_batched's)."""
        torch = _torch()
        odt = self.out_dtype(A.dtype)
        batch = bd.count0 * bd.count1
        om_ptr, ldo = 0, 0
        if omega is not None:
            om = omega.to(device=A.device, dtype=odt)
            if om.dim() == 2:
                om, ldo = colmajor(om)
                bd.omega_stride = 0
            elif om.dim() == 3 and om.shape[0] == batch:
                if not (om.stride(1) == 1 and om.stride(2) >= max(1, om.shape[1])):
                    om = om.transpose(1, 2).contiguous().transpose(1, 2)
                ldo = max(om.stride(2), d.n)  # l == 1: the stride of the one-column dimension carries no meaning
                bd.omega_stride = om.stride(0) if batch > 1 else 0
            else:
                raise ValueError("omega must be (n, l) or (batch, n, l)")
            if tuple(om.shape[-2:]) != (d.n, d.l):
                raise ValueError("omega must have n rows and l columns")
            om_ptr = om.data_ptr()
        nbytes = ctypes.c_size_t(0)
        check(lib().rsvd_compress_workspace_bytes(ctypes.byref(d), ctypes.byref(bd), ctypes.byref(cd),
                                                  ctypes.byref(nbytes)))
        self._reserve_bytes(nbytes.value)
        self._bind_stream()
        err = torch.zeros((batch, 2), dtype=torch.float64, device=A.device) if return_err else None
        info = torch.zeros((batch, 2), dtype=torch.int32, device=A.device) if return_info else None
        U, S, V, ldu, ldv = factors if factors is not None else (None, None, None, 0, 0)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        check(lib().rsvd_compress_batched(self.h, ctypes.byref(d), ctypes.byref(bd), ctypes.byref(cd), ptr(A),
                                          ctypes.c_void_p(om_ptr), ldo, ptr(C), ptr(U), ldu, ptr(S), ptr(V), ldv,
                                          ptr(err), ptr(info)), self.h)
        if check_errors:
            self.sync()
        return err, info

    def compress_batched(self, A, l: int, k=None, q: int = 2, omega=None, seed: int = 0, out=None,
                         in_place: bool = False, return_factors: bool = False, return_err: bool = True,
                         return_info: bool = False, check_errors: bool = True, a_scale: float = 1.0):
        """Rank-k compression of every matrix of a CUDA tensor A (B, m, n): C (B, m, n), each matrix
        column-major, C[b] = U[:, :k] diag(S[:k]) V[:, :k]^T of rsvd_batched's entry b (k = l when None;
        what Image::compress_parallel rebuilds, image_compression/src/image_com.cpp:374), in
        out_dtype(A.dtype).  err (B, 2) float64 on the device: ||a_scale A[b]||_F^2 and
        ||a_scale A[b] - C[b]||_F^2 with C as stored.  Inside the fused limits (batched_is_fused) the
        rebuild and the error run in the same ONE launch as the rSVD and, without return_factors, the
        factors never leave the workgroup.  in_place: C overwrites A (fp64 / fp32 A, every matrix
        column-major and not overlapping its neighbours) and A itself is returned.
        Returns C, then err if return_err, then (U, S, V) if return_factors, then info if return_info."""
        torch = _torch()
        if A.dim() != 3:
            raise ValueError("expected a (B, m, n) tensor")
        B, m, n = A.shape
        k = self._check_k(k, l, n)
        odt = self.out_dtype(A.dtype)
        colm = A.stride(1) == 1 and A.stride(2) >= max(1, m)
        if in_place:
            if A.dtype != odt:
                raise ValueError("in_place needs an A of the result dtype (float64 or float32)")
            if not colm:
                raise ValueError("in_place needs every A[b] column-major")
            if out is not None:
                raise ValueError("in_place and out= exclude each other")
            C = A
        else:
            if not colm:
                A = A.transpose(1, 2).contiguous().transpose(1, 2)
            C = torch.empty((B, n, m), dtype=odt, device=A.device).transpose(1, 2) if out is None else out
            if tuple(C.shape) != (B, m, n) or C.dtype != odt or C.stride(1) != 1 or C.stride(2) < m:
                raise ValueError("out: C must be (B, m, n), each matrix column-major, of the result dtype")
        factors = None
        if return_factors:
            U = torch.empty((B, l, m), dtype=odt, device=A.device).transpose(1, 2)
            S = torch.empty((B, l), dtype=odt, device=A.device)
            V = torch.empty((B, l, n), dtype=odt, device=A.device).transpose(1, 2)
            factors = (U, S, V, m, n)
        d = Desc(m=m, n=n, lda=max(A.stride(2), m), l=l, q=q, dtype=self.abi_dtype(A.dtype),
                 method=int(SVDMethod.Jacobi), qr_mode=int(QRMode.Auto), flags=0, seed=seed, a_scale=a_scale)
        one = B == 1  # a stride of a one-element dimension carries no meaning
        bd = _capi.BatchDesc(count0=B, count1=1, a_stride0=0 if one else A.stride(0), a_stride1=0, omega_stride=0,
                             u_stride=m * l, s_stride=l, v_stride=n * l)
        cd = _capi.CompressDesc(k=k, reserved=0, ldc=max(C.stride(2), m), c_stride0=0 if one else C.stride(0),
                                c_stride1=0)
        err, info = self._run_compress(d, bd, cd, A, omega, C, factors, return_err, return_info, check_errors)
        res = [C] + ([err] if return_err else []) + ([factors[:3]] if return_factors else [])
        res += [info] if return_info else []
        return res[0] if len(res) == 1 else tuple(res)

    def compress_tiles(self, A, tile_m: int, tile_n: int, l: int, k=None, q: int = 2, omega=None, seed: int = 0,
                       out=None, in_place: bool = False, return_factors: bool = False, return_err: bool = True,
                       return_info: bool = False, check_errors: bool = True, a_scale: float = 1.0):
        """Image::compress_parallel's numeric core (image_compression/src/image_com.cpp:325-404): every
        tile_m x tile_n tile of the 2-D column-major A is replaced by its rank-k rebuild, in one launch
        inside the fused limits.  Returns C (m, n) column-major -- A itself when in_place -- and
        err (gr, gc, 2) as compress_batched's; tile (i, j) draws seed + i + gr*j, exactly as rsvd_tiles;
        factors come back in rsvd_tiles' shapes, info as (gr, gc, 2)."""
        torch = _torch()
        if A.dim() != 2:
            raise ValueError("expected a matrix")
        m, n = A.shape
        if tile_m <= 0 or tile_n <= 0 or m % tile_m or n % tile_n:
            raise ValueError(f"tile {tile_m} x {tile_n} does not divide the {m} x {n} matrix")
        k = self._check_k(k, l, tile_n)
        odt = self.out_dtype(A.dtype)
        if in_place:
            if A.dtype != odt:
                raise ValueError("in_place needs an A of the result dtype (float64 or float32)")
            if not (A.stride(0) == 1 and A.stride(1) >= max(1, m)):
                raise ValueError("in_place needs a column-major A")
            if out is not None:
                raise ValueError("in_place and out= exclude each other")
            lda = A.stride(1)
            C = A
        else:
            A, lda = colmajor(A)
            C = empty_colmajor(m, n, odt, A.device) if out is None else out
            if tuple(C.shape) != (m, n) or C.dtype != odt or C.stride(0) != 1 or C.stride(1) < m:
                raise ValueError("out: C must be (m, n), column-major, of the result dtype")
        gr, gc = m // tile_m, n // tile_n
        factors = None
        if return_factors:
            Ub = torch.empty((gc, gr, l, tile_m), dtype=odt, device=A.device)
            Sb = torch.empty((gc, gr, l), dtype=odt, device=A.device)
            Vb = torch.empty((gc, gr, l, tile_n), dtype=odt, device=A.device)
            factors = (Ub, Sb, Vb, tile_m, tile_n)
        lda, ldc = max(lda, m), max(C.stride(1), m)
        d = Desc(m=tile_m, n=tile_n, lda=lda, l=l, q=q, dtype=self.abi_dtype(A.dtype), method=int(SVDMethod.Jacobi),
                 qr_mode=int(QRMode.Auto), flags=0, seed=seed, a_scale=a_scale)
        bd = _capi.BatchDesc(count0=gr, count1=gc, a_stride0=tile_m, a_stride1=tile_n * lda, omega_stride=0,
                             u_stride=tile_m * l, s_stride=l, v_stride=tile_n * l)
        cd = _capi.CompressDesc(k=k, reserved=0, ldc=ldc, c_stride0=tile_m, c_stride1=tile_n * ldc)
        err, info = self._run_compress(d, bd, cd, A, omega, C, factors, return_err, return_info, check_errors)
        res = [C] + ([err.view(gc, gr, 2).permute(1, 0, 2)] if return_err else [])
        if return_factors:
            res.append((factors[0].permute(1, 0, 3, 2), factors[1].permute(1, 0, 2), factors[2].permute(1, 0, 3, 2)))
        res += [info.view(gc, gr, 2).permute(1, 0, 2)] if return_info else []
        return res[0] if len(res) == 1 else tuple(res)

    def lowrank(self, U, S, V, k=None, A=None, out=None, a_scale: float = 1.0):
        """C = U[:, :k] diag(S[:k]) V[:, :k]^T (Image::reconstruct, image_compression/src/image_com.cpp:
        184-190) for factors of any size, column-major in their dtype (float64 / float32); k = all of
        them when None.  With A (m x n: float64 for float64 factors, else float32 / bfloat16 /
        float8_e4m3fn; the matrix is a_scale * A) also returns err (2,) float64 on the device:
        ||a_scale A||_F^2 and ||a_scale A - C||_F^2, computed in the same pass.  out: a column-major
        (m, n) tensor to write into (A itself compresses in place); out=False with A: the error alone."""
        torch = _torch()
        if U.dim() != 2 or V.dim() != 2 or S.dim() != 1:
            raise ValueError("expected U (m, d), S (d), V (n, d)")
        m, n, dd = U.shape[0], V.shape[0], S.shape[0]
        if U.shape[1] != dd or V.shape[1] != dd or U.dtype != S.dtype or V.dtype != S.dtype:
            raise ValueError("U, S and V must share their dtype and their number of columns")
        if U.dtype not in (torch.float64, torch.float32):
            raise TypeError(f"unsupported dtype {U.dtype}")
        k = dd if k is None else int(k)
        if not 1 <= k <= dd:
            raise ValueError(f"k = {k} must be in 1 .. {dd}")
        if A is not None and (tuple(A.shape) != (m, n) or self.out_dtype(A.dtype) != U.dtype):
            raise ValueError("A must be (m, n) with the factors as its result dtype")
        if out is False and A is None:
            raise ValueError("nothing to compute: no C and no A")
        U, ldu = colmajor(U)
        V, ldv = colmajor(V)
        S = S.contiguous()
        if out is None:
            C = empty_colmajor(m, n, U.dtype, U.device)
        elif out is False:
            C = None
        else:
            C = out
            if tuple(C.shape) != (m, n) or C.dtype != U.dtype or C.stride(0) != 1 or C.stride(1) < m:
                raise ValueError("out: C must be (m, n), column-major, of the factors' dtype")
        lda, a_dt, err = 0, 0, None
        if A is not None:
            if not (C is not None and A.data_ptr() == C.data_ptr()):
                A, _ = colmajor(A)
            lda, a_dt = max(A.stride(1), m), self.abi_dtype(A.dtype)
            err = torch.zeros(2, dtype=torch.float64, device=U.device)
            nbytes = ctypes.c_size_t(0)
            check(lib().rsvd_lowrank_workspace_bytes(m, n, ctypes.byref(nbytes)))
            self._reserve_bytes(nbytes.value)
        self._bind_stream()
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        check(lib().rsvd_lowrank(self.h, m, n, k, self.abi_dtype(U.dtype), ptr(U), max(ldu, m), ptr(S), ptr(V),
                                 max(ldv, n), ptr(C), max(C.stride(1), m) if C is not None else 0, ptr(A), lda, a_dt,
                                 a_scale, ptr(err)), self.h)
        if A is None:
            return C
        return err if C is None else (C, err)

    # -- POD (rsvd_pod, include/rsvd_c.h ABI 9) ---------------------------------------------------
    @staticmethod
    def _pod_desc(nh: int, ns: int, lds: int, r: int, dtype: int, svd_type: int, q: int, seed: int, tol: float,
                  textbook: bool) -> "_capi.PodDesc":
        return _capi.PodDesc(nh=nh, ns=ns, lds=lds, r=r, dtype=dtype, svd_type=int(svd_type), q=q,
                             flags=_capi.POD_FLAG_TEXTBOOK if textbook else 0, reserved=0, seed=seed, tol=tol)

    def pod_plan(self, nh: int, ns: int, dtype=_capi.F64, r: int = 1):
        """rsvd_pod_plan: (upper 32 x 32 block pairs of C, row chunks) of the correlation kernel for an
        nh x ns S -- host arithmetic, a function of (nh, ns, dtype) alone."""
        dt = dtype if isinstance(dtype, int) else self.abi_dtype(dtype)
        pd = self._pod_desc(nh, ns, nh, r, dt, 4, 2, 0, 0.0, False)
        tiles, chunks = ctypes.c_int32(0), ctypes.c_int32(0)
        check(lib().rsvd_pod_plan(ctypes.byref(pd), ctypes.byref(tiles), ctypes.byref(chunks)))
        return tiles.value, chunks.value

    def pod(self, S, r: int, tol: float, Xh=None, d=None, svd_type: int = 4, q: int = 2, seed: int = 0,
            textbook: bool = False, return_corr: bool = False, out=None, truncate: bool = True):
        """POD modes of the snapshot matrix S (nh x ns CUDA, column-major float64 / float32, ns <= nh), the
        snapshot method of the reference's class POD (POD.cpp:136-462) on the device: C = D^1/2 S^T Xh S
        D^1/2 in fp64 by the split-K correlation kernel, the small SVD (svd_type 1 / 2) or rSVD (4 / 5, width
        r, q power iterations, Omega = Philox(seed)) of C in fp64, the reference's rank rule, and
        W[:, i] = S D^1/2 V[:, i] / sigma_i.  S is read in place (any leading dimension, any storage offset).
        Xh: a torch sparse-CSR tensor or a (rowptr, colind, val) triple (indices are cast to int32, values to
        S's dtype); d: ns positive weights (the diagonal of D).  textbook: RSVD_POD_FLAG_TEXTBOOK.
        out: a column-major nh x r tensor for W (any leading dimension >= nh).
        Returns (W[:, :N], sigma, N) -- sigma float64 with ns entries, N an int; this reads N back and is the
        one place that synchronises -- with C (ns x ns float64) appended when return_corr.  truncate=False
        returns the full W and N as a device int32 tensor without synchronising."""
        torch = _torch()
        if S.dim() != 2:
            raise ValueError("expected a matrix")
        if S.dtype not in (torch.float64, torch.float32):
            raise TypeError(f"unsupported dtype {S.dtype}")
        S, lds = colmajor(S)
        nh, ns = S.shape
        lds = max(lds, nh) if ns > 1 else nh
        dev = S.device
        pd = self._pod_desc(nh, ns, lds, int(r), self.abi_dtype(S.dtype), svd_type, q, seed, float(tol), textbook)
        nbytes = ctypes.c_size_t(0)
        check(lib().rsvd_pod_workspace_bytes(ctypes.byref(pd), int(Xh is not None), ctypes.byref(nbytes)))
        csr, keep = None, None
        if Xh is not None:
            if _is_torch(Xh):
                rowptr, colind, val = Xh.crow_indices(), Xh.col_indices(), Xh.values()
            else:
                rowptr, colind, val = Xh
            rowptr = torch.as_tensor(rowptr).to(device=dev, dtype=torch.int32).contiguous()
            colind = torch.as_tensor(colind).to(device=dev, dtype=torch.int32).contiguous()
            val = torch.as_tensor(val).to(device=dev, dtype=S.dtype).contiguous()
            if rowptr.numel() != nh + 1 or colind.numel() != val.numel():
                raise ValueError("Xh must be nh x nh in CSR: nh + 1 row pointers, as many column indices as values")
            keep = (rowptr, colind, val)
            csr = _capi.Csr(rowptr=rowptr.data_ptr(), colind=colind.data_ptr(), val=val.data_ptr(), nnz=val.numel())
        dv = None
        if d is not None:
            dv = torch.as_tensor(d).to(device=dev, dtype=torch.float64).contiguous()
            if dv.dim() != 1 or dv.numel() != ns:
                raise ValueError("d must hold ns weights")
        W = empty_colmajor(nh, r, S.dtype, dev) if out is None else out
        ldw = self._check_out(W, nh, r, S.dtype, "W")
        sigma = torch.empty(ns, dtype=torch.float64, device=dev)
        N = torch.empty(1, dtype=torch.int32, device=dev)
        C = torch.empty((ns, ns), dtype=torch.float64, device=dev) if return_corr else None
        self._reserve_bytes(nbytes.value)
        self._bind_stream()
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        check(lib().rsvd_pod(self.h, ctypes.byref(pd), ptr(S), ctypes.byref(csr) if csr is not None else None,
                             ptr(dv), ptr(W), ldw, ptr(sigma), ptr(N), ptr(C)), self.h)
        del keep
        if not truncate:
            return (W, sigma, N, C) if return_corr else (W, sigma, N)
        self.sync()
        n = int(N.item())
        return (W[:, :n], sigma, n, C) if return_corr else (W[:, :n], sigma, n)

    def pod_host(self, S: np.ndarray, r: int, tol: float, Xh=None, d=None, svd_type: int = 4, q: int = 2,
                 seed: int = 0, textbook: bool = False):
        """pod() for numpy input through rsvd_pod_host_f64 (what include/POD.hpp calls): S float64, Xh a
        dense nh x nh array (exact zeros dropped) or a (rowptr, colind, val) triple, d the ns weights.
        Returns (W[:, :N], sigma, N)."""
        S = np.asfortranarray(S, dtype=np.float64)
        nh, ns = S.shape
        pd = self._pod_desc(nh, ns, nh, int(r), _capi.F64, svd_type, q, seed, float(tol), textbook)
        nbytes = ctypes.c_size_t(0)
        check(lib().rsvd_pod_workspace_bytes(ctypes.byref(pd), int(Xh is not None), ctypes.byref(nbytes)))
        rp = ci = va = None
        nnz = 0
        if Xh is not None:
            if isinstance(Xh, tuple):
                rp, ci, va = Xh
            else:
                rp, ci, va = dense_to_csr(np.asarray(Xh, dtype=np.float64))
            rp = np.ascontiguousarray(rp, dtype=np.int32)
            ci = np.ascontiguousarray(ci, dtype=np.int32)
            va = np.ascontiguousarray(va, dtype=np.float64)
            if rp.size != nh + 1 or ci.size != va.size:
                raise ValueError("Xh must be nh x nh in CSR: nh + 1 row pointers, as many column indices as values")
            nnz = va.size
        dv = None
        if d is not None:
            dv = np.ascontiguousarray(d, dtype=np.float64)
            if dv.ndim != 1 or dv.size != ns:
                raise ValueError("d must hold ns weights")
        W = np.zeros((nh, r), order="F")
        sigma = np.zeros(ns)
        N = ctypes.c_int32(0)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if a is not None else None
        self._reserve_bytes(nbytes.value)
        self._bind_stream()
        check(lib().rsvd_pod_host_f64(self.h, ctypes.byref(pd), _dp(S), ip(rp), ip(ci),
                                      _dp(va) if va is not None else None, nnz,
                                      _dp(dv) if dv is not None else None, _dp(W), _dp(sigma), ctypes.byref(N)),
              self.h)
        return W[:, :N.value].copy(order="F"), sigma, N.value

    def range_finder(self, A, omega, q: int = 2, qr_mode: int = QRMode.Auto, out=None):
        """Device intermediate_step: the orthonormal range basis Q (m x l).  out: a column-major
        m x l tensor to write Q into (any leading dimension >= m), as rsvd's out=."""
        A, _ = colmajor(A)
        odt = self.out_dtype(A.dtype)
        om, ldo = colmajor(omega.to(device=A.device, dtype=odt))
        l = om.shape[1]
        d = self.desc(A, l, q, SVDMethod.Jacobi, 0, qr_mode)
        self.reserve(d)
        self._bind_stream()
        Q = empty_colmajor(A.shape[0], l, odt, A.device) if out is None else out
        if Q.shape != (A.shape[0], l) or Q.dtype != odt or Q.stride(0) != 1 or Q.stride(1) < A.shape[0]:
            raise ValueError("out must be a column-major m x l matrix of the result dtype")
        check(lib().rsvd_range_finder(self.h, ctypes.byref(d), ctypes.c_void_p(A.data_ptr()),
                                      ctypes.c_void_p(om.data_ptr()), ldo, ctypes.c_void_p(Q.data_ptr()),
                                      Q.stride(1)), self.h)
        self.sync()
        return Q

    def generate_omega(self, n: int, l: int, seed: int = 0, dtype=None):
        """Omega on the device.  dtype bfloat16 / float8_e4m3fn: the Omega those A types draw
        (Philox values rounded to bf16 / e4m3), returned as float32."""
        torch = _torch()
        dtype = dtype or torch.float64
        lp = 16
        while lp < l:
            lp *= 2
        self._reserve_bytes(n * lp * 8)
        self._bind_stream()
        Om = empty_colmajor(n, l, self.out_dtype(dtype), f"cuda:{self.device}")
        check(lib().rsvd_generate_omega(self.h, n, l, seed, self.abi_dtype(dtype),
                                        ctypes.c_void_p(Om.data_ptr())), self.h)
        return Om

    # -- host fp64 path (the Eigen-callers' drop-in) ----------------------------------------
    def rsvd_host(self, A: np.ndarray, l: int, q: int = 2, method: int = SVDMethod.Jacobi,
                  omega: Optional[np.ndarray] = None, seed: int = 0):
        A = np.asfortranarray(A, dtype=np.float64)
        m, n = A.shape
        dd = min(l, n)
        U = np.zeros((m, dd), order="F")
        S = np.zeros(dd)
        V = np.zeros((n, dd), order="F")
        om = None if omega is None else np.asfortranarray(omega, dtype=np.float64)
        self.reserve(Desc(m=m, n=n, lda=m, l=l, q=q, dtype=_capi.F64, method=int(method)))
        self._bind_stream()
        check(lib().rsvd_run_host_f64(self.h, m, n, _dp(A), m, l, q, int(method),
                                      _dp(om) if om is not None else None, seed, _dp(U), _dp(S), _dp(V)),
              self.h)
        return U, S, V

    def range_finder_host(self, A: np.ndarray, omega: np.ndarray, q: int = 2) -> np.ndarray:
        A = np.asfortranarray(A, dtype=np.float64)
        om = np.asfortranarray(omega, dtype=np.float64)
        m, n = A.shape
        l = om.shape[1]
        Q = np.zeros((m, l), order="F")
        self.reserve(Desc(m=m, n=n, lda=m, l=l, q=q, dtype=_capi.F64))
        self._bind_stream()
        check(lib().rsvd_range_finder_host_f64(self.h, m, n, _dp(A), m, _dp(om), l, q, _dp(Q)), self.h)
        return Q

    def generate_omega_host(self, n: int, l: int, seed: int = 0) -> np.ndarray:
        om = np.zeros((n, l), order="F")
        self._reserve_bytes(n * ((l + 15) // 16 * 16) * 8)
        self._bind_stream()
        check(lib().rsvd_generate_omega_host_f64(self.h, n, l, seed, _dp(om)), self.h)
        return om

    # -- QR() and SVD<method> drop-ins (dense_api.cpp) ------------------------------------------
    def _reserve_dense(self, fn, m, n, dt, arg):
        nbytes = ctypes.c_size_t(0)
        check(fn(m, n, dt, int(arg), ctypes.byref(nbytes)))
        self._reserve_bytes(nbytes.value)
        self._bind_stream()

    @staticmethod
    def _check_out(X, rows: int, cols: int, dtype, what: str):
        """out= matrices as range_finder's: column-major rows x cols of the result dtype, any leading
        dimension >= rows (a one-column matrix may carry any column stride)."""
        if (X.dim() != 2 or tuple(X.shape) != (rows, cols) or X.dtype != dtype or (rows > 1 and X.stride(0) != 1)
                or (cols > 1 and X.stride(1) < rows)):
            raise ValueError(f"out: {what} must be a column-major {rows} x {cols} matrix of the result dtype")
        return max(X.stride(1), rows, 1)

    def qr(self, A, full: bool = False, out=None):
        """Device QR of A (CUDA f64/f32): (Q, R), reduced (m x n, n x n) or full (m x m, m x n).
        out: (Q, R) column-major tensors to write into (any leading dimensions >= their rows)."""
        A, lda = colmajor(A)
        dt = self.abi_dtype(A.dtype)
        m, n = A.shape
        kq = m if full else n
        if out is None:
            Q = empty_colmajor(m, kq, A.dtype, A.device)
            R = empty_colmajor(kq, n, A.dtype, A.device)
        else:
            Q, R = out
        ldq = self._check_out(Q, m, kq, A.dtype, "Q")
        ldr = self._check_out(R, kq, n, A.dtype, "R")
        self._reserve_dense(lib().rsvd_qr_workspace_bytes, m, n, dt, full)
        check(lib().rsvd_qr(self.h, m, n, ctypes.c_void_p(A.data_ptr()), max(lda, m), dt, int(full),
                            ctypes.c_void_p(Q.data_ptr()), ldq, ctypes.c_void_p(R.data_ptr()), ldr), self.h)
        self.sync()
        return Q, R

    def svd(self, A, method: int = SVDMethod.Jacobi, r: int = 0, seed: int = 0, out=None):
        """Device SVD<method> of A (CUDA): (U m x k, S k, V n x k), k = min(m, n) (Power: the
        triplets kept; V's columns are the right singular vectors).  out: (U m x k, S k, V n x k)
        to write into, U and V column-major with any leading dimensions >= their rows, S with unit
        stride; the views of the triplets kept are returned."""
        torch = _torch()
        A, lda = colmajor(A)
        dt = self.abi_dtype(A.dtype)
        m, n = A.shape
        k = min(m, n)
        if out is None:
            U = empty_colmajor(m, k, A.dtype, A.device)
            S = torch.empty(k, dtype=A.dtype, device=A.device)
            V = empty_colmajor(n, k, A.dtype, A.device)
        else:
            U, S, V = out
            if S.dim() != 1 or S.shape[0] != k or S.dtype != A.dtype or (k > 1 and S.stride(0) != 1):
                raise ValueError(f"out: S must be a unit-stride vector of {k} elements of the result dtype")
        ldu = self._check_out(U, m, k, A.dtype, "U")
        ldv = self._check_out(V, n, k, A.dtype, "V")
        self._reserve_dense(lib().rsvd_svd_workspace_bytes, m, n, dt, method)
        kept = ctypes.c_int32(0)
        check(lib().rsvd_svd(self.h, m, n, ctypes.c_void_p(A.data_ptr()), max(lda, m), dt, int(method), r, seed,
                             ctypes.c_void_p(U.data_ptr()), ldu, ctypes.c_void_p(S.data_ptr()),
                             ctypes.c_void_p(V.data_ptr()), ldv, ctypes.byref(kept)), self.h)
        self.sync()
        kk = kept.value
        return U[:, :kk], S[:kk], V[:, :kk]

    def qr_host(self, A: np.ndarray, full: bool = False):
        A = np.asfortranarray(A, dtype=np.float64)
        m, n = A.shape
        kq = m if full else n
        Q = np.zeros((m, kq), order="F")
        R = np.zeros((kq, n), order="F")
        self._reserve_dense(lib().rsvd_qr_workspace_bytes, m, n, _capi.F64, full)
        check(lib().rsvd_qr_host_f64(self.h, m, n, _dp(A), m, int(full), _dp(Q), _dp(R)), self.h)
        return Q, R

    def svd_host(self, A: np.ndarray, method: int = SVDMethod.Jacobi, r: int = 0, seed: int = 0):
        A = np.asfortranarray(A, dtype=np.float64)
        m, n = A.shape
        k = min(m, n)
        U = np.zeros((m, k), order="F")
        S = np.zeros(k)
        V = np.zeros((n, k), order="F")
        kept = ctypes.c_int32(0)
        self._reserve_dense(lib().rsvd_svd_workspace_bytes, m, n, _capi.F64, method)
        check(lib().rsvd_svd_host_f64(self.h, m, n, _dp(A), m, int(method), r, seed, _dp(U), _dp(S), _dp(V),
                                      ctypes.byref(kept)), self.h)
        kk = kept.value
        return U[:, :kk].copy(order="F"), S[:kk].copy(), V[:, :kk].copy(order="F")


_DEFAULT: Optional[Engine] = None


def compression_ratio(m: int, n: int, l: int) -> float:
    """Image::get_compression_ratio (image_compression/src/image_com.cpp:406-410): the m x n matrix
    against its l triplets, m n / (l (m + n + 1))."""
    return m * n / (l * (m + n + 1))


def pod_rank(sigma, tol: float, textbook: bool = False) -> int:
    """The reference's rank rule (POD.cpp:203-216) on the values `sigma` (its first r): the smallest N
    whose running share of sum sigma_i^2 reaches 1 - tol^2, by the reference's loop
        while (I < 1 - tol^2 && N < r) { num += sigma_N^2; I = num / den; N++; }
    in float64.  A zero sum keeps no mode (N = 0), as rsvd_pod.  textbook: weigh by sigma_i instead of
    sigma_i^2 (RSVD_POD_FLAG_TEXTBOOK: sigma_i of the correlation matrix is sigma_i(S)^2 already)."""
    w = [float(s) if textbook else float(s) * float(s) for s in np.asarray(sigma, dtype=np.float64).ravel()]
    den = 0.0
    for x in w:
        den += x
    if den == 0.0:
        return 0
    thr = 1.0 - float(tol) * float(tol)
    N, I, num = 0, 0.0, 0.0
    while I < thr and N < len(w):
        num += w[N]
        I = num / den
        N += 1
    return N


def dense_to_csr(X: np.ndarray):
    """(rowptr, colind, val) of a dense square matrix, exact zeros dropped (what include/POD.hpp does to the
    reference's dense Xh)."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("expected a matrix")
    mask = X != 0
    rowptr = np.zeros(X.shape[0] + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(mask.sum(axis=1))
    rows, cols = np.nonzero(mask)  # row-major order: each row's entries by ascending column
    return rowptr, cols.astype(np.int32), np.ascontiguousarray(X[rows, cols])


def default_engine() -> Engine:
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Engine(0)
    return _DEFAULT


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


# ---- reference-named free functions ------------------------------------------------------------
def rSVD(A, l: int, method: SVDMethod = SVDMethod.Jacobi, q: int = 2, omega=None, seed: int = 0):
    """rSVD (src/rSVD.cpp:72-133). Returns (U, S, V); q defaults to the reference's hard-coded 2.

    SVDMethod.Power returns the reference's layouts (src/rSVD.cpp:106-113): U m x l, S l and V the
    n x n V_ of SVD<Power> (v_i in row i, identity rows beyond), cut to the triplets kept on an
    early stop (SVD_class.hpp:198-208).  Engine.rsvd returns V as columns instead."""
    eng = default_engine()
    if _is_torch(A):
        U, S, V = eng.rsvd(A, l, q=q, method=method, omega=omega, seed=seed)
    else:
        U, S, V = eng.rsvd_host(A, l, q=q, method=method, omega=omega, seed=seed)
    if int(method) != SVDMethod.Power:
        return U, S, V
    kept = eng.info()["power_kept"]
    xp = _torch() if _is_torch(A) else np
    n = V.shape[0]
    Vf = xp.eye(n, dtype=V.dtype, **({"device": V.device} if _is_torch(A) else {}))
    Vf[:kept, :] = V[:, :kept].T
    if kept >= S.shape[0]:
        return U, S, Vf
    if kept == 0:
        z = xp.zeros
        return z((U.shape[0], 1), dtype=U.dtype), z(1, dtype=S.dtype), z((n, 1), dtype=V.dtype)
    return U[:, :kept], S[:kept], Vf[:, :kept]


def rSVD_image_compression(A, l: int, omega=None, seed: int = 0):
    """image_compression's 5-argument rSVD(A, U, S, V, l) (image_compression/src/rSVD.cpp:77-118): q = 1,
    its own power-method SVD of B (image_compression/src/SVD.cpp:30-55 -- B = A^T A recomputed after
    every deflation, no sigma < 1e-12 stop) and V = VT^T with the right singular vectors in columns.
    Returns (U m x d, S d, V n x d), d = min(l, n)."""
    eng = default_engine()
    if _is_torch(A):
        return eng.rsvd(A, l, q=1, method=_capi.SVD_POWER_IC, omega=omega, seed=seed)
    return eng.rsvd_host(A, l, q=1, method=_capi.SVD_POWER_IC, omega=omega, seed=seed)


def intermediate_step(A, Omega, l: int, q: int):
    """intermediate_step (src/rSVD.cpp:57-70): the orthonormal range basis Q (m x l)."""
    eng = default_engine()
    if _is_torch(A):
        return eng.range_finder(A, Omega[:, :l], q=q)
    return eng.range_finder_host(A, np.asarray(Omega)[:, :l], q=q)


def generateOmega(n: int, l: int, seed: int = 0):
    """generateOmega (src/rSVD.cpp:12-55): n x l N(0,1), reproducible from `seed`."""
    return default_engine().generate_omega_host(n, l, seed)


def qr_decomposition_reduced(A):
    """qr_decomposition_reduced (src/QR.cpp:43-80): (Q m x n, R n x n); requires m >= n."""
    eng = default_engine()
    return eng.qr(A, full=False) if _is_torch(A) else eng.qr_host(A, full=False)


def qr_decomposition_full(A):
    """qr_decomposition_full (src/QR.cpp:22-41): (Q m x m, R m x n)."""
    eng = default_engine()
    return eng.qr(A, full=True) if _is_torch(A) else eng.qr_host(A, full=True)


class SVD:
    """template<SVDMethod method> class SVD (include/SVD_class.hpp:35-71) on the GPU engine.

    ``SVD(data, r=0, method=SVDMethod.Jacobi)``; ``compute()``; ``getU/getS/getV``; ``setData``.
    Output shapes follow the reference: Jacobi / ParallelJacobi U m x k, S k, V n x k
    (k = min(m, n), :107-108); Power U m x m and V n x n initialised to the identity with u_i in
    column i of U and v_i in ROW i of V (:82-83, :213-214), S of length min(m, n); when the
    power method stops early at sigma < 1e-12 after i triplets the three are cut to their first i
    columns as conservativeResize does (:198-208).  ``compute()`` prints nothing (the reference
    writes progress to stdout, :80-95).  ``seed`` replaces the power method's random_device start
    vectors (src/PM.cpp:15-16) with Philox(seed + i).
    """

    def __init__(self, data, r: int = 0, method: SVDMethod = SVDMethod.Jacobi, seed: int = 0):
        self._data = np.array(data, dtype=np.float64, order="F", copy=True)
        self._r = int(r)
        self._method = SVDMethod(method)
        self._seed = seed
        self._U = self._S = self._V = None

    def setData(self, data):
        self._data = np.array(data, dtype=np.float64, order="F", copy=True)

    def compute(self):
        m, n = self._data.shape
        eng = default_engine()
        if self._method != SVDMethod.Power:
            self._U, self._S, self._V = eng.svd_host(self._data, self._method)
            return
        dim = self._r if self._r else min(m, n)
        u, s, v = eng.svd_host(self._data, SVDMethod.Power, r=self._r, seed=self._seed)
        k = s.shape[0]
        if k == 0:
            self._U, self._S, self._V = np.zeros((m, 1)), np.zeros(1), np.zeros((n, 1))
            return
        U = np.eye(m, order="F")
        V = np.eye(n, order="F")
        S = np.zeros(min(m, n))
        U[:, :k] = u
        V[:k, :] = v.T
        S[:k] = s
        if k < dim:
            U, S, V = U[:, :k].copy(order="F"), S[:k].copy(), V[:, :k].copy(order="F")
        self._U, self._S, self._V = U, S, V

    def getU(self):
        return self._U

    def getS(self):
        return self._S

    def getV(self):
        return self._V


class POD:
    """class POD (POD/ParametricDiffusion1D/src/POD.hpp:24-49) on the GPU engine: ``.W`` holds the POD
    basis (Nh x N) and ``.sigma`` the singular values.  The reference's four constructors map to

    * ``POD(S, r, svd_type=...)``                       naive: the SVD / rSVD of S itself (POD.cpp:116-133)
    * ``POD(S, r, tol, svd_type=...)``                  standard_POD (:136-224)
    * ``POD(S, r, tol, Xh=Xh, svd_type=...)``           energy_POD (:227-336)
    * ``POD(S, r, tol, Xh=Xh, D=D, svd_type=...)``      weight_POD (:339-462); D a vector of weights or a
      diagonal matrix (a non-diagonal D raises ValueError)

    svd_type is the reference's 0..5 (POD.cpp:49-92).  The three snapshot-method variants need ns <= Nh
    and svd_type 1, 2, 4 or 5 (ValueError otherwise); S may be a numpy array or a CUDA tensor.  Nothing is
    printed.  ``N`` is the rank the rule kept; ``textbook`` selects RSVD_POD_FLAG_TEXTBOOK."""

    def __init__(self, S=None, r: int = 0, tol: Optional[float] = None, svd_type: int = 4, Xh=None, D=None,
                 q: int = 2, seed: int = 0, textbook: bool = False):
        self.W = self.sigma = None
        self.N = 0
        if S is None:  # the default constructor
            return
        if not 0 <= int(svd_type) <= 5:
            raise ValueError("The svd_type should be in [0,5].")
        if tol is None:
            if Xh is not None or D is not None:
                raise ValueError("Xh and D need a tolerance (the naive POD takes neither)")
            self.W, self.sigma = self._naive(S, int(r), int(svd_type), seed)
            self.N = self.W.shape[1]
            return
        nh, ns = S.shape
        if ns > nh:
            raise ValueError("ns > Nh (the reference's K = S S^T branch) is not supported")
        if int(svd_type) in (0, 3):
            raise ValueError("svd_type 0 / 3 (power method) is not supported by the snapshot-method POD")
        d = None
        if D is not None:
            Dn = D.detach().cpu().numpy() if _is_torch(D) else np.asarray(D, dtype=np.float64)
            if Dn.ndim == 2:
                if Dn.shape != (ns, ns) or np.any(Dn - np.diag(np.diag(Dn)) != 0):
                    raise ValueError("D must be an ns x ns diagonal matrix")
                Dn = np.diag(Dn)
            d = np.ascontiguousarray(Dn, dtype=np.float64)
        eng = default_engine()
        if _is_torch(S):
            self.W, self.sigma, self.N = eng.pod(S, r, tol, Xh=Xh, d=d, svd_type=svd_type, q=q, seed=seed,
                                                 textbook=textbook)
        else:
            self.W, self.sigma, self.N = eng.pod_host(S, r, tol, Xh=Xh, d=d, svd_type=svd_type, q=q, seed=seed,
                                                      textbook=textbook)

    @staticmethod
    def _naive(S, r: int, svd_type: int, seed: int):
        """perform_SVD on S itself (POD.cpp:42-114): SVD<method> for 0..2, rSVD(S, r, method) for 3..5."""
        method = (SVDMethod.Power, SVDMethod.Jacobi, SVDMethod.ParallelJacobi)[svd_type % 3]
        if svd_type >= 3:
            U, s, _ = rSVD(S, r, method, seed=seed)
            return U, s
        sv = SVD(S.detach().cpu().numpy() if _is_torch(S) else S, r=r if svd_type == 0 else 0, method=method, seed=seed)
        sv.compute()
        return sv.getU(), sv.getS()
