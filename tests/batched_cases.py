"""Cases of the fused batched rSVD (csrc/batched.hip, batched_rsvd_kernel<T, LP, panels in LDS, compress>):
the case table and the host-only queries that place a shape on an instantiation (a plain helper module in
the style of dense_cases.py, shared by test_batched_cases.py on the CPU and test_gpu_batched.py /
test_gpu_compress.py / test_gpu_workspace.py on the GPU).

One row per case, (m, n, l, q), each the smallest shape found that reaches its path.  Where a row runs is
not written down here: it is derived from rsvd_batched_is_fused and rsvd_batched_workspace_bytes (host
arithmetic, csrc/batched_run.cpp plan_fused):

  LP        16 ceil(l / 16): 16 and 32 run 256 threads, 48 runs 384 (six waves, three rows per Jacobi
            thread), 64 runs 512
  location  "lds" exactly when the reported workspace is the 256-byte floor: the l x l area and both panels,
            (m + n) l sizeof(T) rounded up to 256, fit in the 160 KiB budget; else "ws"

Eleven (type, LP, location) combinations can be reached (REACHABLE; with and without the compress tail, 22
of the kernel's 32 instantiations): fp64 keeps its panels in LDS for every shape at LP 16 and 32
(m + n <= 512) and can leave it at LP 48 and 64; fp32 leaves it at LP 64 only.  test_batched_cases.py
asserts that the table covers all of them and that each budget pair straddles the first n past the budget.
"""
import ctypes

REACHABLE = (
    ("f64", 16, "lds"), ("f64", 32, "lds"), ("f64", 48, "lds"), ("f64", 64, "lds"),
    ("f64", 48, "ws"), ("f64", 64, "ws"),
    ("f32", 16, "lds"), ("f32", 32, "lds"), ("f32", 48, "lds"), ("f32", 64, "lds"),
    ("f32", 64, "ws"),
)

CASES = [
    (9, 7, 1, 1),        # l = 1
    (5, 1, 1, 0),        # n = l = 1, q = 0
    (50, 40, 17, 1),     # odd l, 15 padding columns
    (40, 31, 31, 2),     # odd l = n = LP - 1
    (90, 50, 33, 2),     # odd l, first width on the 384-thread kernel
    (70, 61, 48, 1),     # l = LP = 48
    (150, 124, 48, 1),   # last shape inside the fp64 LDS budget
    (150, 125, 48, 1),   # first shape past the fp64 LDS budget
    (200, 100, 47, 1),   # odd l, more rows than one scale round
    (70, 60, 49, 1),     # fp64 LP 64 in LDS (possible only for l <= 59)
    (64, 64, 64, 1),     # l = m = n = LP
    (100, 63, 63, 1),    # odd l = n = 63
    (256, 110, 64, 1),   # last shape inside the fp32 LDS budget
    (256, 111, 64, 1),   # first shape past the fp32 LDS budget
]

# (type, inside, past): neighbours in n at fixed (m, l, q), the first with its panels in LDS, the second not
BUDGET_PAIRS = [
    ("f64", (150, 124, 48, 1), (150, 125, 48, 1)),
    ("f32", (256, 110, 64, 1), (256, 111, 64, 1)),
]

# the rows the compress tail runs on (test_gpu_compress.py)
COMPRESS_CASES = [(50, 40, 17, 1), (40, 31, 31, 2), (90, 50, 33, 2), (200, 100, 47, 1), (70, 60, 49, 1),
                  (64, 64, 64, 1), (100, 63, 63, 1), (256, 111, 64, 1)]

LDS_FLOOR = 256  # what rsvd_batched_workspace_bytes reports when nothing of the workspace is used


def case_id(c):
    return "{}x{}-l{}-q{}".format(*c)


def lp_of(l):
    return 16 * ((l + 15) // 16)


def _lib():
    from rsvd_kamaneh_raganato_terrana_amd import _capi

    return _capi, _capi.lib()


def _descs(m, n, l, q, f32, batch):
    _capi, _ = _lib()
    d = _capi.Desc(m=m, n=n, lda=m, l=l, q=q, dtype=_capi.F32 if f32 else _capi.F64, method=_capi.SVD_JACOBI,
                   qr_mode=_capi.QR_AUTO, flags=0, seed=0, a_scale=1.0)
    b = _capi.BatchDesc(count0=batch, count1=1, a_stride0=m * n, a_stride1=0, omega_stride=0, u_stride=m * l,
                        s_stride=l, v_stride=n * l)
    return d, b


def is_fused(m, n, l, q, f32, batch=2):
    _, L = _lib()
    d, b = _descs(m, n, l, q, f32, batch)
    return int(L.rsvd_batched_is_fused(ctypes.byref(d), ctypes.byref(b)))


def workspace_bytes(m, n, l, q, f32, batch=2):
    _, L = _lib()
    d, b = _descs(m, n, l, q, f32, batch)
    nb = ctypes.c_size_t(0)
    st = L.rsvd_batched_workspace_bytes(ctypes.byref(d), ctypes.byref(b), ctypes.byref(nb))
    assert st == 0, (m, n, l, q, f32, st)
    return nb.value


def placement(m, n, l, q, f32, batch=2):
    """(type, LP, location) of the instantiation the queries put this shape on."""
    loc = "lds" if workspace_bytes(m, n, l, q, f32, batch) == LDS_FLOOR else "ws"
    return ("f32" if f32 else "f64"), lp_of(l), loc
