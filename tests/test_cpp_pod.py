"""class POD (include/POD.hpp over rsvd_pod_host_f64): tests/cpp/pod_test.cpp compiles and links against
the C ABI with the Eigen stand-in (CPU) and, on a GPU, checks the four constructors on a known answer --
S(i, j) = s_j delta_ij on 64 x 6: sigma = sort(s^2) (2 sort(s^2) with a dense Xh = 2 I, 0.2 sort(s^2) with
D = 0.1 I on top), W[:, i] = +-e_pi(i) / s_pi(i) to 1e-12, N from the reference's rule -- that a
non-diagonal D, ns > Nh and an unsupported svd_type throw, and that the naive constructor returns what
rSVD() returns.  Compiled from here with the flags of tests/cpp/Makefile (which stays as it is)."""
import os
import subprocess

import pytest

from conftest import REPO

CPP = os.path.join(REPO, "tests", "cpp")
EXE = os.path.join(CPP, "pod_test")


def _build():
    import rsvd_kamaneh_raganato_terrana_amd as R
    from rsvd_kamaneh_raganato_terrana_amd import _capi

    R.build(force=False)
    src = os.path.join(CPP, "pod_test.cpp")
    inc = os.path.join(REPO, "include")
    deps = [src, _capi.LIB_PATH] + [os.path.join(inc, f) for f in ("POD.hpp", "rSVD.hpp", "SVD_class.hpp", "rsvd.hpp",
                                                                    "rsvd_c.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        pkg = os.path.dirname(_capi.LIB_PATH)
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(CPP, "eigen_shim"),
                        "-I" + inc, src, "-L" + pkg, "-lrsvd_hip", "-Wl,-rpath,$ORIGIN/../../" + os.path.basename(pkg),
                        "-o", EXE], check=True, capture_output=True)
    return EXE


def test_cpp_pod_compiles_and_links():
    assert os.access(_build(), os.X_OK)


@pytest.mark.gpu
def test_cpp_pod_known_answer():
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
