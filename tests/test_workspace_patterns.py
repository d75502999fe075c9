"""What the workspace fill patterns of tests/ws_patterns.py decode to, in every type the engines keep
in the workspace (fp64 / fp32 / bf16 / e4m3fn panels, int32 flags, uint32 counters): `nan` must be
NaN in all four float types, `big` finite, non-zero and large in all of them, `zero` zero.  A later
change of pattern then cannot silently lose what test_gpu_workspace.py relies on."""
import math

import numpy as np
import pytest

from ws_patterns import PATTERNS

FLOATS = ("float64", "float32", "bfloat16", "float8_e4m3fn")


def _decode(byte, dtype_name):
    import torch

    raw = torch.full((16,), byte, dtype=torch.uint8)
    v = raw.view(getattr(torch, dtype_name))
    assert v.numel() >= 1
    vals = v.to(torch.float64).numpy() if v.is_floating_point() else v.numpy()
    assert (vals == vals[0]).all() or np.isnan(vals).all()  # every aligned word reads the same
    return vals[0]


def test_pattern_table():
    assert PATTERNS == {"zero": 0x00, "nan": 0xFF, "big": 0x4B}


@pytest.mark.parametrize("dt", FLOATS)
def test_zero_nan_big_as_floats(dt):
    assert _decode(PATTERNS["zero"], dt) == 0.0
    assert math.isnan(_decode(PATTERNS["nan"], dt))
    big = _decode(PATTERNS["big"], dt)
    assert math.isfinite(big) and big > 5.0
    want = {"float64": 5.2e54, "float32": 1.33e7, "bfloat16": 1.33e7, "float8_e4m3fn": 5.5}[dt]
    assert abs(big - want) <= 0.01 * want, (dt, big)


def test_patterns_as_integers():
    assert _decode(PATTERNS["zero"], "int32") == 0
    assert _decode(PATTERNS["nan"], "int32") == -1
    assert np.uint32(np.int32(_decode(PATTERNS["nan"], "int32"))) == 2 ** 32 - 1  # a counter past any target
    assert _decode(PATTERNS["big"], "int32") == 1263225675
