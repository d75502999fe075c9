"""The byte patterns tests/test_gpu_workspace.py fills the workspace with before a run (a plain
helper module; tests/test_workspace_patterns.py asserts on the CPU what each decodes to).

  zero  0x00  every aligned word is 0 (the control)
  nan   0xFF  NaN as fp64, fp32, bf16 and e4m3fn; -1 as int32; 2^32 - 1 as a counter
  big   0x4B  finite, non-zero and large: 5.2e54 (fp64), 1.33e7 (fp32 and bf16), 5.5 (e4m3fn);
              1263225675 as int32
"""
PATTERNS = {"zero": 0x00, "nan": 0xFF, "big": 0x4B}
