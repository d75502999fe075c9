#!/usr/bin/env python3
"""POD benchmark: Engine.pod against the composition a user of the engine would write in
torch without it -- C = S^T S (torch.sparse.mm first when Xh is given), Engine.rsvd on C, W = S V / sigma --
on the same card in the same run, the two alternating.

Shapes: nh = 2^20, ns in {64, 256}, r = 32, svd_type 4, q = 2, fp32 and fp64, with and without the
tridiagonal Xh.  Call times are device-event medians after warm-up.  Stage times of the fused path (spmm,
corr + its reduction, small problem, lift) come from torch's kernel profiler in a pass of its own, by kernel
name; they are left out ("not measured") when the profiler reports no kernels.  Also recorded: GB/s over
S's bytes and the share of the fp64-MFMA peak for the correlation kernel, and the accuracy of C against an
fp64 reference for pod_corr and for torch.matmul in S's type.

    python tools/pod_bench.py [--out profiles/pod_bench.json] [--steps 20] [--warmup 5] [--nh 1048576]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

F64_MFMA_PEAK = 78.6e12  # flop/s, the figure DESIGN.md §3.3 uses for v_mfma_f64_16x16x4_f64


def tridiag(nh, dtype, torch):
    i = torch.arange(nh, dtype=torch.int64)
    rows = torch.cat([i[1:], i, i[:-1]])
    cols = torch.cat([i[:-1], i, i[1:]])
    vals = torch.cat([-torch.ones(nh - 1), 2 * torch.ones(nh), -torch.ones(nh - 1)]).to(dtype)
    return torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (nh, nh)).coalesce().to_sparse_csr().cuda()


def timed(fn, steps, warmup, torch):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stage_times(fn, reps, torch):
    """Per-call kernel time by stage (ms), from torch's profiler; None when it saw no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        stages = {"spmm": 0.0, "corr": 0.0, "small": 0.0, "lift": 0.0}
        seen = 0
        for ev in prof.key_averages():
            us = getattr(ev, "device_time_total", None)
            if us is None:
                us = getattr(ev, "cuda_time_total", 0.0)
            if not us:
                continue
            seen += 1
            name = ev.key
            if "pod_spmm" in name:
                stages["spmm"] += us
            elif "pod_corr" in name or "pod_reduce" in name:
                stages["corr"] += us
            elif "gemm_kernel" in name and "proj" not in name:
                stages["lift"] += us
            elif "Memcpy" in name or "Memset" in name or "memcpy" in name or "memset" in name:
                continue
            else:
                stages["small"] += us
        if not seen:
            return None
        return {k: v / reps / 1e3 for k, v in stages.items()}
    except Exception as e:  # the profiler is optional equipment
        return {"error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pod_bench.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nh", type=int, default=1 << 20)
    ap.add_argument("--r", type=int, default=32)
    args = ap.parse_args()

    import torch

    import rsvd_kamaneh_raganato_terrana_amd as R

    if not torch.cuda.is_available():
        raise SystemExit("pod_bench needs a GPU")
    eng = R.Engine(0)
    nh, r = args.nh, args.r
    rows = []
    for ns in (64, 256):
        for dtype in (torch.float32, torch.float64):
            g = torch.Generator(device="cuda").manual_seed(ns)
            # a decaying spectrum (0.9^j) on random directions: what a snapshot matrix looks like
            S64 = torch.randn((ns, nh), generator=g, device="cuda", dtype=torch.float64).t()
            S64 = S64 * (0.9 ** torch.arange(ns, device="cuda", dtype=torch.float64))
            S = S64.to(dtype)
            del S64
            assert S.stride(0) == 1, "S must be column-major (read in place)"
            es = S.element_size()
            for with_xh in (False, True):
                Xh = tridiag(nh, dtype, torch) if with_xh else None
                csr = None
                if with_xh:
                    csr = (Xh.crow_indices().to(torch.int32), Xh.col_indices().to(torch.int32), Xh.values())

                def fused():
                    return eng.pod(S, r, 0.05, Xh=csr, svd_type=4, q=2, seed=1, truncate=False)

                def composed():
                    T = torch.sparse.mm(Xh, S) if with_xh else S
                    C = S.t() @ T
                    _, sg, V = eng.rsvd(C, r, q=2, seed=1, check_errors=False)
                    return S @ (V / sg)

                # the two alternate, so that drift of the shared card hits both alike
                f_ms, c_ms, c_err = [], [], None
                fused()
                try:
                    composed()
                    torch.cuda.synchronize()
                except RuntimeError as e:  # e.g. a sparse product torch does not have for this layout
                    c_err = repr(e)
                for _ in range(2):
                    f_ms += timed(fused, args.steps // 2, args.warmup, torch)
                    if c_err is None:
                        c_ms += timed(composed, args.steps // 2, args.warmup, torch)
                eng.sync()
                st = stage_times(fused, 5, torch)
                tiles, chunks = eng.pod_plan(nh, ns, dtype)
                row = {
                    "nh": nh, "ns": ns, "r": r, "dtype": str(dtype).split(".")[-1], "xh": with_xh,
                    "plan": {"block_pairs": tiles, "chunks": chunks},
                    "pod_ms": statistics.median(f_ms), "pod_ms_min": min(f_ms), "pod_ms_max": max(f_ms),
                    "torch_ms": statistics.median(c_ms) if c_ms else None,
                    "torch_ms_min": min(c_ms) if c_ms else None, "torch_ms_max": max(c_ms) if c_ms else None,
                    "speedup": statistics.median(c_ms) / statistics.median(f_ms) if c_ms else None,
                    "torch_error": c_err,
                    "stages_ms": st if st is not None else "not measured",
                }
                if isinstance(st, dict) and st.get("corr"):
                    sec = st["corr"] / 1e3
                    flops = 2.0 * nh * tiles * 1024  # what the kernel issues: full 32 x 32 upper block pairs
                    row["corr_GBps_over_S"] = nh * ns * es / sec / 1e9
                    row["corr_share_of_f64_mfma_peak"] = flops / sec / F64_MFMA_PEAK
                # accuracy of C (fp32 only: the gain of accumulating in fp64)
                if dtype == torch.float32 and not with_xh:
                    Sd = S.double()
                    Cref = Sd.t() @ Sd
                    Cp = eng.pod(S, r, 0.05, svd_type=4, seed=1, truncate=False, return_corr=True)[3]
                    Ct = (S.t() @ S).double()
                    nrm = torch.linalg.norm(Cref)
                    row["C_rel_fro_pod"] = float(torch.linalg.norm(Cp - Cref) / nrm)
                    row["C_rel_fro_torch_fp32"] = float(torch.linalg.norm(Ct - Cref) / nrm)
                    del Sd, Cref
                rows.append(row)
                print(json.dumps(row), flush=True)
                del Xh, csr
            del S
            torch.cuda.empty_cache()
    eng.close()
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "f64_mfma_peak_flops": F64_MFMA_PEAK, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
