#!/usr/bin/env python
"""Fused batched rSVD against the loop of Engine.rsvd over the same tiles (the only way to do a
batch without rsvd_run_batched), on ONE handle, alternating, in one process.

Per shape: a warm-up of both ways, then --reps timed repetitions of each, alternating fused / loop;
every repetition is bracketed by device events on the handle's stream and ends in a synchronise.
Writes one JSON file (--out): per shape the repetitions in ms, their median / min / max, the speed-up
of the medians, whether the margin exceeds the spread (the slowest fused repetition is faster than
the fastest loop repetition) and (2q + 2) B m n sizeof(T) -- the bytes of A one batch reads -- for the
bytes/s of a kernel time measured apart (rocprofv3 --kernel-trace --stats -- python
tools/batched_bench.py --fused-only ...).

    python tools/batched_bench.py --out profiles/batched_bench.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, kind, m, n, tile_m, tile_n, batch, l, q, dtype)
SHAPES = [
    ("4096sq_f32_32x32_tiles_128", "tiles", 4096, 4096, 128, 128, 1024, 16, 2, "float32"),
    ("4096sq_f32_64x64_tiles_64", "tiles", 4096, 4096, 64, 64, 4096, 8, 2, "float32"),
    ("256_f64_256sq", "batch", 256, 256, 256, 256, 256, 32, 2, "float64"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="batched_bench.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true", help="skip the loops (for a kernel-trace run)")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")

    import torch

    import rsvd_kamaneh_raganato_terrana_amd as R

    eng = R.Engine(0)
    stream = torch.cuda.current_stream(0)
    want = [s for s in args.shapes.split(",") if s]
    results = []
    for name, kind, m, n, tm, tn, batch, l, q, dt in SHAPES:
        if want and name not in want:
            continue
        tdt = getattr(torch, dt)
        gen = torch.Generator(device="cuda").manual_seed(1234)
        if kind == "tiles":
            A = torch.randn((n, m), generator=gen, device="cuda", dtype=tdt).t()  # column-major m x n
            gr, gc = m // tm, n // tn
            tiles = [A[i * tm:(i + 1) * tm, j * tn:(j + 1) * tn] for j in range(gc) for i in range(gr)]  # b = i + gr j

            def fused():
                return eng.rsvd_tiles(A, tm, tn, l, q=q, seed=7, check_errors=False)
        else:
            A = torch.randn((batch, n, m), generator=gen, device="cuda", dtype=tdt).transpose(1, 2)
            tiles = [A[b] for b in range(batch)]

            def fused():
                return eng.rsvd_batched(A, l, q=q, seed=7, check_errors=False)
        assert len(tiles) == batch
        assert eng.batched_is_fused(tm, tn, l, tdt, q=q, batch=batch) == 1, name

        def loop():
            out = None
            for b, T in enumerate(tiles):
                out = eng.rsvd(T, l, q=q, seed=7 + b, check_errors=False)
            return out

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            eng.sync()
            return e0.elapsed_time(e1)

        ways = [("fused", fused)] + ([] if args.fused_only else [("loop", loop)])
        for _, fn in ways:  # warm-up: workspace, code objects, clocks
            timed(fn)
        ms = {k: [] for k, _ in ways}
        for _ in range(args.reps):
            for k, fn in ways:
                ms[k].append(timed(fn))
        elem = 8 if dt == "float64" else 4
        rec = {"shape": name, "m": tm, "n": tn, "batch": batch, "l": l, "q": q, "dtype": dt, "reps": args.reps,
               "a_bytes_read": (2 * q + 2) * batch * tm * tn * elem}
        for k in ms:
            rec[k + "_ms"] = ms[k]
            rec[k + "_median_ms"] = statistics.median(ms[k])
            rec[k + "_min_ms"], rec[k + "_max_ms"] = min(ms[k]), max(ms[k])
        if "loop" in ms:
            rec["speedup_of_medians"] = rec["loop_median_ms"] / rec["fused_median_ms"]
            rec["margin_exceeds_spread"] = rec["fused_max_ms"] < rec["loop_min_ms"]
        rec["fused_end_to_end_bytes_per_s"] = rec["a_bytes_read"] / (rec["fused_median_ms"] * 1e-3)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    eng.close()
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
