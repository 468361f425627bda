#!/usr/bin/env python3
"""bench_i16_io.py: the int16 model boundary (s5fxp_model_forward_i16) against the int32 entry at BASELINE configs[1] (dim_scale
0.5, w8a16, B=32, L=4096), per batch, at G=1 (Engine.enqueue) and G=8 (one grouped call, as forward_batches):
  (a) the int32 entry (the yardstick: tools/disasm_compare.py shows its kernels are the parent commit's);
  (b) the int16 entry on the same values (int16 rows read by the encoder, int16 rows written by the decoder).
Every shape is warmed up first; then (a) and (b) alternate in one process, each timed with device events, for --reps
repetitions.  Reports medians and spread (p10 / p90, min / max) per batch and the gate: (b)'s median may exceed (a)'s by at
most (a)'s own p10-p90 half-width.  The outputs must be equal at this size.  Also times pinned host <-> device copies of one
batch's input and output in both dtypes (what a host-fed pipeline pays per direction).
  python tools/bench_i16_io.py [--reps 30] [--only ab] [--groups 1,8] [--dim-scale 0.5] [--out FILE.json]
--only b (or a) with few reps is the workload of a rocprofv3 --kernel-trace --stats or a counter run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _copies(torch, shape, dtype, reps):
    """Median us of a pinned H2D and D2H copy of one tensor."""
    host = torch.empty(shape, dtype=dtype).pin_memory()
    dev = torch.empty(shape, dtype=dtype, device="cuda")
    out = {}
    for name, fn in (("h2d", lambda: dev.copy_(host, non_blocking=True)), ("d2h", lambda: host.copy_(dev, non_blocking=True))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        out[name] = float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev]))
    out["MB"] = host.numel() * host.element_size() / 1e6
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="ab")
    ap.add_argument("--groups", default="1,8")
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--dim-scale", type=float, default=0.5, help="0.5 is configs[1]; other scales for kernel statistics of their twins")
    ap.add_argument("--no-copies", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from sparsernns_amd import _lib, synth
    from sparsernns_amd._lib import lib
    from sparsernns_amd.fxpmodel import build_regression_model

    torch.cuda.set_device(0)
    md, qc, dims = synth.make_model(args.dim_scale, quantization="w8a16", calib_L=1024, state_headroom_bits=1)   # bench.py's configs[1]
    eng = build_regression_model(md, qc, dims["n_layers"]).engine()
    ib, ie, B, L = eng.inp_bits, eng.inp_exp, args.B, args.L
    groups = [int(g) for g in args.groups.split(",")]
    res = dict(workload=("configs[1]: " if args.dim_scale == 0.5 else "") + f"dim_scale {args.dim_scale} w8a16 B={B} L={L}", reps=args.reps, order="a, b alternating per repetition",
               unit="us per batch (device events around each variant's enqueue)", groups={})
    for G in groups:
        x = torch.from_numpy(synth.make_input(G * B, L, eng.d_in, seed=0)).cuda()
        xi = torch.empty(x.shape, dtype=torch.int32, device="cuda")
        _lib.check(lib.s5fxp_from_fp(x.data_ptr(), xi.data_ptr(), x.numel(), ib, ie, 0, torch.cuda.current_stream().cuda_stream))
        xs = xi.to(torch.int16)
        assert torch.equal(xs.to(torch.int32), xi)
        del x
        yi = torch.empty((G * B, L, eng.d_out), dtype=torch.int32, device="cuda")
        ys = torch.empty(yi.shape, dtype=torch.int16, device="cuda")
        flags = eng.LEVEL_FLAGS[eng.level]

        def run_a():   # int32 entry, lane 0
            eng.enqueue(xi, ib, ie, yi, B, L, flags=flags, groups=G)

        def run_b():   # int16 entry, its own lane (workspace keyed by dtype)
            eng.enqueue(xs, ib, ie, ys, B, L, flags=flags, groups=G, lane=1)

        runs = {k: v for k, v in (("a", run_a), ("b", run_b)) if k in args.only}
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        for lane in (0, 1):
            if lane in eng._status:
                st = eng.check_status(lane)
                assert not (st[0] & _lib.ST_REDO), "the workload left the optimistic recurrence's range"
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)] for k in runs}
        for r in range(args.reps):
            for k, fn in runs.items():
                ev[k][r][0].record()
                fn()
                ev[k][r][1].record()
        torch.cuda.synchronize()
        out = {}
        for k in runs:
            t = np.array([a.elapsed_time(b) * 1e3 / G for a, b in ev[k]])
            out[k] = dict(median=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)),
                          min=float(t.min()), max=float(t.max()))
        if "a" in out and "b" in out:
            half = (out["a"]["p90"] - out["a"]["p10"]) / 2
            out["b_over_a"] = out["b"]["median"] / out["a"]["median"]
            out["a_p10_p90_half_width"] = half
            out["b_median_minus_a_median"] = out["b"]["median"] - out["a"]["median"]
            out["gate_b_within_a_half_width"] = bool(out["b"]["median"] <= out["a"]["median"] + half)
            same = bool(torch.equal(ys.to(torch.int32), yi))
            out["a_equals_b"] = same
            assert same, f"G={G}: the int16 entry differs from the int32 entry"
        res["groups"][str(G)] = out
        print(f"[bench_i16_io] G={G}: " + ", ".join(f"{k} {v['median']:.1f} us" for k, v in out.items() if isinstance(v, dict)), flush=True)
        del xi, xs, yi, ys
        eng._wsl.clear()
        torch.cuda.empty_cache()
    if not args.no_copies:
        res["pinned_copies_us_per_batch"] = {
            f"{name}_{str(dt).split('.')[-1]}": _copies(torch, (B, L, d), dt, args.reps)
            for name, d in (("x", eng.d_in), ("y", eng.d_out)) for dt in (torch.int32, torch.int16)}
        print("[bench_i16_io] pinned copies: " + json.dumps(res["pinned_copies_us_per_batch"]), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
