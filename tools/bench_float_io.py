#!/usr/bin/env python3
"""bench_float_io.py: what the float-in, float-out entry (s5fxp_model_forward_f32) saves at BASELINE configs[1] (dim_scale 0.5,
w8a16, B=32, L=4096), per batch, at G=1 (Engine.enqueue) and G=8 (one grouped call, as forward_batches):
  (a) the int forward alone;
  (b) the three-step route callers ran before: s5fxp_from_fp (FLOOR) + the int forward + s5fxp_to_float;
  (c) the float entry (conversions inside the encoder and decoder kernels).
Every shape is warmed up first; then (a), (b), (c) alternate in one process, each timed with device events, for --reps
repetitions.  Reports medians and spread (p10 / p90, min / max) per batch.  (b) and (c) must agree bit for bit at this size.
  python tools/bench_float_io.py [--reps 30] [--only abc] [--groups 1,8] [--out FILE.json]
--only c (or ac) with few reps is the workload of a rocprofv3 --kernel-trace --stats run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--groups", default="1,8")
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from sparsernns_amd import _lib, synth
    from sparsernns_amd._lib import lib
    from sparsernns_amd.fxpmodel import build_regression_model

    torch.cuda.set_device(0)
    md, qc, dims = synth.make_model(0.5, quantization="w8a16", calib_L=1024, state_headroom_bits=1)   # bench.py's configs[1]
    eng = build_regression_model(md, qc, dims["n_layers"]).engine()
    ib, ie, B, L = eng.inp_bits, eng.inp_exp, args.B, args.L
    groups = [int(g) for g in args.groups.split(",")]
    res = dict(workload=f"configs[1]: dim_scale 0.5 w8a16 B={B} L={L}", reps=args.reps, order="a, b, c alternating per repetition",
               unit="us per batch (device events around each variant's enqueue)", groups={})
    for G in groups:
        x = torch.from_numpy(synth.make_input(G * B, L, eng.d_in, seed=0)).cuda()
        xi = torch.empty(x.shape, dtype=torch.int32, device="cuda")
        xb = torch.empty_like(xi)
        yi = torch.empty((G * B, L, eng.d_out), dtype=torch.int32, device="cuda")
        yb_i, yb, yc = torch.empty_like(yi), torch.empty(yi.shape, dtype=torch.float32, device="cuda"), torch.empty(yi.shape, dtype=torch.float32, device="cuda")
        stream = lambda: torch.cuda.current_stream().cuda_stream
        FLOOR = 0   # S5FXP_FLOOR
        _lib.check(lib.s5fxp_from_fp(x.data_ptr(), xi.data_ptr(), x.numel(), ib, ie, FLOOR, stream()))
        flags = eng.LEVEL_FLAGS[eng.level]

        def run_a():   # int forward, lane 0
            eng.enqueue(xi, ib, ie, yi, B, L, flags=flags, groups=G)

        def run_b():   # the three steps, lane 0
            _lib.check(lib.s5fxp_from_fp(x.data_ptr(), xb.data_ptr(), x.numel(), ib, ie, FLOOR, stream()))
            eng.enqueue(xb, ib, ie, yb_i, B, L, flags=flags, groups=G)
            _lib.check(lib.s5fxp_to_float(yb_i.data_ptr(), yb.data_ptr(), yb_i.numel(), eng.out_exp, stream()))

        def run_c():   # float entry, its own lane (workspace keyed by dtype)
            eng.enqueue(x, ib, ie, yc, B, L, flags=flags, groups=G, lane=1)

        runs = {k: v for k, v in (("a", run_a), ("b", run_b), ("c", run_c)) if k in args.only}
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
        if "a" in out and "c" in out:
            out["c_over_a"] = out["c"]["median"] / out["a"]["median"]
        if "b" in out and "c" in out:
            out["c_over_b"] = out["c"]["median"] / out["b"]["median"]
            same = bool(torch.equal(yb.view(torch.int32), yc.view(torch.int32)))
            out["b_equals_c_bitwise"] = same
            assert same, f"G={G}: the float entry differs from the three-step route"
        res["groups"][str(G)] = out
        print(f"[bench_float_io] G={G}: " + ", ".join(f"{k} {v['median']:.1f} us" for k, v in out.items() if isinstance(v, dict)), flush=True)
        del x, xi, xb, yi, yb_i, yb, yc
        eng._wsl.clear()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
