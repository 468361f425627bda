#!/usr/bin/env python3
"""bench_dim_scales.py: the N-DNS recipe at its four dim_scales (0.25, 0.5, 0.75, 1.0: H = 48, 96, 144, 192) in the launch shape
of BASELINE configs[1] -- B=32, L=4096, groups of 8 in one call, S5FXP_FWD_DEFER_REDO -- in one process, the variants alternating
per repetition:
  ds0.25, ds0.5, ds0.75, ds1.0      the default path of each model (0.5 and 1.0 run compacted to their live states)
  ds0.5_nocompact, ds1.0_nocompact  created under S5FXP_NO_COMPACT: every state slot, like 0.25 and 0.75, which cannot compact
                                    -- the like-for-like pair the ordering by work is judged on
  ds0.25_generic, ds0.75_generic    S5FXP_MODEL_FORCE_GENERIC: the generic kernels these two shapes ran before they were fused
Every variant's output is compared with the C oracle's run of the same batches before anything is timed (--check-groups of
the 8; default all).  Needs a GPU.  Reports frames/s, ms per batch (median) and the spread over repetitions (p10, p90, min, max).
  python tools/bench_dim_scales.py [--reps 12] [--only ds0.25,ds0.75] [--out FILE.json]
A build of the commit before the two shapes were fused reports them on the generic path under their default names (the
"path" field says which); --only with few reps is the workload of a rocprofv3 --kernel-trace --stats run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [("ds0.25", 0.25, {}, 0), ("ds0.5", 0.5, {}, 0), ("ds0.75", 0.75, {}, 0), ("ds1.0", 1.0, {}, 0),
            ("ds0.5_nocompact", 0.5, {"S5FXP_NO_COMPACT": "1"}, 0), ("ds1.0_nocompact", 1.0, {"S5FXP_NO_COMPACT": "1"}, 0),
            ("ds0.25_generic", 0.25, {}, "generic"), ("ds0.75_generic", 0.75, {}, "generic")]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="comma-separated variant names")
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--check-groups", type=int, default=None, help="groups compared with the oracle (default: all)")
    ap.add_argument("--state-headroom-bits", type=int, default=2,
                    help="integer bits added to the calibrated state range of every model (synth.make_model); with 1, the value of "
                         "configs[1], the 256 sequences of a call leave the int16 rungs' range at dim_scale 0.25")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("[bench_dim_scales] no GPU", file=sys.stderr)
        return 2
    from oracle import cref, fxp_oracle as O
    from sparsernns_amd import _lib, synth
    from sparsernns_amd.engine import Engine
    from sparsernns_amd.fxpmodel import build_regression_model

    torch.cuda.set_device(0)
    B, L, G = args.B, args.L, args.groups
    ncheck = G if args.check_groups is None else min(G, args.check_groups)
    want = set(args.only.split(",")) if args.only else None
    models, runs = {}, {}
    for name, ds, env, flags in VARIANTS:
        if want is not None and name not in want:
            continue
        if ds not in models:
            md, qc, dims = synth.make_model(ds, quantization="w8a16", calib_L=1024, state_headroom_bits=args.state_headroom_bits)
            model = build_regression_model(md, qc, dims["n_layers"])
            ex = model.export()
            xf = synth.make_input(G * B, L, dims["d_in"], seed=int(100 * ds))
            fx = O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
            cm = cref.CModel(ex)
            refs = [cm.forward(fx.data[g * B:(g + 1) * B], fx.bits, fx.exp)[0] for g in range(ncheck)]
            models[ds] = (ex, dims, fx, torch.from_numpy(fx.data).cuda(), refs)
        ex, dims, fx, xd, refs = models[ds]
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)          # the library reads its switches when a model is created
        try:
            eng = Engine(ex, flags=_lib.MODEL_FORCE_GENERIC if flags == "generic" else 0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        runs[name] = dict(eng=eng, x=xd, y=y, bits=fx.bits, exp=fx.exp, ds=ds, dims=dims, refs=refs)

    def enqueue(r, flags=None):
        eng = r["eng"]
        eng.enqueue(r["x"], r["bits"], r["exp"], r["y"], B, L, flags=eng.LEVEL_FLAGS[eng.level] if flags is None else flags, groups=G)

    res = dict(workload=f"N-DNS recipe w8a16, B={B} L={L}, groups of {G} per call, S5FXP_FWD_DEFER_REDO", reps=args.reps,
               order="variants alternating per repetition", checked_groups=ncheck, state_headroom_bits=args.state_headroom_bits,
               variants={})
    for name, r in runs.items():          # correctness first: every variant against the oracle
        # the engine's ladder first (a workload beyond a rung's range steps down once and the engine remembers the rung);
        # everything after it, the timed calls included, runs that rung's flags
        r["eng"].run_ladder(lambda fl: enqueue(r, fl), r["eng"].check_status)
        for _ in range(args.warmup):
            enqueue(r)
        torch.cuda.synchronize()
        st = r["eng"].check_status()
        assert not (st[0] & _lib.ST_REDO), f"{name}: the workload left the optimistic recurrence's range"
        got = r["y"].cpu().numpy()
        for g, ref in enumerate(r["refs"]):
            assert np.array_equal(got[g * B:(g + 1) * B], ref), f"{name}: group {g} differs from the oracle"
        r["path"] = {_lib.PATH_FUSED: "fused", _lib.PATH_GENERIC: "generic"}[int(st[2])]
        nl = r["dims"]["n_layers"]
        r["rungs"] = [int(v) for v in st[8 + 5:8 + 8 * nl:8]]
        r["slots"] = [int(v) for v in st[8 + 6:8 + 8 * nl:8]]
        print(f"[bench_dim_scales] {name}: {r['path']}, rungs {r['rungs']}, slots {r['slots']}, output == oracle", flush=True)
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)] for k in runs}
    for i in range(args.reps):
        for k, r in runs.items():
            ev[k][i][0].record()
            enqueue(r)
            ev[k][i][1].record()
    torch.cuda.synchronize()
    for k, r in runs.items():
        t = np.array([a.elapsed_time(b) / G for a, b in ev[k]])   # ms per batch
        fps = B * L / (t * 1e-3)
        med = float(np.median(t))
        res["variants"][k] = dict(
            dim_scale=r["ds"], H=r["dims"]["H"], P=r["dims"]["P"], path=r["path"], rungs=r["rungs"], ladder_level=int(r["eng"].level), state_slots=r["slots"],
            ms_per_batch=dict(median=med, p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)), min=float(t.min()),
                              max=float(t.max())),
            frames_per_s=dict(median=float(np.median(fps)), p10=float(np.percentile(fps, 10)), p90=float(np.percentile(fps, 90))),
            spread_rel=float((np.percentile(t, 90) - np.percentile(t, 10)) / med))
        print(f"[bench_dim_scales] {k}: {med:.3f} ms per batch, {np.median(fps) / 1e6:.2f} M frames/s, "
              f"p10-p90 spread {100 * res['variants'][k]['spread_rel']:.1f} %", flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
