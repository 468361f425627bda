#!/usr/bin/env python3
"""bench_float_hist.py: what the exponent histograms cost, and what a clip-aware calibration buys.

cost      Per dim_scale (0.5, 1.0) at 32 x 4096 frames, device-event times of
            stats       FloatEngine.forward_device with the 34 absmax observers (the kernels without the histogram)
            stats_hist  the same with the 34 x 64 histogram gathered (the k_*_hist kernels)
          alternating inside every repetition of one process, after a warm-up; medians, minima, maxima, every repetition.
          Before timing the two arms are compared: y and the observers must be bit-identical, the row sums the element counts.
          --second-lib PATH measures the same two arms on another build of the library (a fresh child process that loads it
          through S5FXP_LIB), e.g. EXTRA_FLAGS=-DS5_FM_HIST_COPIES=1 tools/build_variant.sh hist1 for the single-copy scheme.
clipping  For w8a16, w8a8 and w4a8 at dim_scale 0.5 (the 8-bit models built as tests/test_gpu_parity.py's ndns05_w4a8 recipe
          builds them: bn_stats="random", input_scale=300): calibrate_clipped on one 8 x 512 batch with clip_fraction in
          {0, 1e-4, 1e-3, 1e-2}, an Engine from each fxp_qconfig, and on a second 8 x 512 batch the output SQNR of
          Engine.forward_float against FloatEngine.forward, with range_report's largest `saturates` on both batches.
          Recorded, not gated: the model is synthetic (random weights), and its lexicographic complex ReLU makes output SQNR
          a blunt instrument.

  python tools/bench_float_hist.py [--reps 20] [--second-lib PATH] [--out FILE.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (32, 4096)
DIMS = (0.5, 1.0)
CLIPS = (0.0, 1e-4, 1e-3, 1e-2)
RECIPES = {"w8a16": dict(), "w8a8": dict(bn_stats="random", input_scale=300.0), "w4a8": dict(bn_stats="random", input_scale=300.0)}


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def cost(args) -> dict:
    import torch
    from sparsernns_amd import floatmodel, synth

    out = {}
    B, L = SHAPE
    for dim in DIMS:
        md, _, dims = synth.make_model(dim, calib_L=1024, state_headroom_bits=1)
        eng = floatmodel.FloatEngine(md, dims["n_layers"])
        assert eng.on_device
        x = torch.from_numpy(synth.make_input(B, L, dims["d_in"], seed=3)).to(eng.device)
        st, st2, hd = eng.new_stats(), eng.new_stats(), eng.new_hist()
        arms = dict(stats=lambda: eng.forward_device(x, st), stats_hist=lambda: eng.forward_device(x, st2, hist_dev=hd))
        for _ in range(args.warmup):
            for run in arms.values():
                run()
        torch.cuda.synchronize()
        ya, yb = arms["stats"](), arms["stats_hist"]()
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)) and torch.equal(st.view(torch.int32), st2.view(torch.int32))
        h1 = eng.new_hist()
        eng.forward_device(x, None, hist_dev=h1)
        N = B * L
        want = [N * (257 if k in ("encoder.inp", "decoder.out") else dims["P"] if k.split(".")[-1] in ("Bu_re", "Bu_im", "x_re", "x_im")
                     else dims["H"]) for k in eng.keys]
        assert h1.sum(dim=1).tolist() == want
        times = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, run in arms.items():  # alternating arms
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        r = dict(dim_scale=dim, B=B, L=L, frames=N, values_counted=int(sum(want)), bins_in_use=int((h1.sum(dim=0) > 0).sum()),
                 **{f"{k}_ms": _stats(v) for k, v in times.items()})
        r["hist_over_stats"] = r["stats_hist_ms"]["median"] / r["stats_ms"]["median"]
        out[f"dim{dim}_B{B}_L{L}"] = r
        print(f"[bench_float_hist] {args.scheme}: dim {dim} {B} x {L}: stats {r['stats_ms']['median']:.3f} ms "
              f"({r['stats_ms']['min']:.3f}-{r['stats_ms']['max']:.3f}), stats + hist {r['stats_hist_ms']['median']:.3f} ms "
              f"({r['stats_hist_ms']['min']:.3f}-{r['stats_hist_ms']['max']:.3f}): x{r['hist_over_stats']:.3f}", flush=True)
        del x
        torch.cuda.empty_cache()
    return out


def clipping() -> dict:
    import torch
    from sparsernns_amd import floatmodel, synth
    from sparsernns_amd.fxpmodel import build_regression_model

    out = {}
    for q, kw in RECIPES.items():
        md, _, dims = synth.make_model(0.5, quantization=q, **kw)
        nl, scale = dims["n_layers"], kw.get("input_scale", 1.0)
        feng = floatmodel.FloatEngine(md, nl)
        xc = synth.make_input(8, 512, dims["d_in"], seed=31, scale=scale)
        xe = synth.make_input(8, 512, dims["d_in"], seed=32, scale=scale)
        he: dict = {}
        yf = feng.forward(xe, hist=he).astype(np.float64)
        rows = []
        for p in CLIPS:
            stats, hist, eff, qc = floatmodel.calibrate_clipped(md, [xc], nl, p, quantization=q, engine=feng)
            ieng = build_regression_model(md, qc, nl).engine()
            yq = ieng.forward_float(torch.from_numpy(xe).to(ieng.device), qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"])
            err = yq.cpu().numpy().astype(np.float64) - yf
            sqnr = float(10 * np.log10((yf ** 2).sum() / (err ** 2).sum()))
            sat_c = max((r["saturates"], k) for k, r in floatmodel.range_report(hist, qc, nl).items())
            sat_e = max((r["saturates"], k) for k, r in floatmodel.range_report(he, qc, nl).items())
            rows.append(dict(clip_fraction=p, observers_changed=sum(eff[k] != stats[k] for k in stats), sqnr_db=sqnr,
                             max_saturates_calibration=dict(share=sat_c[0], key=sat_c[1]),
                             max_saturates_second_batch=dict(share=sat_e[0], key=sat_e[1])))
            print(f"[bench_float_hist] {q} clip {p:g}: {rows[-1]['observers_changed']} observers changed, output SQNR {sqnr:.2f} dB, "
                  f"largest saturating share {sat_c[0]:.2e} ({sat_c[1]}) on the calibration batch, {sat_e[0]:.2e} ({sat_e[1]}) on "
                  "the second", flush=True)
        out[q] = dict(dim_scale=0.5, calibration="8 x 512, seed 31", evaluation="8 x 512, seed 32", input_scale=scale, rows=rows)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scheme", default="16 private LDS copies per workgroup, chosen by lane & 15, laid out [bin][copy]")
    ap.add_argument("--second-lib", default=None, help="another build of libs5fxp.so to run the cost arms on")
    ap.add_argument("--second-scheme", default="one LDS copy per workgroup (-DS5_FM_HIST_COPIES=1)")
    ap.add_argument("--cost-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("[bench_float_hist] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    res = dict(tool="tools/bench_float_hist.py", reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               unit="ms of device time per forward", scheme=args.scheme, cost=cost(args))
    if args.second_lib:
        env = dict(os.environ, S5FXP_LIB=os.path.abspath(args.second_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--cost-only", "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--scheme", args.second_scheme]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        sys.stdout.write("".join(l + "\n" for l in p.stdout.splitlines() if l.startswith("[bench_float_hist]")))
        if p.returncode:
            sys.stderr.write(p.stderr)
            return p.returncode
        res["second_scheme"] = dict(scheme=args.second_scheme, cost=json.loads(p.stdout.splitlines()[-1])["cost"])
    if not args.cost_only:
        res["clipping"] = clipping()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.cost_only:  # the child of --second-lib: everything, for the parent to keep
        print(json.dumps(res))
        return 0
    print(json.dumps({k: v for k, v in res.items() if k not in ("cost", "second_scheme")} | {"cost": {
        k: {f: (w[f]["median"] if isinstance(w[f], dict) else w[f]) for f in w} for k, w in res["cost"].items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
