#!/usr/bin/env python3
"""bench_float_model.py: the float model's forward on the device (floatmodel.FloatEngine, csrc/float_model.hpp).

Per (dim_scale, B x L) -- 0.5 and 1.0, 32 x 4096 and 32 x 3751 frames -- device-event times of
  kernels        FloatEngine.forward_device without observers (2 + 3 * n_layers launches)
  kernels_stats  the same with the 34 observers gathered
  torch_chain    the same forward as torch ops on the GPU: torch.matmul, ssm.associative_scan (the same scan kernel) and
                 elementwise ops -- the honest comparator
  int_forward    Engine.forward_float of the w8a16 model at the same shape, for context
The arms alternate inside every repetition of one process, after a warm-up; medians, minima, maxima and every repetition are
kept.  Before timing the two float arms are compared (max relative difference of the outputs).  Once per dim_scale
synth.float_forward runs on the host at 4 x 3751 frames and is reported as frames/s with the CPUs the process may use.

The floors are taken from the code: bytes per frame = 4 * (2 * (257 + H) + n_layers * (3 H + 8 P)) (every plane a kernel
reads or writes once; weights stay on chip) against --hbm-tbs, and FLOP per frame = 2 * (2 * 257 H + n_layers * (4 P H + H H))
against --mfma-tflops (the f32 MFMA's rate is the f32 vector rate).

  python tools/bench_float_model.py [--reps 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((32, 4096), (32, 3751))
DIMS = (0.5, 1.0)


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def torch_chain(md, n_layers, dev):
    """synth.float_forward as torch ops, parameters uploaded once."""
    import torch
    from sparsernns_amd import ssm, synth

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    enc = md["encoder"]
    We, be = t(enc["encoder"]["kernel"]), t(enc["encoder"]["bias"])
    Wd, bd = t(md["decoder"]["kernel"]), t(md["decoder"]["bias"])
    layers = []
    for i in range(n_layers):
        layer = enc[f"layers_{i}"]
        lam_bar, B_bar, C = synth.zoh(layer["mixer"])
        nm = layer["norm"]
        istd = (np.float32(1) / np.sqrt(nm["var"] + np.float32(1e-5))).astype(np.float32)
        layers.append(dict(mean=t(nm["mean"]), istd=t(istd), lam=t(lam_bar), BT=t(B_bar.T.copy()), CreT=t(C.real.T.copy()),
                           CimT=t(C.imag.T.copy()), D=t(layer["mixer"]["D"]), W2=t(layer["out2"]["kernel"]), b2=t(layer["out2"]["bias"])))

    def run(x):
        h = torch.relu(torch.matmul(x, We) + be)
        for l in layers:
            u = (h - l["mean"]) * l["istd"]
            Bu = torch.matmul(u.to(torch.complex64), l["BT"])
            xs = ssm.complex_relu(ssm.associative_scan(l["lam"], Bu))
            y = 2 * (torch.matmul(xs.real, l["CreT"]) - torch.matmul(xs.imag, l["CimT"])) + l["D"] * u
            x1 = torch.relu(y)
            g = torch.sigmoid(torch.matmul(x1, l["W2"]) + l["b2"])
            h = torch.relu(x1 * g + h)
        return torch.matmul(h, Wd) + bd

    return run


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak the byte floor is taken against, TB/s")
    ap.add_argument("--mfma-tflops", type=float, default=157.3, help="f32 MFMA peak: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz")
    ap.add_argument("--no-host", action="store_true", help="skip the synth.float_forward host run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from sparsernns_amd import floatmodel, synth
    from sparsernns_amd.fxpmodel import build_regression_model

    if not torch.cuda.is_available():
        print("[bench_float_model] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    res = dict(tool="tools/bench_float_model.py", reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               unit="ms of device time per forward", hbm_tbs=args.hbm_tbs, mfma_tflops=args.mfma_tflops, workloads={}, host={})
    for dim in DIMS:
        md, qc, dims = synth.make_model(dim, calib_L=1024, state_headroom_bits=1)  # bench.py's w8a16 model
        nl, H, P = dims["n_layers"], dims["H"], dims["P"]
        feng = floatmodel.FloatEngine(md, nl)
        assert feng.on_device
        ieng = build_regression_model(md, qc, nl).engine()
        ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
        chain = torch_chain(md, nl, dev)
        bytes_per_frame = 4 * (2 * (257 + H) + nl * (3 * H + 8 * P))
        flop_per_frame = 2 * (2 * 257 * H + nl * (4 * P * H + H * H))
        if not args.no_host:
            xh = synth.make_input(4, 3751, dims["d_in"], seed=7)
            t0 = time.perf_counter()
            synth.float_forward(md, xh, nl)
            dt = time.perf_counter() - t0
            res["host"][f"dim{dim}"] = dict(frames=4 * 3751, seconds=dt, frames_per_s=4 * 3751 / dt, cpus=cpus,
                                            omp_num_threads=os.environ.get("OMP_NUM_THREADS"))
            print(f"[bench_float_model] dim {dim}: synth.float_forward on the host, 4 x 3751 frames: {dt:.2f} s = "
                  f"{4 * 3751 / dt:.3g} frames/s on {cpus} CPUs", flush=True)
        for B, L in SHAPES:
            x = torch.from_numpy(synth.make_input(B, L, dims["d_in"], seed=3)).to(dev)
            st = feng.new_stats()
            arms = dict(kernels=lambda: feng.forward_device(x), kernels_stats=lambda: feng.forward_device(x, st),
                        torch_chain=lambda: chain(x), int_forward=lambda: ieng.forward_float(x, ib, ie, check_status=False))
            for _ in range(args.warmup):
                for run in arms.values():
                    run()
            sync()
            ya, yb = arms["kernels"](), arms["torch_chain"]()
            # the complex ReLU makes the model discontinuous: the largest difference is not a rounding figure
            rel = float((ya - yb).abs().max() / yb.abs().max())
            rel_med = float((ya - yb).abs().median() / yb.abs().max())
            times = {k: [] for k in arms}
            for _ in range(args.reps):
                for k, run in arms.items():   # alternating arms
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    sync()
                    times[k].append(e0.elapsed_time(e1))
            N = B * L
            r = dict(dim_scale=dim, B=B, L=L, frames=N, H=H, P=P, bytes_per_frame=bytes_per_frame, flop_per_frame=flop_per_frame,
                     hbm_floor_ms=N * bytes_per_frame / (args.hbm_tbs * 1e12) * 1e3,
                     mfma_floor_ms=N * flop_per_frame / (args.mfma_tflops * 1e12) * 1e3, max_rel_diff_kernels_vs_torch=rel, median_rel_diff_kernels_vs_torch=rel_med,
                     **{f"{k}_ms": _stats(v) for k, v in times.items()})
            km = r["kernels_ms"]["median"]
            r["fraction_of_hbm_floor"] = r["hbm_floor_ms"] / km
            r["fraction_of_mfma_floor"] = r["mfma_floor_ms"] / km
            r["torch_over_kernels"] = r["torch_chain_ms"]["median"] / km
            r["frames_per_s"] = N / (km * 1e-3)
            res["workloads"][f"dim{dim}_B{B}_L{L}"] = r
            print(f"[bench_float_model] dim {dim} {B} x {L}: kernels {km:.3f} ms (with observers "
                  f"{r['kernels_stats_ms']['median']:.3f}), torch chain {r['torch_chain_ms']['median']:.3f} ms "
                  f"(x{r['torch_over_kernels']:.2f}), int forward {r['int_forward_ms']['median']:.3f} ms; HBM floor "
                  f"{r['hbm_floor_ms']:.3f} ms ({r['fraction_of_hbm_floor']:.0%}), MFMA floor {r['mfma_floor_ms']:.3f} ms "
                  f"({r['fraction_of_mfma_floor']:.0%}); rel diff vs torch: max {rel:.2e}, median {rel_med:.2e}", flush=True)
            del x
            torch.cuda.empty_cache()
    print(json.dumps({k: v for k, v in res.items() if k != "workloads"} | {"workloads": {
        k: {f: (w[f]["median"] if isinstance(w[f], dict) else w[f]) for f in w} for k, w in res["workloads"].items()}}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
