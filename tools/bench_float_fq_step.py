#!/usr/bin/env python3
"""bench_float_fq_step.py: what the stepping recurrence costs, and what it and the quantised weights say.

cost         Per dim_scale (0.5, 1.0) at 32 x 4096 frames, w8a8's sites all on, device-event times of
               scan   FloatEngine.forward_device with fq_spec(recurrence="scan"): the associative scan, the state sites in the gate
               step   the same with fq_spec(recurrence="step"): k_scan_fq_c64 in place of the associative scan
             alternating inside every repetition of one process, after a warm-up; medians, minima, maxima, every repetition.
             Then the scan launch alone in both arms, on layer 0's own Bu plane of that forward: s5fxp_assoc_scan_c64 against
             s5fxp_fq_scan_c64 (also on one sequence of it), next to the orientation figure 140 * L cycles at 2.4 GHz.
host         Frames per second of floatmodel.fq_scan (float64 NumPy) at 8 x 1024 frames.
sensitivity  For w8a8 and w4a8 at dim_scale 0.5, on the batches of tools/bench_float_fq.py (calibrated on 8 x 512, seed 31;
             evaluated on 8 x 512, seed 32): floatmodel.sensitivity(recurrence="step", weights=qc) -- the 34 sites, the row
             "recurrence", one row per weight group, and "all".
integer      The fully quantised float model (all sites, step mode, all weight groups) against the integer model on the
             evaluation batch: the SQNR of its output measured against Engine.forward_float's, the same figure for the plain
             float model, and per layer the share of Bu and xs elements that equal the integer model's exactly.
             Recorded, not gated: the model is synthetic (random weights), one seed.

  python tools/bench_float_fq_step.py [--reps 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (32, 4096)
DIMS = (0.5, 1.0)
RECIPE = dict(bn_stats="random", input_scale=300.0)
CLOCK_MHZ = 2400.0  # the MI355X's peak engine clock: the orientation figure's, not a measured one
CHAIN_CYCLES_PER_STEP = 140  # about 35 dependent-issue VALU operations, one per 4 cycles for one wave on a SIMD


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def _time(arms, reps, warmup):
    import torch

    for _ in range(warmup):
        for run in arms.values():
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, run in arms.items():  # alternating arms
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {f"{k}_ms": _stats(v) for k, v in times.items()}


def cost(args) -> dict:
    import torch
    from sparsernns_amd import floatmodel, synth
    from sparsernns_amd._lib import check, lib

    out = {}
    B, L = SHAPE
    clock_khz = CLOCK_MHZ * 1e3
    for dim in DIMS:
        md, qc, dims = synth.make_model(dim, quantization="w8a8", **RECIPE)
        nl, P = dims["n_layers"], dims["P"]
        eng = floatmodel.FloatEngine(md, nl)
        assert eng.on_device
        x = torch.from_numpy(synth.make_input(B, L, dims["d_in"], seed=3, scale=RECIPE["input_scale"])).to(eng.device)
        scan, step = floatmodel.fq_spec(qc, nl, recurrence="scan"), floatmodel.fq_spec(qc, nl, recurrence="step")
        st, st2 = eng.new_stats(), eng.new_stats()
        r = dict(dim_scale=dim, B=B, L=L, P=P, frames=B * L)
        r.update(_time(dict(scan=lambda: eng.forward_device(x, st, fq=scan), step=lambda: eng.forward_device(x, st2, fq=step)),
                       args.reps, args.warmup))
        r["step_over_scan"] = r["step_ms"]["median"] / r["scan_ms"]["median"]
        left = [k for k in eng.keys if k.split(".")[-1] in floatmodel.STATE_SITES
                and float(st2[eng.keys.index(k)]) * 2.0 ** floatmodel.quantiser_of(k, qc)[1] >= floatmodel.FQ_STEP_XMAX]
        r["left_domain"] = left
        # the scan launch alone, on layer 0's quantised Bu of this very forward
        lam = torch.view_as_real(torch.from_numpy(synth.zoh(md["encoder"]["layers_0"]["mixer"])[0])).to(eng.device).contiguous()
        _, _, ws = eng.forward_device(x[:, :L], trace=True, fq=step)
        NH, NP2 = B * L * eng.H, B * L * 2 * P
        bu = ws[2 * NH:2 * NH + NP2].clone()
        xs = torch.empty_like(bu)
        er, ei = (floatmodel.quantiser_of(f"l0.{k}", qc)[1] for k in floatmodel.STATE_SITES)
        stream = torch.cuda.current_stream().cuda_stream
        r["scan_launch"] = _time(dict(
            assoc=lambda: check(lib.s5fxp_assoc_scan_c64(lam.data_ptr(), bu.data_ptr(), xs.data_ptr(), None, None, B, L, P, 0, stream)),
            step=lambda: check(lib.s5fxp_fq_scan_c64(lam.data_ptr(), bu.data_ptr(), xs.data_ptr(), None, None, None, B, L, P, er, ei,
                                                     stream))), args.reps, args.warmup)
        # one sequence (P / 64 waves) and all of them: the chain's time does not depend on B while the waves fit the chip
        r["scan_launch"].update(_time(dict(step_one_sequence=lambda: check(lib.s5fxp_fq_scan_c64(
            lam.data_ptr(), bu.data_ptr(), xs.data_ptr(), None, None, None, 1, L, P, er, ei, stream))), args.reps, args.warmup))
        est = CHAIN_CYCLES_PER_STEP * L / clock_khz  # cycles / kHz = ms
        r["scan_launch"].update(waves=(B * P + 63) // 64, clock_mhz=clock_khz / 1e3, chain_estimate_ms=est,
                                step_over_estimate=r["scan_launch"]["step_ms"]["median"] / est)
        out[f"dim{dim}_B{B}_L{L}"] = r
        print(f"[bench_float_fq_step] dim {dim} {B} x {L}: scan {r['scan_ms']['median']:.3f} ms "
              f"({r['scan_ms']['min']:.3f}-{r['scan_ms']['max']:.3f}), step {r['step_ms']['median']:.3f} ms "
              f"({r['step_ms']['min']:.3f}-{r['step_ms']['max']:.3f}): x{r['step_over_scan']:.3f}; the launch alone: assoc "
              f"{r['scan_launch']['assoc_ms']['median']:.3f} ms, step {r['scan_launch']['step_ms']['median']:.3f} ms "
              f"({r['scan_launch']['step_one_sequence_ms']['median']:.3f} ms for one sequence; estimate {est:.3f} ms at "
              f"{clock_khz / 1e3:.0f} MHz)", flush=True)
        del x, ws, bu, xs
        torch.cuda.empty_cache()
    return out


def host() -> dict:
    from sparsernns_amd import floatmodel, synth

    md, qc, dims = synth.make_model(0.5, quantization="w8a8", **RECIPE)
    B, L, P = 8, 1024, dims["P"]
    rng = np.random.default_rng(5)
    lam = synth.zoh(md["encoder"]["layers_0"]["mixer"])[0]
    bu = (0.05 * (rng.standard_normal((B, L, P)) + 1j * rng.standard_normal((B, L, P)))).astype(np.complex64)
    er, ei = (floatmodel.quantiser_of(f"l0.{k}", qc)[1] for k in floatmodel.STATE_SITES)
    t0 = time.perf_counter()
    floatmodel.fq_scan(lam, bu, er, ei)
    dt = time.perf_counter() - t0
    print(f"[bench_float_fq_step] host fq_scan {B} x {L} x {P}: {B * L / dt:.0f} frames/s", flush=True)
    return dict(B=B, L=L, P=P, seconds=dt, frames_per_s=B * L / dt)


def sensitivity() -> dict:
    import torch
    from sparsernns_amd import floatmodel, synth
    from sparsernns_amd.fxparray import RoundingMode, fxp_from_fp
    from sparsernns_amd.fxpmodel import build_regression_model

    out = {}
    for q in ("w8a8", "w4a8"):
        md, _, dims = synth.make_model(0.5, quantization=q, **RECIPE)
        nl, scale = dims["n_layers"], RECIPE["input_scale"]
        eng = floatmodel.FloatEngine(md, nl)
        xc = synth.make_input(8, 512, dims["d_in"], seed=31, scale=scale)
        xe = synth.make_input(8, 512, dims["d_in"], seed=32, scale=scale)
        _, qc = floatmodel.calibrate(md, [xc], nl, quantization=q, engine=eng)
        table = floatmodel.sensitivity(md, [xe], qc, nl, engine=eng, recurrence="step", weights=qc)
        scan_all = floatmodel.sensitivity(md, [xe], qc, nl, groups={"sites": eng.keys}, engine=eng)["all"]
        left = table.pop("left_domain", [])
        # against the integer model
        full = floatmodel.FloatEngine(floatmodel.quantised_modeldict(md, qc, nl), nl)
        t = full.forward_traced(xe, fq=floatmodel.fq_spec(qc, nl, recurrence="step"))
        model = build_regression_model(md, qc, nl, store_intermediates=True)
        fx = fxp_from_fp(xe, bits=qc["encoder"]["inp_bits"], exp=qc["encoder"]["inp_exp"], signed=True, round_mode=RoundingMode.FLOOR)
        yi = model(fx).to_float().double()
        yf = build_regression_model(md, qc, nl).forward_float(torch.from_numpy(xe).to(eng.device)).double()
        assert torch.equal(yi, yf)  # the op-by-op integer model is the fused one
        sq = lambda y: float(10 * torch.log10((yi * yi).sum() / ((y.double() - yi) ** 2).sum()))
        shares = {}
        for i in range(nl):
            inter = model.encoder.seq_layers[i].mixer.last_intermediates()
            for name, key in (("Bu", "Bu_elements"), ("xs", "xs")):
                ref = inter[key].to_float().reshape(t[f"l{i}.{name}"].shape)
                shares[f"l{i}.{name}"] = float((t[f"l{i}.{name}"] == ref).double().mean())
        out[q] = dict(dim_scale=0.5, calibration="8 x 512, seed 31", evaluation="8 x 512, seed 32", input_scale=scale,
                      sqnr_db=table, left_domain=left, all_sites_scan_mode_db=scan_all,
                      against_integer=dict(fully_quantised_float_db=sq(t["out"]), plain_float_db=sq(eng.forward_device(eng._to_device(xe))),
                                           exact_share=shares))
        rows = ["recurrence"] + list(floatmodel.WEIGHT_GROUPS) + ["all"]
        print(f"[bench_float_fq_step] {q}: all sites in scan mode {scan_all:.2f} dB; " + ", ".join(f"{k} {table[k]:.2f}" for k in rows)
              + f"; against the integer model: fully quantised float {out[q]['against_integer']['fully_quantised_float_db']:.2f} dB, "
              f"plain float {out[q]['against_integer']['plain_float_db']:.2f} dB; exact shares "
              + ", ".join(f"{k} {100 * v:.1f} %" for k, v in shares.items()), flush=True)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("[bench_float_fq_step] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    res = dict(tool="tools/bench_float_fq_step.py", reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               unit="ms of device time", cost=cost(args), host_fq_scan=host(), sensitivity=sensitivity())
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"tool": res["tool"],
                      "cost": {k: dict(scan_ms=w["scan_ms"]["median"], step_ms=w["step_ms"]["median"],
                                       assoc_launch_ms=w["scan_launch"]["assoc_ms"]["median"],
                                       step_launch_ms=w["scan_launch"]["step_ms"]["median"]) for k, w in res["cost"].items()},
                      "sensitivity_all_db": {q: v["sqnr_db"]["all"] for q, v in res["sensitivity"].items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
