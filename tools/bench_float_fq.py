#!/usr/bin/env python3
"""bench_float_fq.py: what fake quantisation costs, and what the sensitivity table says.

cost         Per dim_scale (0.5, 1.0) at 32 x 4096 frames, device-event times of
               plain  FloatEngine.forward_device with the 34 absmax observers (the kernels without fake quantisation)
               fq     the same with all 34 sites on (the k_*_fq kernels), w8a8's fields
             alternating inside every repetition of one process, after a warm-up; medians, minima, maxima, every repetition.
             Before timing an all-off spec is compared with no spec: y and the observers must be bit-identical.
sensitivity  For w8a8 and w4a8 at dim_scale 0.5 (the models built as tests/test_gpu_parity.py's 8-bit recipes build them:
             bn_stats="random", input_scale=300): the fxp_qconfig calibrated on one 8 x 512 batch, and on a second 8 x 512 batch
             floatmodel.sensitivity: per-site output SQNR and "all".  Next to it the SI-SNR of audio.validate_float with and
             without the full spec on synthetic audio of the same length (8 clips of 512 frames).
             Recorded, not gated: the model is synthetic (random weights), one seed, and its lexicographic complex ReLU makes
             output SQNR a blunt instrument.

  python tools/bench_float_fq.py [--reps 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (32, 4096)
DIMS = (0.5, 1.0)
RECIPE = dict(bn_stats="random", input_scale=300.0)


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def cost(args) -> dict:
    import torch
    from sparsernns_amd import floatmodel, synth

    out = {}
    B, L = SHAPE
    for dim in DIMS:
        md, qc, dims = synth.make_model(dim, quantization="w8a8", **RECIPE)
        nl = dims["n_layers"]
        eng = floatmodel.FloatEngine(md, nl)
        assert eng.on_device
        x = torch.from_numpy(synth.make_input(B, L, dims["d_in"], seed=3, scale=RECIPE["input_scale"])).to(eng.device)
        spec, off = floatmodel.fq_spec(qc, nl), floatmodel.fq_spec(qc, nl, [])
        st, st2 = eng.new_stats(), eng.new_stats()
        arms = dict(plain=lambda: eng.forward_device(x, st), fq=lambda: eng.forward_device(x, st2, fq=spec))
        for _ in range(args.warmup):
            for run in arms.values():
                run()
        torch.cuda.synchronize()
        s0, s1 = eng.new_stats(), eng.new_stats()
        ya, yb = eng.forward_device(x, s0), eng.forward_device(x, s1, fq=off)
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))
        yq = arms["fq"]()
        sqnr = float(10 * torch.log10((ya.double() ** 2).sum() / ((yq.double() - ya.double()) ** 2).sum()))
        times = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, run in arms.items():  # alternating arms
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        r = dict(dim_scale=dim, B=B, L=L, frames=B * L, sites_on=int((spec["bits"] != 0).sum()), output_sqnr_db=sqnr,
                 **{f"{k}_ms": _stats(v) for k, v in times.items()})
        r["fq_over_plain"] = r["fq_ms"]["median"] / r["plain_ms"]["median"]
        out[f"dim{dim}_B{B}_L{L}"] = r
        print(f"[bench_float_fq] dim {dim} {B} x {L}: plain {r['plain_ms']['median']:.3f} ms "
              f"({r['plain_ms']['min']:.3f}-{r['plain_ms']['max']:.3f}), all sites on {r['fq_ms']['median']:.3f} ms "
              f"({r['fq_ms']['min']:.3f}-{r['fq_ms']['max']:.3f}): x{r['fq_over_plain']:.3f}", flush=True)
        del x
        torch.cuda.empty_cache()
    return out


def sensitivity() -> dict:
    import torch
    from sparsernns_amd import audio, floatmodel, synth

    out = {}
    for q in ("w8a8", "w4a8"):
        md, _, dims = synth.make_model(0.5, quantization=q, **RECIPE)
        nl, scale = dims["n_layers"], RECIPE["input_scale"]
        eng = floatmodel.FloatEngine(md, nl)
        xc = synth.make_input(8, 512, dims["d_in"], seed=31, scale=scale)
        xe = synth.make_input(8, 512, dims["d_in"], seed=32, scale=scale)
        _, qc = floatmodel.calibrate(md, [xc], nl, quantization=q, engine=eng)
        table = floatmodel.sensitivity(md, [xe], qc, nl, engine=eng)
        spec = floatmodel.fq_spec(qc, nl)
        rng = np.random.default_rng(33)
        T = 512 + 128 * (512 - 1)  # 512 frames
        clean = (0.05 * rng.standard_normal((8, T))).astype(np.float32)
        noisy = clean + (0.05 * rng.standard_normal((8, T))).astype(np.float32)
        nd, cd = torch.from_numpy(noisy).to(eng.device), torch.from_numpy(clean).to(eng.device)
        gain = float(np.abs(xc).mean()) / float(audio.stft_mag(nd).abs().mean())  # the STFT is linear: the model sees magnitudes
        nd, cd = nd * gain, cd * gain                                             # of the size it was calibrated on
        snr0 = audio.validate_float(eng, nd, cd)[1].double().cpu().numpy()
        snr1 = audio.validate_float(eng, nd, cd, fq=spec)[1].double().cpu().numpy()
        worst = sorted((v, k) for k, v in table.items() if k != "all")[:5]
        out[q] = dict(dim_scale=0.5, calibration="8 x 512, seed 31", evaluation="8 x 512, seed 32", input_scale=scale,
                      quantisers={k: list(floatmodel.quantiser_of(k, qc)) for k in eng.keys}, sqnr_db=table,
                      si_snr_db=dict(audio="8 x 512 frames of white noise on white noise, seed 33, scaled so that the mean STFT "
                                     "magnitude is the calibration batch's mean |x|", gain=gain, plain_mean=float(snr0.mean()),
                                     fq_mean=float(snr1.mean()), difference_mean=float((snr1 - snr0).mean()),
                                     plain=[float(v) for v in snr0], fq=[float(v) for v in snr1]))
        print(f"[bench_float_fq] {q}: all sites {table['all']:.2f} dB; lowest " + ", ".join(f"{k} {v:.2f}" for v, k in worst)
              + f"; SI-SNR {snr0.mean():.3f} dB plain, {snr1.mean():.3f} dB fake-quantised", flush=True)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("[bench_float_fq] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    res = dict(tool="tools/bench_float_fq.py", reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               unit="ms of device time per forward", cost=cost(args), sensitivity=sensitivity())
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"tool": res["tool"], "cost": {k: {f: (w[f]["median"] if isinstance(w[f], dict) else w[f]) for f in w}
                                                    for k, w in res["cost"].items()},
                      "sensitivity_all_db": {q: v["sqnr_db"]["all"] for q, v in res["sensitivity"].items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
