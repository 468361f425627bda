#!/usr/bin/env python3
"""bench_float_clips.py: the float model over clips of different lengths against the two routes there were.

Workloads: n in 256, 1024 clips at dim_scale 0.5 and 1.0, lengths seeded-uniform in [33, 513] frames (PCG64(1000 + n), the
seeding of tools/bench_clips.py), padded to (n, Lmax, 257) with zeros.  Arms, device-event times of one pass over all clips:
  clips        FloatEngine.forward_clips_device with the 34 absmax observers
  clips_hist   the same with the 34 x 64 histograms gathered
  padded       FloatEngine.forward_device on the padded (n, Lmax) batch, observers on -- fast, and wrong for calibration:
               every padding frame is observed
  padded_hist  the same with histograms
  per_clip     one FloatEngine.forward_device per clip, observers on -- correct, 11 launches per clip
alternating inside every repetition of one process, after a warm-up; medians, minima, maxima, every repetition.  Before
timing, the clip launch is compared with the per-clip forwards: outputs, observers and histograms must be identical.

calibration  On the same sets: calibrate_clipped(p = 1e-3) through the padded route and through the clip route; the histogram
             row sums (range_report's denominators) of both, and how many of the 34 effective observers differ.

Recorded, not gated.
  python tools/bench_float_clips.py [--reps 20] [--warmup 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = (0.5, 1.0)
COUNTS = (256, 1024)
P_CLIP = 1e-3


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def lengths(n):
    rng = np.random.Generator(np.random.PCG64(1000 + n))
    return [int(v) for v in rng.integers(33, 514, n)]


def workload(args, dim, n) -> dict:
    import torch
    from sparsernns_amd import floatmodel, synth

    md, _, dims = synth.make_model(dim, calib_L=1024, state_headroom_bits=1)
    nl = dims["n_layers"]
    eng = floatmodel.FloatEngine(md, nl)
    assert eng.on_device
    lens = lengths(n)
    Lmax = max(lens)
    base = synth.make_input(64, Lmax, dims["d_in"], seed=17)  # 64 distinct clips, repeated with other lengths
    x = torch.from_numpy(base).to(eng.device).repeat((n + 63) // 64, 1, 1)[:n].contiguous()
    for e, l in enumerate(lens):
        x[e, l:] = 0
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=eng.device)
    singles = [x[e:e + 1, :l].contiguous() for e, l in enumerate(lens)]
    y = torch.empty_like(x)
    st = {k: eng.new_stats() for k in ("clips", "clips_hist", "padded", "padded_hist", "per_clip")}
    hd = {k: eng.new_hist() for k in ("clips_hist", "padded_hist")}

    def per_clip():
        for c in singles:
            eng.forward_device(c, st["per_clip"])

    arms = dict(clips=lambda: eng.forward_clips_device(x, lens_dev, st["clips"], out=y),
                clips_hist=lambda: eng.forward_clips_device(x, lens_dev, st["clips_hist"], hd["clips_hist"], out=y),
                padded=lambda: eng.forward_device(x, st["padded"]),
                padded_hist=lambda: eng.forward_device(x, st["padded_hist"], hist_dev=hd["padded_hist"]),
                per_clip=per_clip)
    # identity first: the clip launch against the per-clip forwards
    s1, h1, s2, h2 = eng.new_stats(), eng.new_hist(), eng.new_stats(), eng.new_hist()
    yc = eng.forward_clips_device(x, lens_dev, s1, h1)
    for e, c in enumerate(singles):
        ye = eng.forward_device(c, s2, hist_dev=h2)
        assert torch.equal(ye[0].view(torch.int32), yc[e, :lens[e]].view(torch.int32)), e
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(h1, h2)
    for _ in range(args.warmup):
        for run in arms.values():
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, run in arms.items():  # alternating arms
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    tpc = (Lmax + 31) // 32
    r = dict(dim_scale=dim, n=n, Lmax=Lmax, frames=int(sum(lens)), padded_frames=n * Lmax, tiles=n * tpc,
             tiles_with_rows=int(sum((l + 31) // 32 for l in lens)), **{f"{k}_ms": _stats(v) for k, v in times.items()})
    med = lambda k: r[f"{k}_ms"]["median"]
    r.update(clips_over_padded=med("clips") / med("padded"), clips_hist_over_padded_hist=med("clips_hist") / med("padded_hist"),
             per_clip_over_clips=med("per_clip") / med("clips"))
    # what padding does to a calibration
    xp = x.cpu().numpy()
    sp, hp, ep, _ = floatmodel.calibrate_clipped(md, [xp], nl, P_CLIP, engine=eng)
    sc, hc, ec, _ = floatmodel.calibrate_clipped(md, [(xp, lens)], nl, P_CLIP, engine=eng)
    differ = [k for k in ec if ec[k] != ep[k]]
    r["calibration"] = dict(clip_fraction=P_CLIP, row_sums_padded={k: int(v.sum()) for k, v in hp.items()},
                            row_sums_clips={k: int(v.sum()) for k, v in hc.items()},
                            absmax_observers_that_differ=[k for k in sc if sc[k] != sp[k]],
                            effective_observers_that_differ=differ, n_effective_observers_that_differ=len(differ))
    print(f"[bench_float_clips] dim {dim} n {n} (Lmax {Lmax}, {r['frames']} of {r['padded_frames']} frames): clips "
          f"{med('clips'):.3f} ms, + hist {med('clips_hist'):.3f}; padded {med('padded'):.3f}, + hist {med('padded_hist'):.3f}; "
          f"per clip {med('per_clip'):.3f}; clips / padded x{r['clips_over_padded']:.3f}, per clip / clips "
          f"x{r['per_clip_over_clips']:.2f}; {len(differ)} of {len(ec)} effective observers differ through padding", flush=True)
    return r


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("[bench_float_clips] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    res = dict(tool="tools/bench_float_clips.py", reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               unit="ms of device time per pass over all clips", lengths="uniform in [33, 513] frames, PCG64(1000 + n)",
               workloads={f"ds{dim}_n{n}": workload(args, dim, n) for dim in DIMS for n in COUNTS})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: {f: (w[f]["median"] if f.endswith("_ms") else w[f]) for f in w if f != "calibration"}
                      for k, w in res["workloads"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
