#!/usr/bin/env python3
"""What the stage-by-stage comparison of a ragged clip list costs, one call against the per-clip loop.

dim_scale 0.5 and 1.0, the synthetic w8a16 model, n = 16, 256 and 1024 clips of 33 .. 513 frames (seeded).  Two arms on the same
clips, alternating in one process, each timed with device events around it AND on the host's wall clock (both end in the read
of the records, so both include every sync the arm needs):
  clips   verify.compare_clips(by="stage"): one integer launch, the float model's 2 + 3 n_layers launches, two comparison
          launches, one read of the status words, one of the records;
  loop    verify.compare_engines(clip[None], by="stage") clip after clip: the only way before the clip entries had trace
          planes, and code they do not touch -- the yardstick.
Next to them, device-event ms:
  Engine.clips_traced against Engine.clips on the same launch (the price of storing 11 planes per layer), and
  s5fxp_stage_err_clips against s5fxp_stage_err on the padded boxes of the same extents (the price of the mask; the unmasked
  call also reads the padding, which is zero-filled for it).
Equal results: the clips arm's counts equal the sum of the loop's for every stage, at every size.

Writes the JSON given with --out and prints one summary line.  Exit status 1 when, at n = 256, the clips arm is not faster
than the loop in every repetition (device and host), or when the counts disagree.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = (0.5, 1.0)
SIZES = (16, 256, 1024)
LMIN, LMAX = 33, 513


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), min=min(v), max=max(v), reps=v)


def _time(arms, reps, warmup):
    """Alternating arms -> {arm: {device_ms, host_ms}}; an arm returns when its results are on the host."""
    import torch

    for _ in range(warmup):
        for run in arms.values():
            run()
    torch.cuda.synchronize()
    dev, host = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(reps):
        for k, run in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            host[k].append(1e3 * (time.perf_counter() - t0))
            dev[k].append(e0.elapsed_time(e1))
    return {k: dict(device_ms=_stats(dev[k]), host_ms=_stats(host[k])) for k in arms}


def _time_enqueue(arms, reps, warmup):
    """Device-event ms of arms that only enqueue."""
    import torch

    for _ in range(warmup):
        for run in arms.values():
            run()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, run in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return {f"{k}_ms": _stats(v) for k, v in out.items()}


def one(dim, n, args, problems) -> dict:
    import torch
    from sparsernns_amd import floatmodel, synth, verify
    from sparsernns_amd.fxparray import RoundingMode, fxp_from_fp
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = synth.make_model(dim)
    nl = dims["n_layers"]
    eng, feng = build_regression_model(md, qc, nl).engine(), floatmodel.FloatEngine(md, nl)
    assert feng.on_device
    lens = [int(v) for v in np.random.Generator(np.random.PCG64(1000 + n)).integers(LMIN, LMAX + 1, n)]
    Lmax = max(lens)
    x = torch.from_numpy(synth.make_input(n, Lmax, dims["d_in"], seed=7)).to(feng.device)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=feng.device)
    for e, L in enumerate(lens):
        x[e, L:] = 0
    clips = [x[e:e + 1, :L].contiguous() for e, L in enumerate(lens)]
    keep = {}

    def arm_clips():
        keep["clips"] = verify.compare_clips(eng, feng, (x, lens_dev), qc, by="stage")

    def arm_loop():
        keep["loop"] = [verify.compare_engines(eng, feng, c, qc, by="stage") for c in clips]

    r = dict(dim_scale=dim, n=n, frames=sum(lens), Lmax=Lmax, padded_frames=n * Lmax)
    r.update(_time(dict(clips=arm_clips, loop=arm_loop), args.reps, args.warmup))
    for clock in ("device_ms", "host_ms"):
        a, b = r["clips"][clock]["reps"], r["loop"][clock]["reps"]
        r[f"loop_over_clips_{clock[:-3]}"] = r["loop"][clock]["median"] / r["clips"][clock]["median"]
        r[f"clips_faster_in_every_rep_{clock[:-3]}"] = all(u < v for u, v in zip(a, b))
        if n == 256 and not r[f"clips_faster_in_every_rep_{clock[:-3]}"]:
            problems.append(f"dim {dim} n {n}: compare_clips is not faster than the per-clip loop in every repetition ({clock})")
    for i, s in enumerate(keep["clips"]):
        for k in ("n", "n_nonfinite", "n_equal", "n_ref_nonzero"):
            if s[k] != sum(rows[i][k] for rows in keep["loop"]):
                problems.append(f"dim {dim} n {n}: {s['name']}: {k} of the one call is not the sum over the loop")
    # the traced launch against the untraced one
    fx = fxp_from_fp(x, bits=eng.inp_bits, exp=eng.inp_exp, signed=True, round_mode=RoundingMode.FLOOR, warn_on_clip=False)
    data = fx.data.contiguous()
    y = torch.empty((n, Lmax, eng.d_out), dtype=torch.int32, device=feng.device)
    planes = [eng._trace_planes(data) for _ in range(nl)]
    r["launch"] = _time_enqueue(dict(untraced=lambda: eng.clips(data, lens_dev, y, x_bits=fx.bits, x_exp=fx.exp),
                                     traced=lambda: eng.clips_traced(data, lens_dev, y, x_bits=fx.bits, x_exp=fx.exp, traces=planes)),
                                args.reps, args.warmup)
    r["launch"]["traced_over_untraced"] = r["launch"]["traced_ms"]["median"] / r["launch"]["untraced_ms"]["median"]
    del planes
    # the masked comparison against the unmasked one on the padded boxes
    rows, status = verify.clip_rows(eng, feng, x, lens_dev, qc)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    pad = torch.arange(Lmax, device=feng.device)[None, :] >= lens_dev[:, None]
    plain_rows = []
    for name, a, b, a_exp, relu in rows:
        if isinstance(a_exp, tuple):   # the padded box has one exponent per pair; any legal one: the cost does not depend on it
            a_exp = int(st[0, 8 + 4])
        az, bz = a.clone(), b.clone()
        az[pad], bz[pad] = 0, 0        # the unmasked call reads the padding: give it numbers
        plain_rows.append((name, az, bz, a_exp, relu))
    masked = verify.StageCallClips(verify._split_clips(rows, lens_dev, "stage", 8)[0])
    padded = verify.StageCall(verify._split(plain_rows, "stage", 8)[0])
    r["compare"] = _time_enqueue(dict(masked=masked.enqueue, padded=padded.enqueue), args.reps, args.warmup)
    r["compare"]["masked_over_padded"] = r["compare"]["masked_ms"]["median"] / r["compare"]["padded_ms"]["median"]
    r["compare"]["elements_inside"] = sum(rec["n"] for rec in masked.records())
    r["compare"]["elements_padded"] = sum(p.n for p in padded.pairs)
    print(f"[bench_verify_clips] dim {dim} n {n} ({r['frames']} frames, Lmax {Lmax}): clips {r['clips']['device_ms']['median']:.2f} ms dev "
          f"/ {r['clips']['host_ms']['median']:.2f} ms host, loop {r['loop']['device_ms']['median']:.2f} / {r['loop']['host_ms']['median']:.2f}: "
          f"x{r['loop_over_clips_device']:.1f} dev, x{r['loop_over_clips_host']:.1f} host; launch traced {r['launch']['traced_ms']['median']:.3f} "
          f"vs {r['launch']['untraced_ms']['median']:.3f} ms; compare masked {r['compare']['masked_ms']['median']:.3f} vs padded "
          f"{r['compare']['padded_ms']['median']:.3f} ms", flush=True)
    return r


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dims", type=float, nargs="*", default=list(DIMS))
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 10:
        print("[bench_verify_clips] the protocol asks for at least ten repetitions", file=sys.stderr)

    import torch

    if not torch.cuda.is_available():
        print("[bench_verify_clips] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    problems: list = []
    res = dict(tool="tools/bench_verify_clips.py", reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               clips=f"{LMIN}..{LMAX} frames, PCG64(1000 + n)", results={}, problems=problems)
    for dim in args.dims:
        for n in args.sizes:
            res["results"][f"dim{dim}_n{n}"] = one(dim, n, args, problems)
            torch.cuda.empty_cache()
            if args.out:   # after every size: a run that is cut short leaves what it measured
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(res, f, indent=1)
    print(json.dumps({"tool": res["tool"], "problems": problems,
                      "results": {k: dict(clips_dev_ms=v["clips"]["device_ms"]["median"], loop_dev_ms=v["loop"]["device_ms"]["median"],
                                          clips_host_ms=v["clips"]["host_ms"]["median"], loop_host_ms=v["loop"]["host_ms"]["median"],
                                          traced_over_untraced=v["launch"]["traced_over_untraced"],
                                          masked_over_padded=v["compare"]["masked_over_padded"]) for k, v in res["results"].items()}}))
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main())
