#!/usr/bin/env python3
"""bench_clips.py: n clips of different lengths, each its own compute_best batch -- the one-launch clip kernel
(Engine.clips, s5fxp_model_clips) against the only way the batch path computes the same results: one
Engine.enqueue(B=1, L=len, FWD_DEFER_REDO) per clip, back to back on one stream.

Per model (bench.py's w8a16 model at dim_scale 0.5 and 1.0) and workload:
  mixed_n{1,64,256,1024}   lengths seeded-uniform in [32, 512]
  equal_n{1,64,256,1024}   all lengths 128; here the grouped forward (groups = n, B = 1) is timed too
  single_L{32..2048}       one clip of that length: where a single clip stops paying off against the batch path
Times are device-event times of one pass over all n clips, --reps repetitions after a warm-up (median, min, max and every
repetition are kept).  The batch path is TIMED on FWD_DEFER_REDO whatever the data (its shortest launch set, 17 launches per
clip); the outputs the clip launch is COMPARED with (np.array_equal, every clip, at every timed size) come from a
self-contained forward per clip.  The 64 distinct seeded clips of a model are repeated for n > 64 (with other lengths).

  python tools/bench_clips.py [--reps 10] [--out FILE.json]
  python tools/bench_clips.py --baseline-only ...   only the batch path, with nothing newer than Engine.enqueue: runs unchanged
                                                    on the commit before the clip kernel existed
  python tools/bench_clips.py --merge OUT.json --new a.json,b.json --parent c.json,d.json [--commit ID --parent-commit ID]
                                                    pools the repetitions of alternating runs of two trees into one record
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALES = (0.5, 1.0)
COUNTS = (1, 64, 256, 1024)
SINGLE = (32, 64, 128, 256, 512, 1024, 2048)
DISTINCT = 64


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def workloads():
    out = []
    for n in COUNTS:
        rng = np.random.Generator(np.random.PCG64(1000 + n))
        out.append((f"mixed_n{n}", [int(v) for v in rng.integers(32, 513, n)]))
    for n in COUNTS:
        out.append((f"equal_n{n}", [128] * n))
    for L in SINGLE:
        out.append((f"single_L{L}", [L]))
    return out


def bench_workload(eng, pool, bits, exp, lens, args, grouped):
    """pool: (DISTINCT, 2048, d_in) int32 device tensor; clip e is rows 0 .. lens[e]-1 of pool[e % DISTINCT]."""
    import torch
    from sparsernns_amd import _lib

    n, Lmax = len(lens), max(lens)
    sync = torch.cuda.synchronize
    x = torch.zeros((n, Lmax, eng.d_in), dtype=torch.int32, device="cuda")
    for e, L in enumerate(lens):
        x[e, :L] = pool[e % DISTINCT, :L]
    yb = torch.zeros((n, Lmax, eng.d_out), dtype=torch.int32, device="cuda")

    def base(flags=_lib.FWD_DEFER_REDO):
        for e, L in enumerate(lens):
            eng.enqueue(x[e:e + 1, :L], bits, exp, yb[e:e + 1, :L], 1, L, flags=flags)

    def timed(run):
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            e0.record()
            run()
            e1.record()
            sync()
            out.append(e0.elapsed_time(e1) * 1e3)
        return out

    res = dict(n=n, Lmax=Lmax, frames=int(sum(lens)), baseline_timed_flags=int(_lib.FWD_DEFER_REDO))
    base(0)   # the reference outputs: self-contained forwards
    sync()
    want = yb.cpu().numpy().copy()
    for _ in range(2):
        base()
    sync()
    res["baseline_device_us"] = _stats(timed(base))
    if grouped:
        yg = torch.zeros_like(yb)
        run_g = lambda: eng.enqueue(x, bits, exp, yg, 1, Lmax, flags=_lib.FWD_DEFER_REDO, lane=2, groups=n)
        for _ in range(2):
            run_g()
        sync()
        res["grouped_device_us"] = _stats(timed(run_g))
        res["grouped_redo"] = bool(int(eng.check_status(2)[0]) & _lib.ST_REDO)
        res["grouped_outputs_equal"] = bool(np.array_equal(yg.cpu().numpy(), want))
    if args.baseline_only:
        return res

    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    yc = torch.zeros_like(yb)
    run_c = lambda: eng.clips(x, lens_d, yc, x_bits=bits, x_exp=exp, lane=1)
    for _ in range(2):
        run_c()
    sync()
    st = eng.lane_status(1, n).cpu().numpy()[:n * _lib.STATUS_WORDS].reshape(n, _lib.STATUS_WORDS)
    assert (st[:, 2] == _lib.PATH_CLIP).all() and not (st[:, 0] & ~_lib.ST_WIDE_STATE).any(), st[:, :3]
    same = bool(np.array_equal(yc.cpu().numpy(), want))
    res["outputs_equal"] = same
    assert same, f"n={n}: the clip launch differs from the per-clip forwards"
    res["clips_device_us"] = _stats(timed(run_c))
    return res


def merge(args) -> int:
    def pool(files, field):
        out = {}
        for f in files:
            for k, v in json.load(open(f))["workloads"].items():
                if field in v:
                    out.setdefault(k, []).extend(v[field]["reps"])
        return out
    new, par = args.new.split(","), args.parent.split(",")
    first = json.load(open(new[0]))
    rec = dict(tool="tools/bench_clips.py", commit=args.commit, parent_commit=args.parent_commit,
               order="parent tree and new tree alternating in one GPU call; repetitions pooled per tree",
               unit="us of device time per pass over all clips", runs=dict(new=new, parent=par), device=first.get("device"),
               bound="mixed_n256 and mixed_n1024: clip launch <= 0.5 x the parent's per-clip forwards (medians)", workloads={})
    pb = pool(par, "baseline_device_us")
    pc = pool(par, "clips_device_us")   # a parent that has the clip kernel too: its clip launch against this tree's
    mine = {f: pool(new, f) for f in ("baseline_device_us", "clips_device_us", "grouped_device_us")}
    ok = True
    for k, v in first["workloads"].items():
        s = dict(n=v["n"], Lmax=v["Lmax"], frames=v["frames"], outputs_equal=all(json.load(open(f))["workloads"][k]["outputs_equal"] for f in new))
        s["parent_device_us"] = _stats(pb[k])
        s["new_tree_baseline_device_us"] = _stats(mine["baseline_device_us"][k])
        s["clips_device_us"] = _stats(mine["clips_device_us"][k])
        if k in mine["grouped_device_us"]:
            s["grouped_device_us"] = _stats(mine["grouped_device_us"][k])
            s["grouped_outputs_equal"] = v.get("grouped_outputs_equal")
            s["grouped_redo"] = v.get("grouped_redo")
        s["ratio_parent_over_clips"] = s["parent_device_us"]["median"] / s["clips_device_us"]["median"]
        bounded = "mixed_n256" in k or "mixed_n1024" in k
        if bounded:
            s["meets_half"] = s["clips_device_us"]["median"] <= 0.5 * s["parent_device_us"]["median"]
            ok = ok and s["meets_half"]
        ok = ok and s["outputs_equal"]
        if k in pc:   # no slower than the parent's clip launch: its median plus its own spread (max - min) in the same call
            p = s["parent_clips_device_us"] = _stats(pc[k])
            s["clips_within_parent_spread"] = s["clips_device_us"]["median"] <= p["median"] + (p["max"] - p["min"])
        rec["workloads"][k] = s
        print(f"[bench_clips] {k}: parent {s['parent_device_us']['median']:.0f} us, clips {s['clips_device_us']['median']:.0f} us "
              f"(x{s['ratio_parent_over_clips']:.2f})" + (f", grouped {s['grouped_device_us']['median']:.0f} us" if "grouped_device_us" in s else "")
              + (f", bound {'met' if s['meets_half'] else 'MISSED'}" if bounded else "")
              + (f"; parent's clip launch {s['parent_clips_device_us']['median']:.0f} us: {'within' if s['clips_within_parent_spread'] else 'BEYOND'} its spread"
                 if k in pc else ""))
    rec["bound_met"] = ok
    with open(args.merge, "w") as f:
        json.dump(rec, f, indent=1)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--only", default=None, help="substrings of the workload names to run, e.g. mixed_n256,single_L32")
    ap.add_argument("--scales", default=None, help="subset of the dim_scales, e.g. 0.5")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--new", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent-commit", default=None)
    args = ap.parse_args()
    if args.merge:
        return merge(args)
    if args.reps < 10:
        print("[bench_clips] note: fewer than 10 repetitions is a rehearsal, not a measurement", flush=True)

    import torch
    from sparsernns_amd import _lib, synth
    from sparsernns_amd._lib import check, lib
    from sparsernns_amd.fxpmodel import build_regression_model

    if not torch.cuda.is_available():
        print("[bench_clips] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    res = dict(tool="tools/bench_clips.py", baseline_only=args.baseline_only, reps=args.reps, device=torch.cuda.get_device_name(0),
               unit="us of device time per pass over all clips", workloads={})
    for ds in ([float(s) for s in args.scales.split(",")] if args.scales else SCALES):
        md, qc, dims = synth.make_model(ds, calib_L=1024, state_headroom_bits=1)   # bench.py's w8a16 model at this dim_scale
        eng = build_regression_model(md, qc, dims["n_layers"]).engine()
        bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
        xf = torch.from_numpy(synth.make_input(DISTINCT, max(SINGLE), dims["d_in"], seed=17)).cuda()
        pool = torch.empty(xf.shape, dtype=torch.int32, device="cuda")
        check(lib.s5fxp_from_fp(xf.data_ptr(), pool.data_ptr(), xf.numel(), bits, exp, 0, torch.cuda.current_stream().cuda_stream))
        for name, lens in workloads():
            if args.only and not any(o in name for o in args.only.split(",")):
                continue
            key = f"ds{ds}_{name}"
            r = bench_workload(eng, pool, bits, exp, lens, args, grouped=name.startswith("equal"))
            res["workloads"][key] = r
            msg = f"[bench_clips] {key}: per-clip forwards {r['baseline_device_us']['median']:.0f} us"
            if "grouped_device_us" in r:
                msg += f", grouped {r['grouped_device_us']['median']:.0f} us"
            if "clips_device_us" in r:
                msg += f", clip launch {r['clips_device_us']['median']:.0f} us"
            print(msg, flush=True)
            eng._wsl.clear()
            torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
