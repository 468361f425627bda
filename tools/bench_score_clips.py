#!/usr/bin/env python3
"""bench_score_clips.py: the validation step for n audio clips of different lengths (bench.py's w8a16 model at dim_scale 0.5).

Workloads: tools/bench_audio_clips.py's -- n in 1, 64, 256, 1024 clips, lengths seeded-uniform in [4096, 65536] samples.
  (a) the scored inverse alone, on the same noisy and clean audio and the same fixed masks, no plane stored:
        ragged    s5fxp_mask_istft_score_clips: 2 launches
        per clip  s5fxp_mask_istft_score at B = 1, T = T_e, back to back on one stream, through the C ABI on rows of the padded
                  tensors: 2n launches.  Both sides use one preallocated workspace, so no allocation is timed.
  (b) the whole step: audio.validate_clips (4 launches) against audio.validate_fused clip by clip (19 + 2 launches each)
Times are device-event times of one pass over all n clips, --reps repetitions after a warm-up (median, min, max and every
repetition are kept).  At every timed size the ragged scores are compared with the per-clip ones (torch.equal) before timing.

  python tools/bench_score_clips.py [--reps 10] [--out FILE.json]
  python tools/bench_score_clips.py --baseline-only ...   only the per-clip sides, with nothing newer than audio.validate_fused:
                                                          runs unchanged on the commit before the ragged kernels existed
  python tools/bench_score_clips.py --merge OUT.json --new a.json,b.json --parent c.json,d.json [--commit ID --parent-commit ID]
                                                          pools the repetitions of alternating runs of two trees into one record
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (1, 64, 256, 1024)
T_LO, T_HI = 4096, 65536
DISTINCT = 64
LAM = 0.001
FIELDS = ("per_clip_score_us", "per_clip_validate_us", "ragged_score_us", "validate_clips_us")


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def workloads():
    out = []
    for n in COUNTS:
        rng = np.random.Generator(np.random.PCG64(2000 + n))
        out.append((f"n{n}", [int(v) for v in rng.integers(T_LO, T_HI + 1, n)]))
    return out


def bench_workload(model, ib, ie, pools, Ts, args):
    """pools: (noisy, clean), each (DISTINCT, T_HI) float32 on the device; clip e is the first Ts[e] samples of row e % DISTINCT."""
    import torch
    from sparsernns_amd import _lib, audio

    lib, sync = _lib.lib, torch.cuda.synchronize
    n, Tmax = len(Ts), max(Ts)
    L = [audio.stft_frames(T) for T in Ts]
    Lmax = audio.stft_frames(Tmax)
    a, c = torch.zeros((n, Tmax), device="cuda"), torch.zeros((n, Tmax), device="cuda")
    for e, T in enumerate(Ts):
        a[e, :T], c[e, :T] = pools[0][e % DISTINCT, :T], pools[1][e % DISTINCT, :T]
    mask = torch.rand((n, Lmax, 257), device="cuda", generator=torch.Generator("cuda").manual_seed(n)) * 0.6 - 0.3
    row = Lmax * 257 * 4
    # one workspace for either side: the batch entry at B = 1 never needs more than a row of the ragged one
    wb = max(lib.s5fxp_score_workspace_bytes(1, Tmax), 48 * n * -(-(Lmax - 1) // 13))
    ws = torch.zeros(wb // 8, dtype=torch.float64, device="cuda")
    pc = torch.zeros((3, n), device="cuda")   # loss, si_snr, mag_mse per clip

    def per_clip_score():
        s = torch.cuda.current_stream().cuda_stream
        for e, T in enumerate(Ts):
            lib.s5fxp_mask_istft_score(a.data_ptr() + e * Tmax * 4, c.data_ptr() + e * Tmax * 4, mask.data_ptr() + e * row, 1, T, LAM,
                                       None, None, ws.data_ptr(), wb, pc.data_ptr() + (n + e) * 4, pc.data_ptr() + (2 * n + e) * 4,
                                       pc.data_ptr() + e * 4, s)

    noisy, clean = [a[e, :T] for e, T in enumerate(Ts)], [c[e, :T] for e, T in enumerate(Ts)]
    keep = {}

    def per_clip_validate():
        keep["per_clip"] = [audio.validate_fused(model, ib, ie, x[None], y[None], LAM) for x, y in zip(noisy, clean)]

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

    res = dict(n=n, Tmax=Tmax, Lmax=Lmax, frames=int(sum(L)), samples=int(sum(Ts)))
    if args.baseline_only:
        for run, field in ((per_clip_score, FIELDS[0]), (per_clip_validate, FIELDS[1])):
            for _ in range(2):
                run()
            sync()
            res[field] = _stats(timed(run))
        return res

    smp = torch.tensor(Ts, dtype=torch.int32, device="cuda")
    rg = torch.zeros((3, n), device="cuda")

    def ragged_score():
        _lib.check(lib.s5fxp_mask_istft_score_clips(a.data_ptr(), c.data_ptr(), mask.data_ptr(), n, Tmax, smp.data_ptr(), LAM, None, None,
                                                    ws.data_ptr(), wb, rg[1].data_ptr(), rg[2].data_ptr(), rg[0].data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "s5fxp_mask_istft_score_clips")

    def validate_clips():
        keep["clips"] = audio.validate_clips(model, ib, ie, noisy, clean, LAM)

    # the scores first: nothing is timed that does not give the per-clip bits
    for run in (per_clip_score, ragged_score, per_clip_validate, validate_clips):
        for _ in range(2):
            run()
    sync()
    res["scores_equal"] = bool(torch.equal(rg, pc))
    res["validate_equal"] = bool(torch.equal(keep["clips"][0], torch.cat([r[0] for r in keep["per_clip"]]))
                                 and torch.equal(keep["clips"][1], torch.cat([r[1] for r in keep["per_clip"]])))
    st = model.engine().lane_status(0, n).cpu().numpy()[:n * _lib.STATUS_WORDS].reshape(n, _lib.STATUS_WORDS)
    res["validate_clips_path_clip"] = bool((st[:, 2] == _lib.PATH_CLIP).all())
    assert res["scores_equal"], f"n={n}: the ragged scores differ from the per-clip scores"
    assert res["validate_equal"], f"n={n}: validate_clips differs from validate_fused clip by clip"
    for run, field in ((per_clip_score, FIELDS[0]), (per_clip_validate, FIELDS[1]), (ragged_score, FIELDS[2]), (validate_clips, FIELDS[3])):
        res[field] = _stats(timed(run))
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
    rec = dict(tool="tools/bench_score_clips.py", commit=args.commit, parent_commit=args.parent_commit,
               order="parent tree and new tree alternating in one GPU call; repetitions pooled per tree",
               unit="us of device time per pass over all clips", runs=dict(new=new, parent=par), device=first.get("device"),
               expectation="n256 and n1024, medians: the two ragged launches <= 0.5 x the parent's 2n per-clip launches, and "
                           "validate_clips <= 0.5 x the parent's validate_fused clip by clip",
               workloads={})
    parent = {f: pool(par, f) for f in FIELDS[:2]}
    mine = {f: pool(new, f) for f in FIELDS}
    ok = True
    for k, v in first["workloads"].items():
        s = {f: v[f] for f in ("n", "Tmax", "Lmax", "frames", "samples")}
        for f in ("scores_equal", "validate_equal", "validate_clips_path_clip"):
            s[f] = all(json.load(open(p))["workloads"][k][f] for p in new)
        s["parent_per_clip_score_us"] = _stats(parent[FIELDS[0]][k])
        s["parent_per_clip_validate_us"] = _stats(parent[FIELDS[1]][k])
        s["new_tree_per_clip_score_us"] = _stats(mine[FIELDS[0]][k])
        s["new_tree_per_clip_validate_us"] = _stats(mine[FIELDS[1]][k])
        s["ragged_score_us"] = _stats(mine[FIELDS[2]][k])
        s["validate_clips_us"] = _stats(mine[FIELDS[3]][k])
        s["ratio_score"] = s["parent_per_clip_score_us"]["median"] / s["ragged_score_us"]["median"]
        s["ratio_validate"] = s["parent_per_clip_validate_us"]["median"] / s["validate_clips_us"]["median"]
        expected = v["n"] >= 256
        if expected:
            s["meets_half_score"] = s["ragged_score_us"]["median"] <= 0.5 * s["parent_per_clip_score_us"]["median"]
            s["meets_half_validate"] = s["validate_clips_us"]["median"] <= 0.5 * s["parent_per_clip_validate_us"]["median"]
            ok = ok and s["meets_half_score"] and s["meets_half_validate"]
        rec["workloads"][k] = s
        print(f"[bench_score_clips] {k}: score per clip (parent) {s['parent_per_clip_score_us']['median']:.0f} us, ragged "
              f"{s['ragged_score_us']['median']:.0f} us (x{s['ratio_score']:.2f}); validate per clip (parent) "
              f"{s['parent_per_clip_validate_us']['median']:.0f} us, validate_clips {s['validate_clips_us']['median']:.0f} us "
              f"(x{s['ratio_validate']:.2f})"
              + (f"; expectation {'met' if s['meets_half_score'] and s['meets_half_validate'] else 'MISSED'}" if expected else ""))
    rec["expectation_met"] = ok
    with open(args.merge, "w") as f:
        json.dump(rec, f, indent=1)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--only", default=None, help="comma-separated workload names to run, e.g. n256")
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
        print("[bench_score_clips] note: fewer than 10 repetitions is a rehearsal, not a measurement", flush=True)

    import torch
    from sparsernns_amd import synth
    from sparsernns_amd.fxpmodel import build_regression_model

    if not torch.cuda.is_available():
        print("[bench_score_clips] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    res = dict(tool="tools/bench_score_clips.py", baseline_only=args.baseline_only, reps=args.reps,
               device=torch.cuda.get_device_name(0), unit="us of device time per pass over all clips", workloads={})
    md, qc, dims = synth.make_model(0.5, calib_L=1024, state_headroom_bits=1)   # bench.py's w8a16 model at dim_scale 0.5
    model = build_regression_model(md, qc, dims["n_layers"])
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    g = torch.Generator().manual_seed(17)
    clean = 0.05 * torch.randn((DISTINCT, T_HI), generator=g)
    noisy = clean + 0.02 * torch.randn((DISTINCT, T_HI), generator=g)
    pools = (noisy.cuda(), clean.cuda())
    for name, Ts in workloads():
        if args.only and name not in args.only.split(","):
            continue
        r = bench_workload(model, ib, ie, pools, Ts, args)
        res["workloads"][name] = r
        msg = (f"[bench_score_clips] {name}: score per clip {r[FIELDS[0]]['median']:.0f} us, validate per clip "
               f"{r[FIELDS[1]]['median']:.0f} us")
        if FIELDS[2] in r:
            msg += f"; ragged score {r[FIELDS[2]]['median']:.0f} us, validate_clips {r[FIELDS[3]]['median']:.0f} us"
        print(msg, flush=True)
        model.engine()._wsl.clear()
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
