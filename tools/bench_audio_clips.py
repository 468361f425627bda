#!/usr/bin/env python3
"""bench_audio_clips.py: the denoising loop for n audio clips of different lengths (bench.py's w8a16 model at dim_scale 0.5).

Workloads: n in 1, 64, 256, 1024 clips, lengths seeded-uniform in [4096, 65536] samples (33 .. 513 frames).
  (a) the audio steps alone, on the same audio and the same fixed masks:
        ragged    s5fxp_stft_mag_clips + s5fxp_mask_istft_clips (with cleaned_mag): 2 launches
        per clip  s5fxp_stft_mag + s5fxp_mask_istft (with cleaned_mag) at B = 1, T = T_e, back to back on one stream, through
                  the C ABI into the padded tensors: 2n launches, the cheapest way the batch kernels serve the same clips
  (b) the whole loop: audio.denoise_clips (3 launches) against audio.denoise_fused clip by clip (19 launches each)
Times are device-event times of one pass over all n clips, --reps repetitions after a warm-up (median, min, max and every
repetition are kept).  At every timed size the ragged outputs are compared with the per-clip ones (torch.equal).

  python tools/bench_audio_clips.py [--reps 10] [--out FILE.json]
  python tools/bench_audio_clips.py --baseline-only ...   only the per-clip sides, with nothing newer than audio.denoise_fused:
                                                          runs unchanged on the commit before the ragged kernels existed
  python tools/bench_audio_clips.py --merge OUT.json --new a.json,b.json --parent c.json,d.json [--commit ID --parent-commit ID]
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
FIELDS = ("per_clip_audio_us", "per_clip_denoise_us", "ragged_audio_us", "denoise_clips_us")


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def workloads():
    out = []
    for n in COUNTS:
        rng = np.random.Generator(np.random.PCG64(2000 + n))
        out.append((f"n{n}", [int(v) for v in rng.integers(T_LO, T_HI + 1, n)]))
    return out


def bench_workload(model, ib, ie, pool, Ts, args):
    """pool: (DISTINCT, T_HI) float32 device tensor; clip e is the first Ts[e] samples of pool[e % DISTINCT]."""
    import torch
    from sparsernns_amd import _lib, audio

    lib, sync = _lib.lib, torch.cuda.synchronize
    n, Tmax = len(Ts), max(Ts)
    L = [audio.stft_frames(T) for T in Ts]
    Lmax = audio.stft_frames(Tmax)
    a = torch.zeros((n, Tmax), device="cuda")
    for e, T in enumerate(Ts):
        a[e, :T] = pool[e % DISTINCT, :T]
    mask = torch.rand((n, Lmax, 257), device="cuda", generator=torch.Generator("cuda").manual_seed(n)) * 2.0 - 1.0
    shape = (n, Lmax, 257)
    xb, cb = torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda")
    ob = torch.zeros((n, (Lmax - 1) * 128), device="cuda")
    # a clip's mask rows as the B = 1 kernel wants them: contiguous (L_e, 257), which a row of the padded tensor is
    row, orow = Lmax * 257 * 4, (Lmax - 1) * 128 * 4

    def per_clip_audio():
        s = torch.cuda.current_stream().cuda_stream
        for e, T in enumerate(Ts):
            lib.s5fxp_stft_mag(a.data_ptr() + e * Tmax * 4, 1, T, audio.STFT_MAG_MEAN, xb.data_ptr() + e * row, None, s)
        for e, T in enumerate(Ts):
            lib.s5fxp_mask_istft(a.data_ptr() + e * Tmax * 4, mask.data_ptr() + e * row, 1, T, ob.data_ptr() + e * orow,
                                 cb.data_ptr() + e * row, s)

    clips = [a[e, :T] for e, T in enumerate(Ts)]
    keep = {}

    def per_clip_denoise():
        keep["per_clip"] = [audio.denoise_fused(model, ib, ie, c[None]) for c in clips]

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
    for run, field in ((per_clip_audio, "per_clip_audio_us"), (per_clip_denoise, "per_clip_denoise_us")):
        for _ in range(2):
            run()
        sync()
        res[field] = _stats(timed(run))
    if args.baseline_only:
        return res

    smp = torch.tensor(Ts, dtype=torch.int32, device="cuda")
    xr, cr = torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda")
    orr = torch.zeros((n, (Lmax - 1) * 128), device="cuda")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")

    def ragged_audio():
        audio.stft_mag_clips(a, smp, out=(xr, lens))
        audio.mask_istft_clips(a, smp, mask, cleaned_mag=True, out=(orr, cr))

    def denoise_clips():
        keep["clips"] = audio.denoise_clips(model, ib, ie, clips)

    for run, field in ((ragged_audio, "ragged_audio_us"), (denoise_clips, "denoise_clips_us")):
        for _ in range(2):
            run()
        sync()
        res[field] = _stats(timed(run))
    # the padding of all six tensors is the zeros they were made with: whole tensors compare
    res["audio_outputs_equal"] = bool(torch.equal(xr, xb) and torch.equal(orr, ob) and torch.equal(cr, cb) and lens.tolist() == L)
    res["denoise_outputs_equal"] = all(torch.equal(g, w[0]) for got, want in zip(keep["clips"], keep["per_clip"])
                                       for g, w in zip(got, want))
    st = model.engine().lane_status(0, n).cpu().numpy()[:n * _lib.STATUS_WORDS].reshape(n, _lib.STATUS_WORDS)
    res["denoise_clips_path_clip"] = bool((st[:, 2] == _lib.PATH_CLIP).all())
    assert res["audio_outputs_equal"], f"n={n}: the ragged launches differ from the per-clip launches"
    assert res["denoise_outputs_equal"], f"n={n}: denoise_clips differs from denoise_fused clip by clip"
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
    rec = dict(tool="tools/bench_audio_clips.py", commit=args.commit, parent_commit=args.parent_commit,
               order="parent tree and new tree alternating in one GPU call; repetitions pooled per tree",
               unit="us of device time per pass over all clips", runs=dict(new=new, parent=par), device=first.get("device"),
               expectation="n256 and n1024: the two ragged audio launches <= 0.5 x the parent's 2n per-clip launches (medians)",
               workloads={})
    parent = {f: pool(par, f) for f in FIELDS[:2]}
    mine = {f: pool(new, f) for f in FIELDS}
    ok = True
    for k, v in first["workloads"].items():
        s = {f: v[f] for f in ("n", "Tmax", "Lmax", "frames", "samples")}
        for f in ("audio_outputs_equal", "denoise_outputs_equal", "denoise_clips_path_clip"):
            s[f] = all(json.load(open(p))["workloads"][k][f] for p in new)
        s["parent_per_clip_audio_us"] = _stats(parent["per_clip_audio_us"][k])
        s["parent_per_clip_denoise_us"] = _stats(parent["per_clip_denoise_us"][k])
        s["new_tree_per_clip_audio_us"] = _stats(mine["per_clip_audio_us"][k])
        s["new_tree_per_clip_denoise_us"] = _stats(mine["per_clip_denoise_us"][k])
        s["ragged_audio_us"] = _stats(mine["ragged_audio_us"][k])
        s["denoise_clips_us"] = _stats(mine["denoise_clips_us"][k])
        s["ratio_audio"] = s["parent_per_clip_audio_us"]["median"] / s["ragged_audio_us"]["median"]
        s["ratio_denoise"] = s["parent_per_clip_denoise_us"]["median"] / s["denoise_clips_us"]["median"]
        expected = v["n"] >= 256
        if expected:
            s["meets_half"] = s["ragged_audio_us"]["median"] <= 0.5 * s["parent_per_clip_audio_us"]["median"]
            ok = ok and s["meets_half"]
        rec["workloads"][k] = s
        print(f"[bench_audio_clips] {k}: audio per clip (parent) {s['parent_per_clip_audio_us']['median']:.0f} us, ragged "
              f"{s['ragged_audio_us']['median']:.0f} us (x{s['ratio_audio']:.2f})"
              + (f", expectation {'met' if s['meets_half'] else 'MISSED'}" if expected else "")
              + f"; denoise per clip (parent) {s['parent_per_clip_denoise_us']['median']:.0f} us, denoise_clips "
              f"{s['denoise_clips_us']['median']:.0f} us (x{s['ratio_denoise']:.2f})")
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
        print("[bench_audio_clips] note: fewer than 10 repetitions is a rehearsal, not a measurement", flush=True)

    import torch
    from sparsernns_amd import synth
    from sparsernns_amd.fxpmodel import build_regression_model

    if not torch.cuda.is_available():
        print("[bench_audio_clips] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    res = dict(tool="tools/bench_audio_clips.py", baseline_only=args.baseline_only, reps=args.reps,
               device=torch.cuda.get_device_name(0), unit="us of device time per pass over all clips", workloads={})
    md, qc, dims = synth.make_model(0.5, calib_L=1024, state_headroom_bits=1)   # bench.py's w8a16 model at dim_scale 0.5
    model = build_regression_model(md, qc, dims["n_layers"])
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    pool = 0.02 * torch.randn((DISTINCT, T_HI), generator=torch.Generator().manual_seed(17)).cuda()
    for name, Ts in workloads():
        if args.only and name not in args.only.split(","):
            continue
        r = bench_workload(model, ib, ie, pool, Ts, args)
        res["workloads"][name] = r
        msg = (f"[bench_audio_clips] {name}: audio per clip {r['per_clip_audio_us']['median']:.0f} us, denoise per clip "
               f"{r['per_clip_denoise_us']['median']:.0f} us")
        if "ragged_audio_us" in r:
            msg += f"; ragged audio {r['ragged_audio_us']['median']:.0f} us, denoise_clips {r['denoise_clips_us']['median']:.0f} us"
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
