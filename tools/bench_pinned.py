#!/usr/bin/env python3
"""bench_pinned.py: what stating the exponents (s5fxp_model_step_at / s5fxp_model_clips_at) costs and buys.

Three measurements, each after a warm-up, --reps repetitions (median, min, max and every repetition are kept):
  existing   s5fxp_model_step at 1 frame x {1, 256, 1024} streams (carry fed back, --steps back-to-back steps per repetition)
             and s5fxp_model_clips on 256 clips of 32 .. 512 frames: device-event time and host wall time per launch.  The
             part --existing-only runs, with nothing newer than Engine.step / Engine.clips, so it runs on the parent's tree.
  pinned     the same workloads through the _at entries next to the unpinned ones of the same run, and a 4096-frame stream
             pushed as 128 steps of 32 rows on both.  Reported, no bar.
  quality    audio.validate_clips over 64 synthetic clips of 33 .. 513 frames with exps=None, calibrate_exps(headroom=0) and
             headroom=1 (calibrated on the same 64 clips): SI-SNR per arm and the share of clips whose mask is bit-identical
             to the unpinned one.  A SYNTHETIC model and synthetic audio: the figures say how much moves, not how it sounds.

  python tools/bench_pinned.py [--steps 200] [--reps 7] [--out FILE.json]
  python tools/bench_pinned.py --existing-only --tree DIR ...   the existing entries only, on the package under DIR
  python tools/bench_pinned.py --merge OUT.json --new a.json,b.json --parent c.json,d.json [--commit ID --parent-commit ID]
      pools the repetitions of alternating runs of two trees; the bar of bench_stream_ragged.py --merge: the new tree's
      median is at most the parent's median plus the parent's max - min
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = (1, 256, 1024)
N_CLIPS, CLIP_LO, CLIP_HI = 256, 32, 512
LONG_FRAMES, LONG_ROWS = 4096, 32
NX = 8


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def _timed(run, reps, per):
    """`run()` enqueues the work of one repetition -> (device us, host us) per unit, `per` units per repetition."""
    import torch
    dev, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6 / per)
        dev.append(e0.elapsed_time(e1) * 1e3 / per)
    return _stats(dev), _stats(host)


def _inputs(qc, dims, n, L, seed):
    import torch
    from oracle import fxp_oracle as O
    from sparsernns_amd import synth
    xf = synth.make_input(n, L, dims["d_in"], seed=seed)
    return torch.from_numpy(O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR).data).cuda()


def _status_exps(eng, lane, n):
    from sparsernns_amd import _lib
    W = _lib.STATUS_WORDS
    st = eng.lane_status(lane, n).cpu().numpy()[:n * W].reshape(n, W)
    live = (st[:, 0] & ~_lib.ST_WIDE_STATE) == 0
    return st[live][:, 8:8 + 8 * eng.n_layers].reshape(-1, eng.n_layers, 8)[:, :, :5].min(axis=0).astype(np.int32)


def bench_steps(eng, qc, dims, S, args, pinned):
    import torch
    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    xs = [_inputs(qc, dims, S, 1, 100 + i).view(S, 1, 1, -1) for i in range(NX)]
    carry = torch.zeros((S, eng.n_layers, 2, 1, eng.P), dtype=torch.int32, device="cuda")
    y = torch.empty((S, 1, 1, eng.d_out), dtype=torch.int32, device="cuda")

    def run(kw):
        def go():
            carry.zero_()
            for k in range(args.steps):
                eng.step(xs[k % NX], carry, y, 1, 1, S, bits, exp, lane=1, **kw)
        return go

    res = dict(sessions=S, L=1, steps=args.steps)
    run({})()
    res["step_device_us"], res["step_host_us"] = _timed(run({}), args.reps, args.steps)
    if pinned:
        exps = _status_exps(eng, 1, S)   # the exponents the last unpinned step chose: a legal set; time does not depend on it
        eng.check_exps(exps)
        run(dict(exps=exps))()
        res["step_at_device_us"], res["step_at_host_us"] = _timed(run(dict(exps=exps)), args.reps, args.steps)
    return res


def bench_clips(eng, qc, dims, args, pinned):
    import torch
    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    rng = np.random.default_rng(12)
    lens = rng.integers(CLIP_LO, CLIP_HI + 1, size=N_CLIPS).astype(np.int32)
    x = _inputs(qc, dims, N_CLIPS, CLIP_HI, 300)
    ld = torch.from_numpy(lens).cuda()
    y = torch.empty((N_CLIPS, CLIP_HI, eng.d_out), dtype=torch.int32, device="cuda")
    res = dict(clips=N_CLIPS, frames=[int(lens.min()), int(lens.max())], total_frames=int(lens.sum()))
    go = lambda kw: (lambda: eng.clips(x, ld, y, x_bits=bits, x_exp=exp, lane=2, **kw))
    go({})()
    res["clips_device_us"], res["clips_host_us"] = _timed(go({}), args.reps, 1)
    if pinned:
        exps = _status_exps(eng, 2, N_CLIPS)
        eng.check_exps(exps)
        go(dict(exps=exps))()
        res["clips_at_device_us"], res["clips_at_host_us"] = _timed(go(dict(exps=exps)), args.reps, 1)
    return res


def bench_long_stream(eng, qc, dims, args):
    """One 4096-frame stream as 128 steps of 32 rows, the carry fed back: unpinned (each step its own exponents) and pinned."""
    import torch
    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    x = _inputs(qc, dims, 1, LONG_FRAMES, 500).view(LONG_FRAMES // LONG_ROWS, 1, 1, LONG_ROWS, -1)
    carry = torch.zeros((1, eng.n_layers, 2, 1, eng.P), dtype=torch.int32, device="cuda")
    y = torch.empty((x.shape[0], 1, 1, LONG_ROWS, eng.d_out), dtype=torch.int32, device="cuda")

    def run(kw):
        def go():
            carry.zero_()
            for k in range(x.shape[0]):
                eng.step(x[k], carry, y[k], 1, LONG_ROWS, 1, bits, exp, lane=3, **kw)
        return go

    res = dict(frames=LONG_FRAMES, rows_per_step=LONG_ROWS, steps=int(x.shape[0]))
    run({})()
    res["step_device_us"], res["step_host_us"] = _timed(run({}), args.reps, x.shape[0])
    exps = _status_exps(eng, 3, 1)
    run(dict(exps=exps))()
    res["step_at_device_us"], res["step_at_host_us"] = _timed(run(dict(exps=exps)), args.reps, x.shape[0])
    return res


def quality(model, qc, dims):
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd.fxparray import FxpArray
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    eng = model.engine()
    g = torch.Generator().manual_seed(77)
    frames = torch.randint(33, 514, (64,), generator=g).tolist()
    clean, noisy = [], []
    for f in frames:
        T = (f - 1) * 128
        t = torch.arange(T) / 16000.0
        c = 0.05 * torch.sin(2 * np.pi * (200.0 + 30.0 * (f % 17)) * t) * (0.5 + 0.5 * torch.sin(2 * np.pi * 3.0 * t))
        clean.append(c.float().cuda())
        noisy.append((c + 0.02 * torch.randn(T, generator=g)).float().cuda())
    rows = [torch.floor(audio.stft_mag(n[None])[0] * float(1 << ie)).clamp(-(1 << (ib - 1)), (1 << (ib - 1)) - 1).to(torch.int32)
            for n in noisy]
    fx = [FxpArray(r.contiguous(), ib, ie, True) for r in rows]
    arms = {"unpinned": None, "headroom0": eng.calibrate_exps(fx, 0), "headroom1": eng.calibrate_exps(fx, 1)}
    base = [t[3].clone() for t in audio.denoise_clips(model, ib, ie, noisy)]
    res = dict(clips=64, frames=[min(frames), max(frames)], model="synthetic (synth.make_model), synthetic audio", arms={})
    for name, exps in arms.items():
        loss, snr = audio.validate_clips(model, ib, ie, noisy, clean, exps=exps)
        masks = [t[3] for t in audio.denoise_clips(model, ib, ie, noisy, exps=exps)]
        same = sum(bool(torch.equal(a, b)) for a, b in zip(masks, base))
        res["arms"][name] = dict(exps=None if exps is None else exps.tolist(), si_snr_db_mean=float(snr.mean()),
                                 si_snr_db_min=float(snr.min()), loss_mean=float(loss.mean()), share_bit_identical=same / 64.0)
    return res


def merge(args) -> int:
    new, par = args.new.split(","), args.parent.split(",")

    def pool(files):
        out = {}
        for f in files:
            d = json.load(open(f))
            for k, v in d["existing"].items():
                for field, s in v.items():
                    if isinstance(s, dict) and "reps" in s and not field.count("_at_"):
                        out.setdefault((k, field), []).extend(s["reps"])
        return out

    pn, pp = pool(new), pool(par)
    rec = dict(tool="tools/bench_pinned.py", commit=args.commit, parent_commit=args.parent_commit,
               order="parent tree and new tree alternating in one GPU call; repetitions pooled per tree",
               bar="new median <= parent median + (parent max - parent min), device time", runs=dict(new=new, parent=par),
               existing={})
    ok = True
    for (k, field), reps in sorted(pp.items()):
        p, n = _stats(reps), _stats(pn[(k, field)])
        within = n["median"] <= p["median"] + (p["max"] - p["min"])
        rec["existing"].setdefault(k, {})[field] = dict(parent=p, new=n, within_parent_spread=within)
        if field.endswith("device_us"):
            ok = ok and within
            print(f"[bench_pinned] {k} {field}: parent {p['median']:.1f} ({p['min']:.1f}-{p['max']:.1f}), new {n['median']:.1f}: "
                  f"{'within' if within else 'BEYOND'} the parent's spread")
    rec["existing_entries_no_slower"] = ok
    full = json.load(open(new[-1]))
    for part in ("device", "steps", "reps", "pinned", "long_stream", "quality"):
        rec[part] = full.get(part)
    with open(args.merge, "w") as f:
        json.dump(rec, f, indent=1)
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dim-scale", type=float, default=0.5)
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the directory whose sparsernns_amd package is measured")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--new", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent-commit", default=None)
    args = ap.parse_args()
    if args.merge:
        return merge(args)
    sys.path.insert(0, os.path.abspath(args.tree))

    import torch
    import sparsernns_amd
    from sparsernns_amd import synth
    from sparsernns_amd.fxpmodel import build_regression_model

    torch.cuda.set_device(0)
    md, qc, dims = synth.make_model(args.dim_scale, calib_L=1024, state_headroom_bits=1)   # bench.py's w8a16 model
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    pinned = not args.existing_only
    res = dict(tool="tools/bench_pinned.py", tree=os.path.dirname(os.path.abspath(sparsernns_amd.__file__)), steps=args.steps,
               reps=args.reps, dim_scale=args.dim_scale, device=torch.cuda.get_device_name(0), unit="us per launch", existing={})
    for S in STREAMS:
        r = res["existing"][f"step_S{S}_L1"] = bench_steps(eng, qc, dims, S, args, pinned)
        print(f"[bench_pinned] step S={S}: {r['step_device_us']['median']:.1f} us device"
              + (f", _at {r['step_at_device_us']['median']:.1f} us" if pinned else ""), flush=True)
    r = res["existing"]["clips_256"] = bench_clips(eng, qc, dims, args, pinned)
    print(f"[bench_pinned] 256 clips: {r['clips_device_us']['median']:.0f} us device"
          + (f", _at {r['clips_at_device_us']['median']:.0f} us" if pinned else ""), flush=True)
    if pinned:
        res["pinned"] = {k: {f: v[f] for f in v if "_at_" in f} for k, v in res["existing"].items()}
        r = res["long_stream"] = bench_long_stream(eng, qc, dims, args)
        print(f"[bench_pinned] 4096 frames as 128 steps of 32 rows: {r['step_device_us']['median']:.1f} us per step, "
              f"_at {r['step_at_device_us']['median']:.1f} us", flush=True)
        if not args.no_quality:
            q = res["quality"] = quality(model, qc, dims)
            for name, a in q["arms"].items():
                print(f"[bench_pinned] quality {name}: SI-SNR {a['si_snr_db_mean']:.3f} dB (min {a['si_snr_db_min']:.3f}), "
                      f"{100 * a['share_bit_identical']:.0f}% of the clips bit-identical to the unpinned forward", flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
