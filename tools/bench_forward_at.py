#!/usr/bin/env python3
"""bench_forward_at.py: what the batch forward at stated exponents (s5fxp_model_forward_at) costs and buys.

Device-event time, --reps repetitions after a warm-up (median, min, max and every repetition are kept), bench.py's w8a16 model
at dim_scale 0.5 and 1.0:
  existing   s5fxp_model_forward on 32 x 4096 frames under S5FXP_FWD_DEFER_REDO (--steps back-to-back forwards per repetition).
             The part --existing-only runs, with nothing newer than Engine.enqueue, so it runs on the parent's tree.
  pinned     the same batch through s5fxp_model_forward_at, at the exponents the unpinned forward's status words report.
  vs_clips   s5fxp_model_forward_at against s5fxp_model_clips_at at the same exponents on 32 clips of 3751 frames (a
             validation batch at N-DNS size) and on 256 clips of 512 frames: the ratio the entry exists for.
  launches   kernel launches per forward, counted from the plan (the status words name each layer's recurrence rung).
  quality    audio.validate_fused(exps=) beside audio.validate_clips(exps=) on the same synthetic clips (dim_scale 0.5).  A
             SYNTHETIC model and synthetic audio: the model denoises nothing, the figures only say that both routes agree.

  python tools/bench_forward_at.py [--steps 20] [--reps 7] [--out FILE.json]
  python tools/bench_forward_at.py --existing-only --tree DIR ...   the existing entry only, on the package under DIR
  python tools/bench_forward_at.py --merge OUT.json --new a.json,b.json --parent c.json,d.json [--commit ID --parent-commit ID]
      pools the repetitions of alternating runs of two trees; the bar of bench_stream_ragged.py --merge: the new tree's
      median is at most the parent's median plus the parent's max - min
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (0.5, 1.0)
BATCH = (32, 4096)
CLIP_SETS = ((32, 3751), (256, 512))


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def _timed(run, reps, per):
    """`run()` enqueues the work of one repetition -> device us per unit, `per` units per repetition."""
    import torch
    dev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3 / per)
    return _stats(dev)


def _inputs(qc, dims, n, L, seed):
    import torch
    from oracle import fxp_oracle as O
    from sparsernns_amd import synth
    xf = synth.make_input(n, L, dims["d_in"], seed=seed)
    return torch.from_numpy(O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR).data).cuda()


def _exps_of(eng, lane, n=1):
    from sparsernns_amd import _lib
    W = _lib.STATUS_WORDS
    st = eng.lane_status(lane, n).cpu().numpy()[:n * W].reshape(n, W)
    return st[:, 8:8 + 8 * eng.n_layers].reshape(n, eng.n_layers, 8)[:, :, :5].min(axis=0).astype(np.int32), st


def launches_per_forward(eng, pinned: bool) -> dict:
    """Kernel launches of one carry-free S5FXP_FWD_DEFER_REDO forward, read off the plan (s5fxp_fast.hpp forward_fast), not
    measured: the head, the encoder, per layer the B projection, the recurrence and the gate kernel, a residual pass after a
    layer, and the decoder.  Unpinned, the decoder does the last layer's residual, and at H = 96 the pass between two layers is
    its one-workgroup head; pinned, every layer has a storing pass.  (Without DEFER_REDO both add two gated launches per layer.)"""
    nl = eng.n_layers
    between = nl if pinned else nl - 1
    return dict(head=1, encoder=1, per_layer=3, between_layers=between, decoder=1, total=3 + 3 * nl + between)


def bench_batch(eng, qc, dims, args, pinned):
    import torch
    from sparsernns_amd.engine import Engine
    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    B, L = BATCH
    x = _inputs(qc, dims, B, L, 700)
    y = torch.empty((B, L, eng.d_out), dtype=torch.int32, device="cuda")
    fl = Engine.LEVEL_FLAGS[0]

    def go(kw):
        def run():
            for _ in range(args.steps):
                eng.enqueue(x, bits, exp, y, B, L, flags=fl, lane=1, **kw)
        return run

    res = dict(B=B, L=L, steps=args.steps)
    go({})()
    torch.cuda.synchronize()
    exps, st = _exps_of(eng, 1)
    assert (st[0, 0] & ~4) == 0, st[0, 0]
    y0 = y.clone()
    res["forward_device_us"] = _timed(go({}), args.reps, args.steps)
    if pinned:
        eng.check_exps(exps)
        go(dict(exps=exps))()
        torch.cuda.synchronize()
        _, st1 = _exps_of(eng, 1)
        res["bit_identical_to_unpinned"] = bool(torch.equal(y, y0)) and bool(np.array_equal(st1[0, 8:], st[0, 8:]))
        res["forward_at_device_us"] = _timed(go(dict(exps=exps)), args.reps, args.steps)
        res["launches"] = dict(forward=launches_per_forward(eng, False), forward_at=launches_per_forward(eng, True))
        res["frames_per_s"] = dict(forward=B * L / res["forward_device_us"]["median"] * 1e6,
                                   forward_at=B * L / res["forward_at_device_us"]["median"] * 1e6)
    return res


def bench_vs_clips(eng, qc, dims, args, n, L):
    import torch
    from sparsernns_amd.engine import Engine
    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    x = _inputs(qc, dims, n, L, 900 + n)
    lens = torch.full((n,), L, dtype=torch.int32, device="cuda")
    yc = torch.empty((n, L, eng.d_out), dtype=torch.int32, device="cuda")
    yf = torch.empty_like(yc)
    eng.clips(x, lens, yc, x_bits=bits, x_exp=exp, lane=2)
    torch.cuda.synchronize()
    exps, _ = _exps_of(eng, 2, n)
    eng.check_exps(exps)
    clips = lambda: eng.clips(x, lens, yc, x_bits=bits, x_exp=exp, lane=2, exps=exps)
    fwd = lambda: eng.enqueue(x, bits, exp, yf, n, L, flags=Engine.LEVEL_FLAGS[0], lane=1, exps=exps)
    clips(), fwd()
    torch.cuda.synchronize()
    _, st = _exps_of(eng, 1)
    res = dict(clips=n, frames=L, redo=bool(st[0, 0] & 16), bit_identical=bool(torch.equal(yc, yf)))
    res["clips_at_device_us"] = _timed(clips, args.reps, 1)
    res["forward_at_device_us"] = _timed(fwd, args.reps, 1)
    res["ratio"] = res["clips_at_device_us"]["median"] / res["forward_at_device_us"]["median"]
    return res


def quality(model, qc, dims):
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd.fxparray import FxpArray
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    eng = model.engine()
    g = torch.Generator().manual_seed(77)
    n, T = 16, 128 * 300
    t = torch.arange(T) / 16000.0
    clean = torch.stack([0.05 * torch.sin(2 * np.pi * (200.0 + 30.0 * k) * t) * (0.5 + 0.5 * torch.sin(2 * np.pi * 3.0 * t))
                         for k in range(n)]).float()
    noisy = (clean + 0.02 * torch.randn(n, T, generator=g)).float().cuda()
    clean = clean.cuda()
    rows = torch.floor(audio.stft_mag(noisy) * float(1 << ie)).clamp(-(1 << (ib - 1)), (1 << (ib - 1)) - 1).to(torch.int32)
    exps = eng.calibrate_exps([FxpArray(r.contiguous(), ib, ie, True) for r in rows])
    lf, sf = audio.validate_fused(model, ib, ie, noisy, clean, exps=exps)
    lc, sc = audio.validate_clips(model, ib, ie, list(noisy), list(clean), exps=exps)
    mf = audio.denoise_fused(model, ib, ie, noisy, exps=exps)[3]
    mc = [r[3] for r in audio.denoise_clips(model, ib, ie, list(noisy), exps=exps)]
    return dict(clips=n, samples=T, model="synthetic (synth.make_model), synthetic audio: the model denoises nothing",
                exps=exps.tolist(), masks_bit_identical=all(bool(torch.equal(mf[e], mc[e])) for e in range(n)),
                si_snr_db_fused=[float(v) for v in sf], si_snr_db_clips=[float(v) for v in sc],
                si_snr_identical=bool(torch.equal(sf, sc)), si_snr_max_abs_diff=float((sf - sc).abs().max()),
                loss_max_abs_diff=float((lf - lc).abs().max()))


def merge(args) -> int:
    new, par = args.new.split(","), args.parent.split(",")

    def pool(files):
        out = {}
        for f in files:
            for k, v in json.load(open(f))["existing"].items():
                out.setdefault(k, []).extend(v["forward_device_us"]["reps"])
        return out

    pn, pp = pool(new), pool(par)
    rec = dict(tool="tools/bench_forward_at.py", commit=args.commit, parent_commit=args.parent_commit,
               order="parent tree and new tree alternating in one GPU call; repetitions pooled per tree",
               bar="new median <= parent median + (parent max - parent min), device time", runs=dict(new=new, parent=par),
               existing={})
    ok = True
    for k, reps in sorted(pp.items()):
        p, n = _stats(reps), _stats(pn[k])
        within = n["median"] <= p["median"] + (p["max"] - p["min"])
        rec["existing"][k] = dict(parent=p, new=n, within_parent_spread=within)
        ok = ok and within
        print(f"[bench_forward_at] {k} forward: parent {p['median']:.1f} ({p['min']:.1f}-{p['max']:.1f}) us, new {n['median']:.1f}: "
              f"{'within' if within else 'BEYOND'} the parent's spread")
    rec["forward_no_slower"] = ok
    full = json.load(open(new[-1]))
    for part in ("device", "steps", "reps", "unit", "pinned", "vs_clips"):
        rec[part] = full.get(part)
    rec["quality"] = next((q for q in (json.load(open(f)).get("quality") for f in new) if q), None)   # (runs may skip it)
    for k, v in (rec["pinned"] or {}).items():   # forward_at against the PARENT's forward, pooled
        p = rec["existing"][k]["parent"]
        a = v["forward_at_device_us"]
        v["vs_parent_forward"] = dict(parent_median=p["median"], forward_at_median=a["median"], ratio=a["median"] / p["median"],
                                      within_parent_spread=a["median"] <= p["median"] + (p["max"] - p["min"]))
    with open(args.merge, "w") as f:
        json.dump(rec, f, indent=1)
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
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
    pinned = not args.existing_only
    res = dict(tool="tools/bench_forward_at.py", tree=os.path.dirname(os.path.abspath(sparsernns_amd.__file__)), steps=args.steps,
               reps=args.reps, device=torch.cuda.get_device_name(0), unit="us per forward / per launch", existing={})
    if pinned:
        res["pinned"], res["vs_clips"] = {}, {}
    for ds in SCALES:
        md, qc, dims = synth.make_model(ds, calib_L=1024, state_headroom_bits=1)   # bench.py's w8a16 model
        model = build_regression_model(md, qc, dims["n_layers"])
        eng = model.engine()
        key = f"ds{ds}_B{BATCH[0]}_L{BATCH[1]}"
        r = bench_batch(eng, qc, dims, args, pinned)
        res["existing"][key] = dict(B=r["B"], L=r["L"], steps=r["steps"], forward_device_us=r["forward_device_us"])
        print(f"[bench_forward_at] dim_scale {ds}: forward {r['forward_device_us']['median']:.1f} us"
              + (f", forward_at {r['forward_at_device_us']['median']:.1f} us, bit-identical at its own exponents: "
                 f"{r['bit_identical_to_unpinned']}" if pinned else ""), flush=True)
        if pinned:
            res["pinned"][key] = {k: v for k, v in r.items() if k != "forward_device_us"}
            for n, L in CLIP_SETS:
                c = res["vs_clips"][f"ds{ds}_{n}x{L}"] = bench_vs_clips(eng, qc, dims, args, n, L)
                print(f"[bench_forward_at] dim_scale {ds}, {n} clips of {L} frames: clips_at {c['clips_at_device_us']['median']:.0f} us, "
                      f"forward_at {c['forward_at_device_us']['median']:.0f} us ({c['ratio']:.1f}x), bit-identical: "
                      f"{c['bit_identical']}", flush=True)
            if ds == 0.5 and not args.no_quality:
                q = res["quality"] = quality(model, qc, dims)
                print(f"[bench_forward_at] quality: masks bit-identical {q['masks_bit_identical']}, SI-SNR identical "
                      f"{q['si_snr_identical']} (max |diff| {q['si_snr_max_abs_diff']:.3g} dB)", flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
