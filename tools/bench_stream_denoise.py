#!/usr/bin/env python3
"""bench_stream_denoise.py: what one push of the streaming denoising loop costs -- c hops of audio of `sessions` live signals
in, c cleaned hops out -- on audio.StreamDenoiser (s5fxp_stream_stft -> SessionPool.push -> s5fxp_stream_mask_istft: three
launches) and on the torch-op loop a caller had to write before it (the baseline arm: nothing newer than SessionPool.push).

Baseline arm per push: history `cat` -> `unfold` -> `rfft` -> `abs` -> SessionPool.push -> the scaled spectrum -> `irfft` -> a
carried overlap-add tail.  Both arms run in the same process, alternating per repetition, on the same audio; first their x rows
and -- with both back ends given the same mask -- their audio must agree push by push within the tolerances of
tests/test_audio_kernels.py (2e-6 and 2e-5 x amplitude).

Per shape (dim_scale, sessions, c), after a warm-up of that shape in both arms (the streams are past their first three hops):
  device_us  device-event time of --steps back-to-back pushes (check=False: no host synchronisation inside), per push;
  host_us    host wall time per push with a synchronise after each (check=True: the status words are read), the shape of a
             real-time loop;
  pool_*     the bare SessionPool.push on the same rows, so that what the audio steps add is visible.
--reps repetitions each: median, min, max and every repetition are kept.

  python tools/bench_stream_denoise.py [--steps 200] [--reps 7] [--shapes 0.5:1:1,...] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(0.5, 1, 1), (0.5, 32, 1), (0.5, 256, 1), (0.5, 256, 4), (0.5, 1024, 1), (1.0, 256, 1)]
NX = 8       # distinct audio chunks, fed round robin
AMP = 0.02
ATOL_SPEC, ATOL_AUDIO = 2e-6, 2e-5
HOP, NFFT = 128, 512


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


class TorchLoop:
    """The streaming front and back end in torch ops around SessionPool.push: what served a live signal before the kernels."""

    def __init__(self, engine, S, sub):
        import torch
        self.torch, self.S, self.sub = torch, S, sub
        self.pool = engine.pool(S)
        self.hist = torch.zeros(S, 3 * HOP, device="cuda")
        self.tail = torch.zeros(S, 3 * HOP, device="cuda")   # overlap-add sums of the next three output hops
        self.hops = 0

    def reset(self):
        self.pool.reset()
        self.hist.zero_()
        self.tail.zero_()
        self.hops = 0

    def push(self, hops, check=True, mask=None):
        """Steady state only (hops >= 3 received): c frames in, c hops out, each divided by a cover of 4.  `mask`: used in
        place of the pool's (the agreement check gives both arms' back ends the same one)."""
        torch = self.torch
        c = hops.shape[1] // HOP
        window = torch.cat([self.hist, hops], dim=1)
        z = torch.fft.rfft(window.unfold(-1, NFFT, HOP), n=NFFT, dim=-1) / NFFT
        x = (z.abs() - self.sub).contiguous()
        own = self.pool.push(x, check=check)
        mask = own if mask is None else mask
        seg = torch.fft.irfft(z * (1.0 + mask), n=NFFT, dim=-1) * NFFT          # (S, c, 512)
        ola = torch.cat([self.tail, torch.zeros(self.S, c * HOP, device=hops.device)], dim=1)
        for i in range(c):
            ola[:, i * HOP:i * HOP + NFFT] += seg[:, i]
        self.hist = window[:, -3 * HOP:]
        self.tail = ola[:, c * HOP:]
        self.hops += c
        self.x = x
        return ola[:, :c * HOP] / 4.0


def bench_shape(model, S, c, args):
    import torch
    from sparsernns_amd import audio

    eng = model.engine()
    K = args.steps
    sync = torch.cuda.synchronize
    g = torch.Generator().manual_seed(100 + S + c)
    chunks = [(AMP * torch.randn(S, c * HOP, generator=g)).cuda() for _ in range(NX)]
    new = audio.StreamDenoiser(model, S)
    base = TorchLoop(eng, S, audio.STFT_MAG_MEAN)
    pool = eng.pool(S)

    def start(arm):
        arm.reset()
        for k in range(-(-4 // c)):       # past the first three hops: every later push has F = O = c
            arm.push(chunks[k % NX])

    def run(arm, n, check=False):
        out = None
        for k in range(n):
            out = arm.push(chunks[k % NX], check=check)
        return out

    # agreement of the two arms on the same signal, push by push: the x rows, and the audio with both back ends given the new
    # arm's mask (two FFTs differ in the last bits of |Z|, FLOOR turns some of that into an input LSB, and a recurrent model
    # carries it on: the arms' own masks are not comparable bit for bit)
    start(new)
    start(base)
    dx = da = 0.0
    for k in range(NX):
        out, x, mask, _ = new.push(chunks[k], details=True)
        ob = base.push(chunks[k], mask=mask)
        dx = max(dx, float((x - base.x).abs().max()))
        if k * c >= 3:   # the baseline's tail still holds three hops made with its own masks of the warm-up
            da = max(da, float((out - ob).abs().max()))
    sync()
    res = dict(sessions=S, c=c, steps=K, max_abs_diff_x=dx, atol_x=ATOL_SPEC * AMP, max_abs_diff_audio=da,
               atol_audio=ATOL_AUDIO * AMP, outputs_agree=dx <= ATOL_SPEC * AMP and da <= ATOL_AUDIO * AMP)
    assert res["outputs_agree"], f"S={S} c={c}: the two arms differ by {dx:.3e} on x, {da:.3e} on audio"

    xrows = new._buf[(c, c)][0].clone()

    class PoolArm:
        def reset(self):
            pool.reset()

        def push(self, _, check=True):
            return pool.push(xrows, check=check)

    arms = (("new", new), ("baseline", base), ("pool", PoolArm()))
    dev = {n: [] for n, _ in arms}
    host = {n: [] for n, _ in arms}
    for _ in range(args.reps):           # the arms alternate within the run
        for name, arm in arms:
            start(arm) if name != "pool" else arm.reset()
            run(arm, 2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            e0.record()
            run(arm, K)
            e1.record()
            sync()
            dev[name].append(e0.elapsed_time(e1) * 1e3 / K)
            if hasattr(arm, "_pool"):
                arm._pool.check()
            elif name == "baseline":
                arm.pool.check()
            else:
                pool.check()
        for name, arm in arms:
            start(arm) if name != "pool" else arm.reset()
            sync()
            t0 = time.perf_counter()
            for k in range(K):
                arm.push(chunks[k % NX], check=True)
                sync()
            host[name].append((time.perf_counter() - t0) * 1e6 / K)
    for name, _ in arms:
        res[f"{name}_device_us"] = _stats(dev[name])
        res[f"{name}_host_us"] = _stats(host[name])
    res["device_ratio_baseline_over_new"] = res["baseline_device_us"]["median"] / res["new_device_us"]["median"]
    res["host_ratio_baseline_over_new"] = res["baseline_host_us"]["median"] / res["new_host_us"]["median"]
    # the bar: the medians are below the baseline's; `separated`: so is every repetition (the margin exceeds the spread)
    for k in ("device", "host"):
        n, b = res[f"new_{k}_us"], res[f"baseline_{k}_us"]
        res[f"meets_bar_{k}"] = n["median"] < b["median"]
        res[f"separated_{k}"] = n["max"] < b["min"]
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=None, help="subset, e.g. 0.5:1:1,1.0:256:1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 200 or args.reps < 7:
        print("[bench_stream_denoise] note: fewer than 200 steps or 7 repetitions is a rehearsal, not a measurement", flush=True)

    import torch
    from sparsernns_amd import synth
    from sparsernns_amd.fxpmodel import build_regression_model

    torch.cuda.set_device(0)
    shapes = SHAPES if not args.shapes else [tuple(float(p) if i == 0 else int(p) for i, p in enumerate(s.split(":")))
                                             for s in args.shapes.split(",")]
    res = dict(tool="tools/bench_stream_denoise.py", steps=args.steps, reps=args.reps, device=torch.cuda.get_device_name(0),
               unit="us per push", amplitude=AMP, order="arms alternate within each repetition, one process", shapes={})
    models = {}
    for ds, S, c in shapes:
        if ds not in models:
            md, qc, dims = synth.make_model(ds, calib_L=1024, state_headroom_bits=1)   # bench.py's w8a16 model at this dim_scale
            models[ds] = build_regression_model(md, qc, dims["n_layers"])
        r = bench_shape(models[ds], S, c, args)
        key = f"ds{ds}_S{S}_c{c}"
        res["shapes"][key] = r
        print(f"[bench_stream_denoise] {key}: new {r['new_device_us']['median']:.1f} us device, {r['new_host_us']['median']:.0f} us host; "
              f"torch loop {r['baseline_device_us']['median']:.1f} / {r['baseline_host_us']['median']:.0f}; "
              f"bare pool {r['pool_device_us']['median']:.1f} / {r['pool_host_us']['median']:.0f}; "
              f"bar device {r['meets_bar_device']} host {r['meets_bar_host']}", flush=True)
        torch.cuda.empty_cache()
    res["all_shapes_meet_bar"] = all(r["meets_bar_device"] and r["meets_bar_host"] for r in res["shapes"].values())
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
