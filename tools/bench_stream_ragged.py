#!/usr/bin/env python3
"""bench_stream_ragged.py: what the per-session descriptors of audio.SessionDenoiser cost against the lock-step
audio.StreamDenoiser, and what a mixed tick of a multi-tenant pool costs against the only route to it without them.

Arms (one process, alternating per repetition, after a warm-up that takes every stream past its first four hops):
  a  StreamDenoiser.push            S sessions in lock step, c hops each: the yardstick (its kernels are untouched)
  b  SessionDenoiser.push           the same S sessions, all at the same phase, through the descriptors
  c  SessionPool.stage_desc alone   building, checking and copying the descriptors of that push
  d  a mixed tick at S = 256        one session starting (FRESH), one finishing (ZEROS | FINAL), 16 idle, the rest c = 1
  e  one StreamDenoiser(model, 1) per session at S = 32, c = 1: how such traffic is served without the descriptors
Per arm and shape: device-event time of --steps back-to-back ticks (check=False) and host wall time per tick with the status
read and a synchronise after each (check=True), per tick; --reps repetitions, every one kept.  Before anything is timed the
outputs of a and b are compared push by push (torch.equal) at every timed shape, and b's at S = 32 with e's.

Bars (recorded, not tuned):
  b   median device time <= a's median + a's own p10-p90 width + c's median device time;
  d,e d's cost per session, and b's at S = 32, below e's cost per session in every repetition, device and host.

  python tools/bench_stream_ragged.py [--steps 200] [--reps 7] [--shapes 0.5:32:1,...] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(0.5, 32, 1), (0.5, 256, 1), (0.5, 256, 4), (0.5, 1024, 1), (1.0, 256, 1)]
MIXED_S, EACH_S, IDLE = 256, 32, 16
NX = 8       # distinct audio chunks, fed round robin
AMP = 0.02
HOP = 128


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), p10=float(np.percentile(v, 10)),
                p90=float(np.percentile(v, 90)), reps=v)


def _timed(torch, tick, prepare, K, reps_dev, reps_host):
    """tick(k, check) is one tick; prepare() puts the arm into its steady state."""
    sync = torch.cuda.synchronize
    prepare()
    for k in range(2):
        tick(k, False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync()
    e0.record()
    for k in range(K):
        tick(k, False)
    e1.record()
    sync()
    reps_dev.append(e0.elapsed_time(e1) * 1e3 / K)
    prepare()
    sync()
    t0 = time.perf_counter()
    for k in range(K):
        tick(k, True)
        sync()
    reps_host.append((time.perf_counter() - t0) * 1e6 / K)


class Lockstep:
    def __init__(self, audio, model, S, chunks):
        self.d, self.chunks, self.c = audio.StreamDenoiser(model, S), chunks, chunks[0].shape[1] // HOP

    def prepare(self):
        self.d.reset()
        for k in range(-(-4 // self.c)):
            self.d.push(self.chunks[k % NX])

    def tick(self, k, check):
        return self.d.push(self.chunks[k % NX], check=check)

    def settle(self):
        self.d._pool.check()


class Ragged:
    """Arm b: every session named in every push, all at the same phase."""

    def __init__(self, audio, model, S, chunks):
        self.d, self.chunks, self.c, self.ids = audio.SessionDenoiser(model, S), chunks, chunks[0].shape[1] // HOP, np.arange(S)

    def prepare(self):
        self.d.start(self.ids)
        for k in range(-(-4 // self.c)):
            self.d.push(self.ids, self.chunks[k % NX])

    def tick(self, k, check):
        return self.d.push(self.ids, self.chunks[k % NX], check=check)[0]

    def settle(self):
        self.d._pool.check()


class DescOnly:
    """Arm c: the descriptors of arm b's push, staged and copied, nothing launched."""

    def __init__(self, pool, S, c):
        self.pool, self.S, self.c = pool, S, c
        self.ids, self.rows, self.flags, self.h4 = np.arange(S), np.full(S, c), np.zeros(S, dtype=np.int64), np.full(S, 4)

    def prepare(self):
        pass

    def tick(self, k, check):
        return self.pool.stage_desc(self.ids, self.rows, self.flags, hops=self.rows, h4=self.h4, Lmax=self.c, cmax=self.c)

    def settle(self):
        pass


class Mixed:
    """Arm d: S sessions, each tick one finishes, the one that finished a tick earlier starts again, IDLE of them have nothing
    to push and the rest push one hop.  Rows are two hops wide (counts = 1) so that the finishing entry joins without a copy."""

    def __init__(self, audio, model, S, chunks2):
        self.d, self.S, self.chunks = audio.SessionDenoiser(model, S), S, chunks2
        self.t = 0

    def prepare(self):
        self.d.start(np.arange(self.S))
        for k in range(4):
            self.d.push(np.arange(self.S), self.chunks[k % NX], counts=np.ones(self.S, dtype=np.int64))
        self.t, self.ended = 0, None
        self.ones = np.ones(self.S, dtype=np.int64)

    def entries(self):
        S, t = self.S, self.t
        fin = t % S
        live = np.ones(S, dtype=bool)
        live[fin] = False
        live[(t + 2 + np.arange(IDLE)) % S] = False
        return np.nonzero(live)[0], fin

    def tick(self, k, check):
        push, fin = self.entries()
        if self.ended is not None:
            self.d.start([self.ended])
        out = self.d.push(push, self.chunks[k % NX][:len(push)], counts=self.ones[:len(push)], finish=[fin], check=check)
        self.ended = fin
        self.t += 1
        return out

    def settle(self):
        self.d._pool.check()


class Each:
    """Arm e: one StreamDenoiser(model, 1) per session."""

    def __init__(self, audio, model, S, chunks):
        self.ds, self.chunks = [audio.StreamDenoiser(model, 1) for _ in range(S)], chunks

    def prepare(self):
        for s, d in enumerate(self.ds):
            d.reset()
            for k in range(4):
                d.push(self.chunks[k % NX][s:s + 1])

    def tick(self, k, check):
        return [d.push(self.chunks[k % NX][s:s + 1], check=check) for s, d in enumerate(self.ds)]

    def settle(self):
        for d in self.ds:
            d._pool.check()


def _chunks(torch, S, c, seed):
    g = torch.Generator().manual_seed(seed)
    return [(AMP * torch.randn(S, c * HOP, generator=g)).cuda() for _ in range(NX)]


def _agree_ab(torch, a, b, S, c):
    """a and b on the same signal from the start, push by push: out, x, mask, cleaned_mag."""
    a.d.reset()
    b.d.start(b.ids)
    for k in range(NX + 4):
        ra = a.d.push(a.chunks[k % NX], details=True)
        out, n_out, x, mask, cm, frames = b.d.push(b.ids, b.chunks[k % NX], details=True)
        O, F = int(n_out[0]), int(frames[0])
        assert len(set(n_out)) == 1 and len(set(frames)) == 1
        pairs = ((ra[0], out[:, :O * HOP]), (ra[1], x[:, :F]), (ra[2], mask[:, :F]), (ra[3], cm[:, :F]))
        if not all(torch.equal(p, q) for p, q in pairs):
            return False
    return True


def bench_shape(audio, model, S, c, args):
    import torch
    chunks = _chunks(torch, S, c, 100 + S + c)
    a, b = Lockstep(audio, model, S, chunks), Ragged(audio, model, S, chunks)
    res = dict(sessions=S, c=c, steps=args.steps, outputs_equal=_agree_ab(torch, a, b, S, c))
    assert res["outputs_equal"], f"S={S} c={c}: SessionDenoiser and StreamDenoiser differ"
    arms = (("a", a), ("b", b), ("c", DescOnly(model.engine().pool(S), S, c)))
    dev, host = {n: [] for n, _ in arms}, {n: [] for n, _ in arms}
    for _ in range(args.reps):
        for name, arm in arms:
            _timed(torch, arm.tick, arm.prepare, args.steps, dev[name], host[name])
            arm.settle()
    for name, _ in arms:
        res[f"{name}_device_us"], res[f"{name}_host_us"] = _stats(dev[name]), _stats(host[name])
    A, B, Cc = res["a_device_us"], res["b_device_us"], res["c_device_us"]
    res["b_bar_device_us"] = A["median"] + (A["p90"] - A["p10"]) + Cc["median"]
    res["b_meets_bar"] = B["median"] <= res["b_bar_device_us"]
    return res


def bench_mixed(audio, model, args, b32):
    import torch
    S = MIXED_S
    d = Mixed(audio, model, S, _chunks(torch, S, 2, 7))
    chunks = _chunks(torch, EACH_S, 1, 100 + EACH_S + 1)     # arm b's chunks at S = 32
    e = Each(audio, model, EACH_S, chunks)
    # e's sessions against arm b at S = 32 on the same signal, push by push
    b = Ragged(audio, model, EACH_S, chunks)
    for dd in e.ds:
        dd.reset()
    b.d.start(b.ids)
    equal = True
    for k in range(NX + 4):
        outs = [dd.push(chunks[k % NX][s:s + 1]) for s, dd in enumerate(e.ds)]
        out, n_out = b.d.push(b.ids, chunks[k % NX])
        equal = equal and torch.equal(torch.cat(outs), out[:, :int(n_out[0]) * HOP])
    assert equal, "arm e and arm b differ at S = 32"
    n_d = S - IDLE
    arms = (("d", d), ("e", e))
    dev, host = {n: [] for n, _ in arms}, {n: [] for n, _ in arms}
    for _ in range(args.reps):
        for name, arm in arms:
            _timed(torch, arm.tick, arm.prepare, args.steps, dev[name], host[name])
            arm.settle()
    res = dict(d_sessions=S, d_entries_per_tick=n_d, d_idle=IDLE, e_sessions=EACH_S, outputs_equal=equal)
    for name, _ in arms:
        res[f"{name}_device_us"], res[f"{name}_host_us"] = _stats(dev[name]), _stats(host[name])
    for k in ("device", "host"):
        dv = [v / n_d for v in res[f"d_{k}_us"]["reps"]]
        ev = [v / EACH_S for v in res[f"e_{k}_us"]["reps"]]
        res[f"d_per_session_{k}_us"], res[f"e_per_session_{k}_us"] = _stats(dv), _stats(ev)
        res[f"d_below_e_every_rep_{k}"] = max(dv) < min(ev)
        if b32 is not None:
            bv = [v / EACH_S for v in b32[f"b_{k}_us"]["reps"]]
            res[f"b32_per_session_{k}_us"] = _stats(bv)
            res[f"b32_below_e_every_rep_{k}"] = max(bv) < min(ev)
    return res


def merge(args) -> int:
    """Two trees alternating in one GPU call: per shape the device time of arm b (the ragged step and audio kernels), and of the
    mixed tick d, repetitions pooled per tree; the new tree is within the bar when its median <= the parent's + (max - min)."""
    new, par = [json.load(open(f)) for f in args.new.split(",")], [json.load(open(f)) for f in args.parent.split(",")]
    rec = dict(tool="tools/bench_stream_ragged.py", commit=args.commit, parent_commit=args.parent_commit, unit="us per tick",
               order="parent tree and new tree alternating in one GPU call; repetitions pooled per tree", device=new[0].get("device"),
               steps=new[0]["steps"], shapes={})
    rows = [(k, lambda r, k=k: r["shapes"][k]["b_device_us"]["reps"]) for k in new[0]["shapes"]]
    rows.append(("mixed_d", lambda r: r["mixed"]["d_device_us"]["reps"]))
    for k, get in rows:
        p, n = _stats([v for r in par for v in get(r)]), _stats([v for r in new for v in get(r)])
        ok = n["median"] <= p["median"] + (p["max"] - p["min"])
        rec["shapes"][k] = dict(parent_device_us=p, new_tree_device_us=n, within_parent_spread=ok)
        print(f"[bench_stream_ragged] {k}: parent {p['median']:.1f} ({p['min']:.1f}-{p['max']:.1f}) us, this tree {n['median']:.1f} "
              f"({n['min']:.1f}-{n['max']:.1f}) us: {'within' if ok else 'BEYOND'} the parent's spread")
    with open(args.merge, "w") as f:
        json.dump(rec, f, indent=1)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=None, help="subset, e.g. 0.5:32:1,1.0:256:1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None, help="OUT.json: pool arm b (and the mixed tick d) of --new and --parent runs of two trees")
    ap.add_argument("--new", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent-commit", default=None)
    args = ap.parse_args()
    if args.merge:
        return merge(args)
    if args.steps < 200 or args.reps < 7:
        print("[bench_stream_ragged] note: fewer than 200 steps or 7 repetitions is a rehearsal, not a measurement", flush=True)

    import torch
    from sparsernns_amd import audio, synth
    from sparsernns_amd.fxpmodel import build_regression_model

    torch.cuda.set_device(0)
    shapes = SHAPES if not args.shapes else [tuple(float(p) if i == 0 else int(p) for i, p in enumerate(s.split(":")))
                                             for s in args.shapes.split(",")]
    res = dict(tool="tools/bench_stream_ragged.py", steps=args.steps, reps=args.reps, device=torch.cuda.get_device_name(0),
               unit="us per tick", amplitude=AMP, order="arms alternate within each repetition, one process", shapes={})
    models = {}

    def model(ds):
        if ds not in models:
            md, qc, dims = synth.make_model(ds, calib_L=1024, state_headroom_bits=1)   # bench.py's w8a16 model at this dim_scale
            models[ds] = build_regression_model(md, qc, dims["n_layers"])
        return models[ds]

    for ds, S, c in shapes:
        r = bench_shape(audio, model(ds), S, c, args)
        key = f"ds{ds}_S{S}_c{c}"
        res["shapes"][key] = r
        print(f"[bench_stream_ragged] {key}: a {r['a_device_us']['median']:.1f} us device / {r['a_host_us']['median']:.0f} us host; "
              f"b {r['b_device_us']['median']:.1f} / {r['b_host_us']['median']:.0f}; c {r['c_device_us']['median']:.1f} / "
              f"{r['c_host_us']['median']:.0f}; b's bar {r['b_bar_device_us']:.1f}: {r['b_meets_bar']}", flush=True)
        torch.cuda.empty_cache()
    m = res["mixed"] = bench_mixed(audio, model(0.5), args, res["shapes"].get(f"ds0.5_S{EACH_S}_c1"))
    print(f"[bench_stream_ragged] mixed tick: d {m['d_per_session_device_us']['median']:.2f} us device / "
          f"{m['d_per_session_host_us']['median']:.2f} us host per session; e {m['e_per_session_device_us']['median']:.1f} / "
          f"{m['e_per_session_host_us']['median']:.1f}; below in every repetition: device {m['d_below_e_every_rep_device']}, "
          f"host {m['d_below_e_every_rep_host']}", flush=True)
    res["b_meets_bar_all_shapes"] = all(r["b_meets_bar"] for r in res["shapes"].values())
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
