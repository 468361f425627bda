#!/usr/bin/env python3
"""bench_stream.py: what one streaming step costs -- a chunk of L frames of `sessions` independent streams with the carry fed
back -- on the one-launch step (Engine.step / SessionPool, s5fxp_model_step) and on the batch path that served streams before
it (grouped Engine.enqueue with state_in / state_out and FWD_DEFER_REDO; Engine.forward_chunk's allocate / ladder / check loop
for the host-wall row).

Per shape (dim_scale, sessions, B, L), after a warm-up of both paths:
  device_us   device-event time of --steps back-to-back steps (carry fed back, no host synchronisation inside), per step;
  host_us     host wall time per step with a synchronise after every step, the shape of a real-time loop:
              baseline = forward_chunk (one session whose data stays on the optimistic rung) or the same work for a group of
              sessions: allocate, one FWD_DEFER_REDO enqueue, synchronise, read the status -- never a repeat on a lower rung;
              step = SessionPool.push(check=True), which synchronises and reads the status words; step_sync = Engine.step +
              one synchronise, no status read.
The batch path is timed on FWD_DEFER_REDO whatever the data (its shortest launch set); the outputs the step is compared with
come from the rung the data needs (reference_flags in the record).
--reps repetitions each (median, min, max and every repetition are kept).  Both paths run the same --steps chunks from a zero
carry and their last outputs and final carries must be equal (np.array_equal) at the timed sizes.

  python tools/bench_stream.py [--steps 200] [--reps 7] [--out FILE.json]
  python tools/bench_stream.py --baseline-only ...     only the batch path, with nothing newer than Engine.enqueue /
                                                       forward_chunk: runs unchanged on the commit before the step existed
  python tools/bench_stream.py --merge OUT.json --new a.json,b.json --parent c.json,d.json [--commit ID --parent-commit ID]
                                                       pools the repetitions of alternating runs of two trees into one record
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(0.5, 1, 1, 1), (0.5, 32, 1, 1), (0.5, 256, 1, 1), (0.5, 256, 1, 4), (0.5, 1024, 1, 1), (1.0, 256, 1, 1)]
NX = 8   # distinct input chunks, fed round robin


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def _key(ds, S, B, L):
    return f"ds{ds}_S{S}_B{B}_L{L}"


def bench_shape(eng, qc, dims, S, B, L, args, baseline_only):
    import torch
    from oracle import fxp_oracle as O
    from sparsernns_amd import _lib, synth
    from sparsernns_amd.fxparray import FxpArray

    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    xs = []
    for i in range(NX):
        xf = synth.make_input(S * B, L, dims["d_in"], seed=100 + i)
        xs.append(torch.from_numpy(O.from_fp(xf, bits, exp, True, O.FLOOR).data.reshape(S, B, L, -1)).cuda())
    K = args.steps
    cshape = (S, eng.n_layers, 2, B, eng.P)
    sync = torch.cuda.synchronize

    # ---- batch path
    sa, sb = torch.zeros(cshape, dtype=torch.int32, device="cuda"), torch.zeros(cshape, dtype=torch.int32, device="cuda")
    yb = torch.empty((S, B, L, eng.d_out), dtype=torch.int32, device="cuda")
    view = (lambda t: t) if S > 1 else (lambda t: t[0])

    # The batch path is TIMED on its optimistic rung (FWD_DEFER_REDO: its shortest launch set, 17 launches at three layers),
    # whatever the data: its launches do the same work whether or not a state leaves the fast recurrence's range.  The
    # outputs the step is COMPARED with come from the rung of Engine.LEVEL_FLAGS the data needs (`level`, found below).
    level = [0]

    def base_steps(n, flags=_lib.FWD_DEFER_REDO):
        a, b = sa, sb
        a.zero_()
        for k in range(n):
            eng.enqueue(xs[k % NX].view(S * B, L, -1), bits, exp, yb.view(S * B, L, -1), B, L, flags=flags,
                        state_in=view(a), state_out=view(b), groups=S)
            a, b = b, a
        return a

    def base_chunk(x, state):   # forward_chunk's work per step (allocate, enqueue, synchronise, read the status), without its repeats
        if S == 1 and level[0] == 0:
            return eng.forward_chunk(FxpArray(x[0], bits, exp), state[0])[1][None]
        y = torch.empty((S * B, L, eng.d_out), dtype=torch.int32, device="cuda")
        new = torch.empty(cshape, dtype=torch.int32, device="cuda")
        eng.enqueue(x.view(S * B, L, -1), bits, exp, y, B, L, flags=_lib.FWD_DEFER_REDO, state_in=view(state), state_out=view(new), groups=S)
        sync()
        eng.check_status()
        return new

    def timed_device(run):
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            e0.record()
            run(K)
            e1.record()
            sync()
            out.append(e0.elapsed_time(e1) * 1e3 / K)
        return out

    def timed_host(one_step, fresh):
        out = []
        for _ in range(args.reps):
            st = fresh()
            sync()
            t0 = time.perf_counter()
            for k in range(K):
                st = one_step(xs[k % NX], st)
                sync()
            out.append((time.perf_counter() - t0) * 1e6 / K)
        return out

    while True:
        for _ in range(2):
            base_steps(NX, eng.LEVEL_FLAGS[level[0]])
        sync()
        # (the status words are the last step's; a step that left the optimistic range also leaves a carry the next one fails on)
        final_b = base_steps(K, eng.LEVEL_FLAGS[level[0]])
        sync()
        if not (int(eng.check_status()[0]) & _lib.ST_REDO):
            break
        assert level[0] < 2
        level[0] += 1   # what forward_chunk's ladder does for such data: the next rung
    want_y, want_s = yb.cpu().numpy().copy(), final_b.cpu().numpy().copy()
    res = dict(sessions=S, B=B, L=L, steps=K, baseline_timed_flags=int(_lib.FWD_DEFER_REDO), reference_flags=int(eng.LEVEL_FLAGS[level[0]]))
    for _ in range(2):
        base_steps(NX)
    sync()
    res["baseline_device_us"] = _stats(timed_device(base_steps))
    res["baseline_host_us"] = _stats(timed_host(base_chunk, lambda: torch.zeros(cshape, dtype=torch.int32, device="cuda")))
    if baseline_only:
        return res

    # ---- the one-launch step
    from sparsernns_amd import SessionPool
    carry = torch.zeros(cshape, dtype=torch.int32, device="cuda")
    ys = torch.empty((S, B, L, eng.d_out), dtype=torch.int32, device="cuda")

    def step_steps(n):
        carry.zero_()
        for k in range(n):
            eng.step(xs[k % NX], carry, ys, B, L, S, bits, exp, lane=1)
        return carry

    for _ in range(2):
        step_steps(NX)
    sync()
    step_steps(K)
    sync()
    st = eng.check_status(1)
    assert int(st[2]) == _lib.PATH_STEP
    same = bool(np.array_equal(ys.cpu().numpy(), want_y) and np.array_equal(carry.cpu().numpy(), want_s))
    res["outputs_equal"] = same
    assert same, f"S={S} B={B} L={L}: the step's outputs or carry differ from the batch path's after {K} steps"
    res["step_device_us"] = _stats(timed_device(step_steps))
    pool = SessionPool(eng, S, B)

    def push(x, _):
        pool.push(FxpArray(x, bits, exp))

    def fresh_pool():
        pool.reset()

    res["step_host_us"] = _stats(timed_host(push, fresh_pool))

    def step_sync(x, _):
        eng.step(x, carry, ys, B, L, S, bits, exp, lane=1)

    res["step_sync_host_us"] = _stats(timed_host(step_sync, lambda: carry.zero_()))
    return res


def merge(args) -> int:
    def pool(files, field):
        out = {}
        for f in files:
            for k, v in json.load(open(f))["shapes"].items():
                if field in v:
                    out.setdefault(k, []).extend(v[field]["reps"])
        return out
    new, par = args.new.split(","), args.parent.split(",")
    rec = dict(tool="tools/bench_stream.py", commit=args.commit, parent_commit=args.parent_commit,
               order="parent tree and new tree alternating in one GPU call; repetitions pooled per tree",
               unit="us per step", runs=dict(new=new, parent=par), shapes={})
    first = json.load(open(new[0]))
    rec["steps"], rec["device"] = first["steps"], first.get("device")
    pd, ph = pool(par, "baseline_device_us"), pool(par, "baseline_host_us")
    ps = pool(par, "step_device_us")   # a parent that has the step kernel too: its step against this tree's
    fields = ("baseline_device_us", "baseline_host_us", "step_device_us", "step_host_us", "step_sync_host_us")
    mine = {f: pool(new, f) for f in fields}
    ok = True
    for k, v in first["shapes"].items():
        s = dict(sessions=v["sessions"], B=v["B"], L=v["L"], outputs_equal=all(json.load(open(f))["shapes"][k]["outputs_equal"] for f in new))
        s["parent_device_us"], s["parent_host_us"] = _stats(pd[k]), _stats(ph[k])
        for f in fields:
            s["new_tree_" + f] = _stats(mine[f][k])
        s["device_ratio_parent_over_step"] = s["parent_device_us"]["median"] / s["new_tree_step_device_us"]["median"]
        s["host_ratio_parent_over_step"] = s["parent_host_us"]["median"] / s["new_tree_step_host_us"]["median"]
        s["meets_half"] = s["new_tree_step_device_us"]["median"] <= 0.5 * s["parent_device_us"]["median"]
        ok = ok and s["meets_half"] and s["outputs_equal"]
        if k in ps:   # no slower than the parent's step: its median plus its own spread (max - min) in the same call
            p = s["parent_step_device_us"] = _stats(ps[k])
            s["step_within_parent_spread"] = s["new_tree_step_device_us"]["median"] <= p["median"] + (p["max"] - p["min"])
            print(f"[bench_stream] {k}: parent's step {p['median']:.1f} ({p['min']:.1f}-{p['max']:.1f}) us, this tree's "
                  f"{s['new_tree_step_device_us']['median']:.1f} us: {'within' if s['step_within_parent_spread'] else 'BEYOND'} the parent's spread")
        rec["shapes"][k] = s
        print(f"[bench_stream] {k}: parent {s['parent_device_us']['median']:.1f} us, step {s['new_tree_step_device_us']['median']:.1f} us "
              f"(x{s['device_ratio_parent_over_step']:.1f}); host {s['parent_host_us']['median']:.0f} -> {s['new_tree_step_host_us']['median']:.0f} us")
    rec["all_shapes_meet_half"] = ok
    with open(args.merge, "w") as f:
        json.dump(rec, f, indent=1)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--shapes", default=None, help="subset, e.g. 0.5:1:1:1,1.0:256:1:1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--new", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent-commit", default=None)
    args = ap.parse_args()
    if args.merge:
        return merge(args)
    if args.steps < 200 or args.reps < 7:
        print("[bench_stream] note: fewer than 200 steps or 7 repetitions is a rehearsal, not a measurement", flush=True)

    import torch
    from sparsernns_amd import synth
    from sparsernns_amd.fxpmodel import build_regression_model

    torch.cuda.set_device(0)
    shapes = SHAPES if not args.shapes else [tuple(float(p) if i == 0 else int(p) for i, p in enumerate(s.split(":"))) for s in args.shapes.split(",")]
    res = dict(tool="tools/bench_stream.py", baseline_only=args.baseline_only, steps=args.steps, reps=args.reps,
               device=torch.cuda.get_device_name(0), unit="us per step", shapes={})
    engines = {}
    for ds, S, B, L in shapes:
        if ds not in engines:
            md, qc, dims = synth.make_model(ds, calib_L=1024, state_headroom_bits=1)   # bench.py's w8a16 model at this dim_scale
            engines[ds] = (build_regression_model(md, qc, dims["n_layers"]).engine(), qc, dims)
        eng, qc, dims = engines[ds]
        r = bench_shape(eng, qc, dims, S, B, L, args, args.baseline_only)
        res["shapes"][_key(ds, S, B, L)] = r
        msg = f"[bench_stream] {_key(ds, S, B, L)}: batch path {r['baseline_device_us']['median']:.1f} us device, {r['baseline_host_us']['median']:.0f} us host"
        if not args.baseline_only:
            msg += f"; step {r['step_device_us']['median']:.1f} us device, {r['step_host_us']['median']:.0f} us host (push), {r['step_sync_host_us']['median']:.0f} us (step + sync)"
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
