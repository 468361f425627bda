#!/usr/bin/env python3
"""bench.py -- frames/s of the fixed-point S5 forward (w8a16, dim_scale=0.5, NDNS shape) on MI355X.

One "step" = one fused forward (encoder -> 3 S5 layers -> decoder, int32 in -> int32 out) over one
batch of synthetic NDNS-shaped sequences that is already resident in HBM.  Workload = BASELINE.json
configs[1]: B=32 sequences x L=4096 frames per GPU, dense (un-pruned) w8a16.

  python bench.py [--gpus N --steps K --warmup W] [--config 1|2|3|4] [--dump-outputs DIR]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (what the driver does)

With --gpus N > 1 and no launcher (WORLD_SIZE unset) the script starts the N ranks itself: fresh child processes,
one per GPU, started before this process has touched the GPU; rank 0's JSON line is relayed.

Multi-GPU: every rank runs whole reference batches of its own (per-shard exponents: exactly what
the reference computes for that batch, SURVEY.md §8e mode B), no data-path collective; weak scaling.
An RCCL all_gather of the outputs is exercised once outside the timed region.

Prints ONE JSON line on rank 0 (contract in the round prompt), with `roofline` for the recurrence
kernel (timed in situ with HIP events attached to its launches) and `cpu_baseline` (the scalar C oracle
on the host cores; a reported baseline, not the thing measured).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
DUMP_BYTES = 48 << 20  # --dump-outputs: at most this much of float64 output (below the 64 MB cap with room for the header)


def pmc_traffic(B, L, P, kernel, groups, slots):
    """HBM bytes per recurrence launch from the committed PMC passes (profiles/r03_scan_traffic.json: FETCH_SIZE doubled per
    MI355X_MICROARCH.md's gfx950 correction, + WRITE_SIZE), if they were taken on this workload: same shape, same batches per
    launch, same state slots per layer."""
    p = os.path.join(ROOT, "profiles", "r03_scan_traffic.json")
    if not os.path.exists(p):
        return None
    with open(p) as f:
        t = json.load(f)
    if (t["B"], t["L"], t["P"]) != (B, L, P) or list(t.get("stream_slots", t.get("state_slots", []))) != list(slots):
        return None
    for e in t["entries"]:
        if e["batches_per_launch"] == groups and kernel in e["traffic_bytes_per_launch"]:
            return e["traffic_bytes_per_launch"][kernel]
    return None


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: start N fresh ranks of this script (one per GPU; RANK, LOCAL_RANK,
    WORLD_SIZE, MASTER_* in their environment, as torch.distributed.run would set them), relay rank 0's output, return
    the worst exit code.  This process never initialises the GPU (a process that has must not be re-executed, and
    does not need to be: the ranks are children)."""
    import socket
    import subprocess

    # build once, in a child of its own, so that N ranks do not race to compile a stale library
    rc = subprocess.call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT)
    if rc != 0:
        return rc
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    procs = []
    for r in range(n):
        out = None if r == 0 else subprocess.DEVNULL  # rank 0 prints the JSON line straight to our stdout
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], cwd=ROOT, stdout=out,
                                      env=dict(env, RANK=str(r), LOCAL_RANK=str(r))))
    rcs = [p.wait() for p in procs]
    return max(abs(c) for c in rcs)


def scan_stored_bytes(kernel: str, algo_bytes: int) -> int:
    """Bytes the recurrence kernel's two streams hold (what it loads + stores when nothing is re-read): int32 in and
    out = the algorithmic 16*P per frame; the optimistic kernels keep int16 on one or both sides."""
    per16 = {"k_scan_quad_asm16": 8, "k_scan_pairl_asm": 8, "k_scan_pair_asm": 12}  # of 16: int16 in + int16 out; int32 in + int16 out
    return algo_bytes * per16.get(kernel, 16) // 16


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--config", type=int, default=1, choices=(1, 2, 3, 4),
                    help="BASELINE.json configs[i]: 1 = dim 0.5 w8a16 dense, 32 x 4096 per GPU (the headline); 2 = the same "
                         "90 %% pruned; 3 = dim 1.0 pruned, ONE batch of 512 sequences sharded over the ranks + timed "
                         "output gather; 4 = dim 1.0 w4a8")
    ap.add_argument("--batch", type=int, default=None, help="sequences per GPU (config 3: the global batch)")
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--dim-scale", type=float, default=None)
    ap.add_argument("--sparsity", type=float, default=None)
    ap.add_argument("--quantization", default=None)
    ap.add_argument("--input-scale", type=float, default=None, help="scale of the synthetic input (default 1; 300 for w4a8)")
    ap.add_argument("--state-headroom-bits", type=int, default=None,
                    help="extra integer bits of the SSM state in the synthetic qconfig (default 1; 2 for pruned models, whose\n"
                         "fixed-point states drift further from the float calibration)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=32, help="sequences per pass of the bounded CPU-baseline sample")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="the CPU baseline repeats its pass until this much time has gone")
    ap.add_argument("--global-exponents", action="store_true", help="mode A: all-reduce(MAX) the exponent maxima")
    ap.add_argument("--inflight", type=int, default=3, help="launch sets in flight (streams); 1 = one at a time")
    ap.add_argument("--groups", type=int, default=8,
                    help="reference batches per launch set (s5fxp_forward_opts::groups): G independent batches of --batch sequences, each "
                         "its own compute_best batch, enqueued as one set of kernel launches; a step is still ONE batch")
    ap.add_argument("--no-scan-sweep", action="store_true", help="skip the extra recurrence-kernel measurement at 4x batch")
    ap.add_argument("--no-one-batch-pass", action="store_true",
                    help="skip the extra pass of plain one-batch forwards (profiling runs that want only the grouped launches)")
    ap.add_argument("--self-contained", action="store_true",
                    help="enqueue the gated exact re-run kernels with every forward (no status check needed)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the output of the last timed step as DIR/y.npy (float64, the values "
                         "y * 2^-out_exp a caller of the forward receives; rank 0's batch; a fixed, seeded sample of frames "
                         "when the whole output exceeds 48 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    preset = {1: (0.5, 0.0, "w8a16", 32), 2: (0.5, 0.9, "w8a16", 32), 3: (1.0, 0.9, "w8a16", 512), 4: (1.0, 0.0, "w4a8", 32)}[args.config]
    args.dim_scale = preset[0] if args.dim_scale is None else args.dim_scale
    args.sparsity = preset[1] if args.sparsity is None else args.sparsity
    args.quantization = preset[2] if args.quantization is None else args.quantization
    args.batch = preset[3] if args.batch is None else args.batch

    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and args.gpus > 1:
        raise SystemExit(launch_ranks(args.gpus))
    if world_env is not None and int(world_env) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world_env}: start one rank per GPU and pass the same N")

    import numpy as np
    import torch

    import __graft_entry__ as graft
    graft.build()
    from sparsernns_amd import _lib, synth
    from sparsernns_amd.fxparray import FxpArray, RoundingMode, fxp_from_fp
    from sparsernns_amd.fxpmodel import build_regression_model

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # S5FXP_BENCH_BACKEND=gloo is a rehearsal aid: several ranks on ONE GPU (RCCL refuses duplicate devices), to
        # exercise this script's multi-rank branches without a multi-GPU node.  The driver's runs use RCCL.
        backend = os.environ.get("S5FXP_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
            dist.init_process_group(backend=backend)
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", torch.cuda.current_device())

    # config 3 is ONE batch of `--batch` (512) sequences sharded over the ranks (strong scaling); the others keep a fixed
    # per-GPU batch (weak scaling)
    sharded = args.config == 3
    if sharded:
        from sparsernns_amd.dist import shard_bounds
        lo, hi = shard_bounds(args.batch, world, rank)
        B, L = hi - lo, args.seq_len
        if world * B != args.batch:
            raise SystemExit(f"config 3: {args.batch} sequences do not split evenly over {world} ranks")
    else:
        B, L = args.batch, args.seq_len
    if args.state_headroom_bits is None:
        args.state_headroom_bits = 2 if args.sparsity > 0 else 1
    # one extra integer bit for the (never clipped) SSM state: see synth.make_model(state_headroom_bits)
    # the 8-bit activation recipe needs activations of order one: at the NDNS input scale (7e-4) the calibrated
    # 1/sqrt(var + 1e-5) of BatchNorm is ~300, which no non-negative exponent holds in 8 bits (synth.make_model raises);
    # the same settings as tests/test_gpu_parity.py's configs[4] case
    narrow = args.quantization == "w4a8"
    in_scale = args.input_scale if args.input_scale is not None else (300.0 if narrow else 1.0)
    if narrow and args.state_headroom_bits == 1:
        args.state_headroom_bits = 0
    md, qc, dims = synth.make_model(args.dim_scale, quantization=args.quantization, sparsity=args.sparsity,
                                    calib_L=256 if narrow else 1024, state_headroom_bits=args.state_headroom_bits,
                                    input_scale=in_scale)
    allreduce = None
    if args.global_exponents and world > 1:
        from sparsernns_amd.dist import make_exponent_allreduce
        allreduce = make_exponent_allreduce(via_host=dist.get_backend() != "nccl")
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    # S5FXP_BENCH_IGNORE_STATUS=1: timing of ABLATED builds only (tools/variant.py: their results are wrong by design and
    # would otherwise walk down the ladder or abort the run); never set for a number that is reported
    ablated = os.environ.get("S5FXP_BENCH_IGNORE_STATUS") == "1"
    if ablated:
        _lib.ST_REDO = 0
        eng.check_status = lambda lane=0: np.zeros(_lib.STATUS_WORDS, dtype=np.int32)
    # `inflight` batches are kept in flight, each on its own HIP stream and engine lane (engine.InflightRunner): the
    # recurrence of one batch (a latency chain on B*P/16 waves) overlaps the projections of the others.  Every lane
    # has its own resident input and output; a step = one forward over one batch, as before.
    depth = 1 if (allreduce or args.self_contained) else max(1, args.inflight)
    # G reference batches per launch set (one exponent group each; mode A and config 3's one global batch stay single)
    G = 1 if (allreduce or sharded) else max(1, min(args.groups, args.steps))
    from sparsernns_amd.engine import InflightRunner
    fxs, ys = [], []
    if sharded:
        for lane in range(depth):  # this rank's slice of the one global batch of lane `lane`
            x = np.concatenate([synth.make_input(1, L, dims["d_in"], seed=100000 * lane + lo + i, scale=in_scale) for i in range(B)])
            fxs.append(fxp_from_fp(x, bits=qc["encoder"]["inp_bits"], exp=qc["encoder"]["inp_exp"], signed=True,
                                   round_mode=RoundingMode.FLOOR))
    else:
        # max(G, depth) distinct batches per rank (generating one takes about a second on the host); a lane's launch set is G of
        # them starting at the lane's own offset, so no two sets in flight are the same tensor and every group of a set differs
        nb = max(G, depth)
        pool = [fxp_from_fp(synth.make_input(B, L, dims["d_in"], seed=1000 + 16 * rank + 4096 * j, scale=in_scale),
                            bits=qc["encoder"]["inp_bits"], exp=qc["encoder"]["inp_exp"], signed=True, round_mode=RoundingMode.FLOOR) for j in range(nb)]
        for lane in range(depth):
            data = torch.cat([pool[(lane + g) % nb].data for g in range(G)])
            fxs.append(FxpArray(data, pool[0].bits, pool[0].exp, True))
        del pool
    for lane in range(depth):
        ys.append(torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device=dev))
    fx, y = fxs[0], ys[0]
    n_ev = 2 * dims["n_layers"]
    nl = dims["n_layers"]

    def sync_all():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def n_sets(steps, g):
        return (steps + g - 1) // g

    def make_events(steps):
        # one layer's recurrence launch per launch set carries a pair of HIP events (rotating over the layers): the library
        # attaches them to the dispatch (hipExtLaunchKernelGGL start/stop events), so elapsed_time() is that launch's
        # own duration -- the quantity rocprofv3's kernel trace reports -- and nothing extra is enqueued
        events = [[None] * n_ev for _ in range(steps)]
        for k, evs in enumerate(events):
            for j in (2 * (k % nl), 2 * (k % nl) + 1):
                evs[j] = torch.cuda.Event(enable_timing=True)
                evs[j].record()  # torch creates the hipEvent lazily on the first record(); the C side needs the handle
        return events

    def scan_avg(events):
        ms = [events[k][2 * (k % nl)].elapsed_time(events[k][2 * (k % nl) + 1]) for k in range(len(events))]
        return float(np.mean(ms)) * 1e-3

    exact_mode = False

    def run(steps, d, events=None, g=None, gate_events=None):
        """`steps` forwards (= batches) as launch sets of g batches each (the last set takes what is left), d sets in flight.
        d > 1: optimistic mode (the gated exact re-run launches are dropped); the status words of every lane are checked
        afterwards and must not carry ST_REDO."""
        g = G if g is None else g
        sets = n_sets(steps, g)
        if d == 1:
            flags = 0 if (allreduce or args.self_contained) else type(eng).LEVEL_FLAGS[eng.level]
            for k in range(sets):
                gk = min(g, steps - k * g)
                eng.enqueue(fx.data, fx.bits, fx.exp, y, B, L, None, allreduce, flags=flags,
                            scan_events=events[k] if events else None, groups=gk, gate_events=gate_events[k] if gate_events else None)
            return None
        runner = InflightRunner(eng, d) if run.runner is None else run.runner
        run.runner = runner
        for k in range(sets):
            lane = k % d
            gk = min(g, steps - k * g)
            runner.submit(fxs[lane].data, fxs[lane].bits, fxs[lane].exp, ys[lane], B, L, check=False,
                          scan_events=events[k] if events else None, groups=gk)
        return runner

    run.runner = None

    def lanes_of(d):  # engine lanes the d batches in flight use: 0 for the one-at-a-time pass, the runner's own otherwise
        return [0] if d == 1 else [run.runner.lane_of(i) for i in range(d)]

    def check_all(d):
        bits = 0
        for lane in lanes_of(d):
            bits |= int(eng.check_status(lane)[0])
        if bits & _lib.ST_REDO:
            raise SystemExit("a state left the fast recurrence's exact range: the timed steps are invalid; "
                             "re-run with --self-contained")
        return bits

    # The optimistic kernels check the data they rely on.  If this model / input leaves their range (the pruned
    # synthetic model with one bit of state headroom does: its states outgrow 16 bits), every optimistic step would
    # have to be repeated with the exact kernels -- so the run switches to the exact kernels (S5FXP_FWD_EXACT: 32-bit
    # recurrence, four-byte-plane gate kernel), still with `inflight` batches in flight, BEFORE the timed region,
    # and says so in the JSON line.  That is what engine.InflightRunner does by itself after two ST_REDOs.
    fallback_note = None
    # setup, not warmup: one forward per lane so that every lane's workspace and status words exist and every kernel
    # has been loaded before anything is timed, however small --warmup / --steps are
    def setup_pass():  # every lane runs a full launch set: every batch of the input pool has been through the kernels
        run(depth * G, depth)
        torch.cuda.synchronize()
        b = 0
        for lane in lanes_of(depth):
            b |= int(eng.check_status(lane)[0])
        return b

    bits = setup_pass()
    while (bits & _lib.ST_REDO) and eng.level < 2:
        # climb the ladder before anything is timed: pair kernel -> quad kernel (int16 streams, full 16-bit bound) -> exact
        eng.level += 1
        fallback_note = ("states left the pair kernel's range: quad recurrence kernel (int16 streams) for every step" if eng.level == 1
                         else "states left the 16-bit fast range: exact kernels (S5FXP_FWD_EXACT) for every step")
        exact_mode = eng.level == 2
        bits = setup_pass()
    if bits & _lib.ST_REDO:
        raise SystemExit("the exact kernels reported ST_REDO: this cannot happen")
    run(args.warmup, depth)  # the W untimed warmup steps
    torch.cuda.synchronize()

    # ---- timed region: exactly K steps, barrier + synchronize on both sides
    events = make_events(n_sets(args.steps, G))
    sync_all()
    t0 = time.perf_counter()
    run(args.steps, depth, events)
    sync_all()
    dt = time.perf_counter() - t0
    st0 = check_all(depth)

    # ---- --dump-outputs: the output of the last timed step (batch K - 1: the last group of the last launch set, on lane
    # (sets - 1) % depth), taken now, before the passes below reuse the output buffers.  Its input is the same in every run
    # with the same arguments (seeded synthetic model and batches), so two builds can be compared output for output.
    if args.dump_outputs and rank == 0:
        sets = n_sets(args.steps, G)
        gk = args.steps - (sets - 1) * G
        y_last = ys[0 if depth == 1 else (sets - 1) % depth][(gk - 1) * B:gk * B].reshape(B * L, -1)
        rows, row_bytes = B * L, y_last.shape[1] * 8
        if rows * row_bytes > DUMP_BYTES:  # a fixed, seeded sample of frames, in order
            keep = np.sort(np.random.default_rng(0).choice(rows, DUMP_BYTES // row_bytes, replace=False))
            y_last = y_last[torch.from_numpy(keep).to(dev)]
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "y.npy"), y_last.cpu().numpy().astype(np.float64) / 2.0 ** eng.out_exp)

    # ---- the same K steps one launch set at a time (no overlap between sets), for reference; not the headline
    single, ev1, evg = None, None, None
    if depth > 1 or G > 1:
        ev1 = make_events(n_sets(args.steps, G))
        evg = make_events(n_sets(args.steps, G))  # ... and one layer's gate-kernel launch another pair
        run(G, 1)  # lane 0's workspace for G groups exists before the clock starts
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run(args.steps, 1, ev1, gate_events=evg)
        torch.cuda.synchronize()
        dt1 = time.perf_counter() - t1
        check_all(1)
        single = dict(ms_per_step=round(dt1 / args.steps * 1e3, 4), value=round(B * L * args.steps / dt1, 1),
                      scan_avg_kernel_us=round(scan_avg(ev1) * 1e6, 2), batches_per_launch=G)
    # ---- ... and plain forwards of ONE batch, one at a time: the launch the recurrence kernel's roofline is quoted on
    ev0 = None
    if G > 1 and not args.no_one_batch_pass:
        k0 = min(args.steps, 12 * nl)
        ev0 = make_events(k0)
        torch.cuda.synchronize()
        run(k0, 1, ev0, g=1)
        torch.cuda.synchronize()
        check_all(1)

    rank_values = None
    if dist is not None:
        # every rank's own clock over the same K steps: the slowest one is the job's (contract); all of them are reported so
        # that a scaling run can be read rank by rank against the N=1 line
        t = torch.zeros(world, dtype=torch.float64, device=dev)
        t[rank] = dt
        if dist.get_backend() != "nccl":
            t = t.cpu()
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        per_rank = [float(v) for v in t.tolist()]
        dt = max(per_rank)
        rank_values = dict(min=round(B * L * args.steps / max(per_rank), 1), max=round(B * L * args.steps / min(per_rank), 1),
                           per_rank=[round(B * L * args.steps / v, 1) for v in per_rank])
    frames = B * L * world * args.steps
    value = frames / dt
    total_bl = B * L * world

    # ---- roofline of the recurrence kernel: algorithmic bytes = 16*P per frame per layer.  Its launch duration is
    # taken where the kernel has the GPU to itself (the one-at-a-time pass of the same K steps when batches are in
    # flight: there its launches share the chip with other batches' projections and the bracket measures the
    # sharing, not the kernel -- that figure is reported beside it).
    scan_inflight_s = scan_avg(events)
    scan_avg_s = scan_avg(ev0) if ev0 is not None else (scan_avg(ev1) if ev1 is not None else scan_inflight_s)
    algo_bytes = B * L * dims["P"] * 16
    # optimistic forwards (everything but --self-contained / mode A) run the int16-stream variant of the kernel: the
    # algorithmic bytes stay SURVEY.md 8(d)'s 16*P per frame (the reference's int32 element type); what the kernel
    # actually moves is in `traffic` (PMC) and `stored_bytes_per_launch`
    optimistic = not (allreduce or args.self_contained or exact_mode)
    kinds = {_lib.lib.s5fxp_model_recurrence_kernel(eng._h, i) for i in range(nl)}
    if eng.level == 1:
        kinds = {min(k, 2) for k in kinds}
    opt_kernel = {0: "k_scan_lane", 1: "k_scan_quad_asm", 2: "k_scan_quad_asm16", 3: "k_scan_pair_asm", 4: "k_scan_pairl_asm"}[max(kinds)]
    scan_kernel = opt_kernel if optimistic else ("k_scan_quad32_asm" if exact_mode else "k_scan_quad_asm")
    # a layer compacted to its live states (s5fxp_model_live_states) runs the recurrence on half the state slots: status word
    # [8 + 8l + 6] of the last forward says how many (the algorithmic bytes stay 16 * P: the dead states are part of the model)
    stw = eng.lane_status(lanes_of(1)[0]).cpu().numpy()
    slots = [int(stw[8 + 8 * i + 6]) or dims["P"] for i in range(nl)]
    # ... and word [8 + 8l + 7] how many of those slots the two recurrence streams hold (the LDS-fed pair kernel on a layer
    # compacted to 32 slots stores and loads only the live ones): that is what the kernel moves
    stream_slots = [int(stw[8 + 8 * i + 7]) or slots[i] for i in range(nl)]
    stored = scan_stored_bytes(scan_kernel, algo_bytes) * sum(stream_slots) // (nl * dims["P"])
    traffic = pmc_traffic(B, L, dims["P"], scan_kernel, 1, stream_slots)
    moved = traffic if traffic is not None else stored
    def roof(bytes_algo, bytes_moved, seconds):
        """`frac` is quoted on the ALGORITHMIC bytes (16*P per frame, the reference's int32 element type);
        `frac_moved` on what the kernel really moves.  The optimistic kernels keep int16 streams and move half of the
        algorithmic bytes, so on a launch that fills the chip the algorithmic rate can exceed the HBM peak: a fraction
        above one is not a bandwidth fraction of anything, and `frac` then falls back to the moved bytes (and says so)."""
        fa, fm = bytes_algo / seconds / 1e9 / HBM_PEAK_GBS, bytes_moved / seconds / 1e9 / HBM_PEAK_GBS
        on_moved = fa > 1.0
        return dict(achieved=round((bytes_moved if on_moved else bytes_algo) / seconds / 1e9, 1), frac=round(fm if on_moved else fa, 4),
                    frac_basis="moved bytes (the algorithmic rate would exceed the peak)" if on_moved else "algorithmic bytes (SURVEY.md 8d)",
                    frac_algorithmic=round(fa, 4), frac_moved=round(fm, 4), avg_kernel_us=round(seconds * 1e6, 2),
                    algorithmic_bytes_per_launch=bytes_algo, moved_bytes_per_launch=bytes_moved)

    roofline = dict(bound="hbm", kernel=scan_kernel + " (the S5 recurrence)", peak=HBM_PEAK_GBS, unit="GB/s", traffic=traffic,
                    **roof(algo_bytes, moved, scan_avg_s),
                    stream_width="int32 arithmetic; " + ("int16 range-guarded streams (Bu in, states out): every stored state is checked against the "
                                                         "kernel's exactness bound by its consumer" if stored < algo_bytes else "int32 streams"),
                    moved_bytes_source="PMC (profiles/r03_scan_traffic.json: 2 x FETCH_SIZE + WRITE_SIZE)" if traffic is not None else "stream sizes",
                    launch=f"one reference batch per launch (B={B}), one launch at a time", state_slots_per_layer=slots, stream_slots_per_layer=stream_slots,
                    measured="HIP start/stop events attached to the launch (hipExtLaunchKernelGGL), one layer per launch set",
                    avg_kernel_us_in_the_timed_region=round(scan_inflight_s * 1e6, 2), batches_per_launch_in_the_timed_region=G)
    if ev1 is not None and G > 1:
        # The timed region is made of launches of G batches: THAT launch is the one the top-level figures describe (its algorithmic
        # bytes are G x 16 P B L; it moves a quarter to a half of them, so its fraction is quoted on the moved bytes: roof()).  The
        # plain one-batch launch -- a latency chain on B * P / 32 workgroups, the launch SURVEY.md 8(d) and the north star's
        # "40 % on the scan kernel" speak of -- stays beside it.
        tg = pmc_traffic(B, L, dims["P"], scan_kernel, G, stream_slots)
        one = {k: roofline[k] for k in ("achieved", "frac", "frac_basis", "frac_algorithmic", "frac_moved", "avg_kernel_us", "traffic",
                                        "algorithmic_bytes_per_launch", "moved_bytes_per_launch", "launch")}
        roofline.update(roof(G * algo_bytes, tg if tg is not None else G * stored, scan_avg(ev1)))
        roofline.update(traffic=tg, launch=f"{G} reference batches per launch (G x B = {G * B} sequences, one exponent group per batch), one launch "
                                           "set at a time", moved_bytes_source="PMC (profiles/r03_scan_traffic.json: 2 x FETCH_SIZE + WRITE_SIZE)" if tg is not None else "stream sizes",
                        one_batch_launch=one)

    # ---- the slowest kernel of the forward, measured the same way (events attached to its launches of the one-set-at-a-time pass):
    # the gate kernel (C projection + out2 + sigmoid gate).  SURVEY.md 8(d) defines no algorithmic byte count for it, so its
    # rate is on the bytes it moves (PMC passes of the same workload, when committed).
    gate_kernel = None
    if evg is not None and optimistic and not allreduce:
        try:
            gate_s = scan_avg(evg)
        except RuntimeError:  # the events were not attached (a path that does not run the fused gate kernel)
            gate_s = None
        if gate_s:
            tgk = pmc_traffic(B, L, dims["P"], "k_cgate_p", G, stream_slots)
            gate_kernel = dict(kernel="k_cgate_p (C projection + D u, out2, table sigmoid, gate, residual maxima)", avg_kernel_us=round(gate_s * 1e6, 2),
                               batches_per_launch=G, traffic=tgk,
                               achieved=round(tgk / gate_s / 1e9, 1) if tgk else None, unit="GB/s", peak=HBM_PEAK_GBS,
                               frac_moved=round(tgk / gate_s / 1e9 / HBM_PEAK_GBS, 4) if tgk else None,
                               note="VALU co-limited (DESIGN.md 4a): 51 M VALU instructions per 8-batch launch beside 0.68 GB of traffic")

    # ---- the recurrence kernel with more chains than one reference batch gives it (not the headline workload): at
    # B=32 its launch is a latency chain on 128 waves, whatever the bandwidth; the same kernel at 4x the batch shows
    # what it moves when the chip is filled.  Single stream, a few steps, rank 0 of a 1-GPU run only.
    scan_big = None
    if rank == 0 and world == 1 and optimistic and not args.no_scan_sweep and G == 1:
        Bb = 4 * B
        xb = synth.make_input(Bb, L, dims["d_in"], seed=77, scale=in_scale)
        fxb = fxp_from_fp(xb, bits=qc["encoder"]["inp_bits"], exp=qc["encoder"]["inp_exp"], signed=True,
                          round_mode=RoundingMode.FLOOR)
        yb = torch.empty((Bb, L, dims["d_out"]), dtype=torch.int32, device=dev)
        eng.enqueue(fxb.data, fxb.bits, fxb.exp, yb, Bb, L, flags=type(eng).LEVEL_FLAGS[eng.level], lane=9)
        evb = make_events(2 * nl)
        torch.cuda.synchronize()
        for k in range(2 * nl):
            eng.enqueue(fxb.data, fxb.bits, fxb.exp, yb, Bb, L, flags=type(eng).LEVEL_FLAGS[eng.level], lane=9, scan_events=evb[k])
        torch.cuda.synchronize()
        if not (int(eng.check_status(9)[0]) & _lib.ST_REDO):
            ab = Bb * L * dims["P"] * 16
            scan_big = dict(batch=Bb, unit="GB/s", **roof(ab, scan_stored_bytes(scan_kernel, ab), scan_avg(evb)),
                            note="same kernel, 4x the sequences in one launch (one exponent group); not the headline workload")
        del fxb, yb

    # ---- RCCL output gather (one all_gather_into_tensor of the int32 outputs over xGMI), outside the timed region: the
    # denoising pipeline consumes a rank's outputs on that rank (audio.py), so the gather is a reporting step.  Timed
    # over 3 repeats after one untimed call (communicator set-up); config 3 reports it as part of its contract.
    gather_ms = None
    if dist is not None:
        out = torch.empty((world,) + tuple(y.shape), dtype=torch.int32, device=dev)

        def gather():
            if dist.get_backend() == "nccl":
                dist.all_gather_into_tensor(out, y)
            else:  # rehearsal backend: through the host
                parts = [torch.empty_like(y, device="cpu") for _ in range(world)]
                dist.all_gather(parts, y.cpu())
                out.copy_(torch.stack(parts))

        gather()
        sync_all()
        g0 = time.perf_counter()
        for _ in range(3):
            gather()
        torch.cuda.synchronize()
        gather_ms = (time.perf_counter() - g0) * 1e3 / 3
        assert torch.equal(out[rank], y)

    # ---- CPU baseline: the scalar C oracle ("port") on a bounded sample of the same workload, rank 0 only
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:  # N=1 only: the host cores belong to one process there
        from oracle import cref
        cb = min(args.cpu_batch, B)
        cm = cref.CModel(model.export())
        comparable = cb == B  # compute_best couples the sequences of a batch: a sub-batch is a different computation
        xs_host = fx.data[:cb].cpu().numpy()
        passes, c0 = 0, time.perf_counter()
        while True:  # whole passes over the same cb sequences until ~cpu_seconds have gone (at least one)
            ref, _, _, _ = cm.forward(xs_host, fx.bits, fx.exp)
            passes += 1
            cdt = time.perf_counter() - c0
            if cdt >= args.cpu_seconds or passes >= 64:
                break
        same = bool(np.array_equal(ref, y[:cb].cpu().numpy())) if comparable else None
        cpu = dict(value=round(passes * cb * L / cdt, 1), unit="frames/s", cores=cref.num_threads(), kind="port",
                   sample=f"{passes} passes over {cb} sequences x {L} frames of the same workload (lane 0's batch), "
                          f"OpenMP scalar C restatement (oracle/s5fxp_ref.c); the reference's JAX path is not "
                          f"installable offline",
                   seconds=round(cdt, 2), matches_gpu=same)

    if rank == 0:
        line = dict(
            metric="frames/sec at w8a16 S5 dim_scale=0.5 (NDNS shape), bit-exact vs CPU fxprun",
            value=round(value, 1), unit="frames/s", n_gpus=world, steps=args.steps, warmup=args.warmup,
            ms_per_step=round(dt / args.steps * 1e3, 4), higher_is_better=True, scaling="strong" if sharded else "weak",
            vs_baseline=None, dtype="int32", data="synthetic",
            config=dict(workload=f"BASELINE configs[{args.config}]: dim_scale={args.dim_scale} {args.quantization} "
                                 f"{'dense' if args.sparsity == 0 else f'{args.sparsity:.0%} sparse'} S5, " +
                                 (f"ONE batch of {args.batch} x L={L} sharded over {world} GPU(s), " if sharded
                                  else f"B={B} x L={L} per GPU, ") +
                                 f"H={dims['H']}, P={dims['P']}, 3 layers, d_in=d_out=257",
                        batch_per_gpu=B, seq_len=L, exponent_mode="global (all-reduce MAX)" if allreduce else "per-shard",
                        parallelism=f"batch-sharded x{world}", batches_per_launch=G, launch_sets_in_flight=depth,
                        batches_in_flight=depth * G,
                        stream_width="int32 arithmetic and model input / output; int16 activations between kernels and int16 "
                                     "range-guarded recurrence streams (a value outside the guarded range repeats the batch on "
                                     "the exact int32 kernels)"),
            roofline=roofline, gate_kernel=gate_kernel, recurrence_kernel_at_4x_batch=scan_big, cpu_baseline=cpu, single_stream=single,
            mode="ABLATED BUILD, STATUS IGNORED: not a result" if ablated else (fallback_note or ("optimistic" if optimistic else "self-contained")),
            status_bits=int(st0),
            output_gather_ms=gather_ms, rank_values=rank_values)
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
