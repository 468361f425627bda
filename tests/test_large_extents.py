"""The integer model's forwards at extents past 2^31 and 2^32 bytes (and 2^31 elements) per plane, where "wave-uniform base +
32-bit offset" addressing is only right while the base is formed in 64 bits, and the size queries at arguments whose true
size does not fit a size_t.

References (tests/large_extents.py): the C oracle's run of R = 7 sequences, which a batch of k copies must repeat bit for bit.
Every test first asserts from its shapes, in Python integers, that each plane it claims to stress is beyond its threshold; the
only way a case is left out is the memory guard's skip.

  S1  B = 7 * 150, L = 4099: 4.3 M frames.  x, y (int32) and both state streams pass 2^32 bytes, every int16 plane 2^30.
  S2  B = 7 * 390, L = 4099: 11.2 M frames.  Every int16 plane passes 2^32 bytes, every plane 2^31 elements.
"""
import time

import numpy as np
import pytest

import large_extents as LX
from large_extents import L_REP, P30, P31, P32, R

pytestmark = pytest.mark.gpu

S1_B, S2_B = R * 150, R * 390


def _report(name, t0, **figures):
    """One line per case for the GPU log: wall time and the largest plane."""
    print(f"[large] {name}: {time.perf_counter() - t0:.2f} s " + " ".join(f"{k}={v}" for k, v in figures.items()), flush=True)


def _largest(sizes):
    return max(b for _, b in sizes.values())


def _claims(which, ds, sizes):
    """The thresholds of the issue, asserted from shapes."""
    if which == "S1":
        LX.assert_exceeds(sizes, ("x", "y", "stream"), nbytes=P32)
        LX.assert_exceeds(sizes, ("h",), nbytes=P30)
    elif ds == 1.0:   # S2
        LX.assert_exceeds(sizes, ("h", "x", "y", "stream"), nbytes=P32, elements=P31)
    else:             # S2's B at dim_scale 0.5
        LX.assert_exceeds(sizes, ("x", "y", "stream"), nbytes=P32)
        LX.assert_exceeds(sizes, ("h",), nbytes=P31)


def _need(eng, B, L, io_bytes, ref_numel, groups=1):
    from sparsernns_amd._lib import lib
    ws = lib.s5fxp_workspace_bytes(eng._h, B, L)
    assert ws > 0
    return groups * (B * L * (eng.d_in + eng.d_out) * io_bytes + ws) + LX.chunk_bytes(ref_numel)


@pytest.mark.parametrize("which,ds", [("S1", 1.0), ("S2", 0.5), ("S2", 1.0)])
def test_forward_int32_repeats_the_oracle(which, ds):
    """Engine.forward on the fused path: k copies of the 7 sequences give k copies of the oracle's output."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray

    t0 = time.perf_counter()
    small, dims = LX.small_run(ds), LX.model(ds)[2]
    B = S1_B if which == "S1" else S2_B
    sizes = LX.plane_sizes(B, L_REP, dims)
    _claims(which, ds, sizes)
    eng = LX.engine(ds)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    free = LX.memory_guard(_need(eng, B, L_REP, 4, small["ref"].size), f"{which} at dim_scale {ds}")
    x = LX.repeated(LX.dev(small["xi"]), B // R)
    ref = LX.dev(small["ref"])
    t1 = time.perf_counter()
    y = eng.forward(FxpArray(x, small["x_bits"], small["x_exp"]))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert (y.bits, y.exp) == (small["bits"], small["exp"])
    assert int(eng.status[2].item()) == _lib.PATH_FUSED
    LX.assert_repeats(y.data, ref, f"{which} ds {ds} int32")
    _report(f"forward_int32[{which}-{ds}]", t0, frames=B * L_REP, largest_plane=_largest(sizes), forward_s=f"{t2 - t1:.3f}",
            free=free, rungs=[int(eng.status[8 + 8 * i + 5].item()) for i in range(eng.n_layers)])
    del x, y, ref, eng
    LX.release()


RUNG_WALKS = (("1.0", 1.0, S1_B), ("1.0 with two bits of state headroom", "1.0h2", S1_B), ("0.5", 0.5, S2_B))


def test_forward_int32_on_every_rung():
    """The walk of test_long_and_ragged_sequences_on_every_rung -- the pair rung, the quad16 rung (FWD_NO_PAIR), the exact
    kernels, the self-contained forward (flags 0) -- at S1 on the dim_scale 1.0 models and at S2's B on the 0.5 model, where
    its P = 64 streams pass 2^32 bytes too.

    An optimistic forward (FWD_DEFER_REDO) whose states leave its rung's range reports ST_REDO and leaves y to the caller's
    repeat: that is the model's range, not an addressing matter, and the same for k copies as for one -- so the 7-sequence
    forward with the same flags must report it as well, and y is compared wherever it is not reported.  EXACT and flags 0 are
    always compared.  Measured on an MI355X: the pair rung is out of range at dim_scale 1.0 with one bit of headroom and in
    range on the other two models; all other rungs are in range everywhere.  The last assertions pin that, so that no rung
    drops out of this test unnoticed."""
    import torch
    from sparsernns_amd import _lib

    optimistic = (_lib.FWD_DEFER_REDO, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR)
    verified = {}
    for name, ds, B in RUNG_WALKS:
        t0 = time.perf_counter()
        small, dims = LX.small_run(ds), LX.model(ds)[2]
        sizes = LX.plane_sizes(B, L_REP, dims)
        LX.assert_exceeds(sizes, ("x", "y", "stream"), nbytes=P32)
        LX.assert_exceeds(sizes, ("h",), nbytes=P30 if B == S1_B else P31)
        eng = LX.engine(ds)
        LX.memory_guard(_need(eng, B, L_REP, 4, small["ref"].size), f"rungs at dim_scale {name}")
        xs = LX.dev(small["xi"])
        x, ref = LX.repeated(xs, B // R), LX.dev(small["ref"])
        y = torch.empty((B, L_REP, eng.d_out), dtype=torch.int32, device="cuda")
        ys = torch.empty((R, L_REP, eng.d_out), dtype=torch.int32, device="cuda")
        seen = {}
        for flags in optimistic + (_lib.FWD_EXACT, 0):
            eng.enqueue(xs, small["x_bits"], small["x_exp"], ys, R, L_REP, flags=flags)
            redo_small = bool(eng.check_status()[0] & _lib.ST_REDO)
            y.fill_(-7)
            eng.enqueue(x, small["x_bits"], small["x_exp"], y, B, L_REP, flags=flags)
            st = eng.check_status()
            redo = bool(st[0] & _lib.ST_REDO)
            assert redo == redo_small, f"{name} flags {flags}: ST_REDO {redo} for k copies, {redo_small} for one"
            if flags in optimistic and redo:
                continue
            LX.assert_repeats(y, ref, f"{name} flags {flags}")
            seen[flags] = [int(st[8 + 8 * i + 5]) for i in range(eng.n_layers)]
        verified[ds] = seen
        _report(f"rungs[{name}]", t0, frames=B * L_REP, largest_plane=_largest(sizes), kernels_verified=seen)
        del x, xs, y, ys, ref, eng
        LX.release()
    pair, quad16 = optimistic
    assert set(verified[1.0]) >= {quad16, _lib.FWD_EXACT, 0} and set(verified[0.5]) == {pair, quad16, _lib.FWD_EXACT, 0}, verified
    assert pair in verified["1.0h2"], verified


@pytest.mark.parametrize("io,which", [("float32", "S1"), ("int16", "S1"), ("int16", "S2")])
def test_forward_float_and_int16_repeat_the_oracle(io, which):
    """forward_float and forward_int16 (other encoder and decoder bodies) at dim_scale 1.0, against the oracle's output
    through exact to_float / exact narrowing."""
    import torch

    t0 = time.perf_counter()
    ds = 1.0
    small, dims = LX.small_run(ds), LX.model(ds)[2]
    B = S1_B if which == "S1" else S2_B
    io_bytes = 4 if io == "float32" else 2
    sizes = LX.plane_sizes(B, L_REP, dims, io_bytes=io_bytes)
    if which == "S1":
        LX.assert_exceeds(sizes, ("stream",) + (("x", "y") if io == "float32" else ()), nbytes=P32)
        LX.assert_exceeds(sizes, ("h",), nbytes=P30)
        if io == "int16":
            LX.assert_exceeds(sizes, ("x", "y"), nbytes=P31)
    else:
        LX.assert_exceeds(sizes, ("h", "x", "y", "stream"), nbytes=P32, elements=P31)
    eng = LX.engine(ds)
    ref_i = small["ref"]
    LX.memory_guard(_need(eng, B, L_REP, io_bytes, ref_i.size * io_bytes), f"{io} {which}")
    if io == "float32":
        assert 0 <= small["exp"] <= 31 and int(np.abs(ref_i).max()) < 1 << 24   # to_float is then exact in float32
        ref = torch.from_numpy((ref_i.astype(np.float64) / float(1 << small["exp"])).astype(np.float32)).cuda()
        x = LX.repeated(LX.dev(small["xf"]), B // R)
        y = eng.forward_float(x, small["x_bits"], small["x_exp"])
    else:
        assert small["x_bits"] <= 16 and small["bits"] <= 16
        assert int(np.abs(ref_i).max()) < 1 << 15 and int(np.abs(small["xi"]).max()) < 1 << 15   # the narrowing loses nothing
        ref = torch.from_numpy(ref_i.astype(np.int16)).cuda()
        x = LX.repeated(torch.from_numpy(small["xi"].astype(np.int16)).cuda(), B // R)
        y = eng.forward_int16(x, small["x_bits"], small["x_exp"])
    torch.cuda.synchronize()
    assert (eng.out_bits, eng.out_exp) == (small["bits"], small["exp"])
    LX.assert_repeats(y, ref, f"{io} {which}")
    _report(f"forward_{io}[{which}]", t0, frames=B * L_REP, largest_plane=_largest(sizes))
    del x, y, ref, eng
    LX.release()


GROUPS, GROUP_B = 50, R * 3   # 50 groups of 21 sequences: S1 in all


def _grouped_claims(eng, dims):
    """The later groups of a grouped call lie beyond 2^32 bytes of x, of y and of the workspace."""
    from sparsernns_amd._lib import lib
    assert GROUPS >= 6 and GROUPS * GROUP_B == S1_B
    ws_one = lib.s5fxp_workspace_bytes(eng._h, GROUP_B, L_REP)
    n = GROUP_B * L_REP
    assert (GROUPS - 1) * ws_one > P32 and (GROUPS - 1) * n * dims["d_in"] * 4 > P32 and (GROUPS - 1) * n * dims["d_out"] * 4 > P32
    return ws_one


def test_forward_batches_at_s1():
    """forward_batches: 50 groups, each a batch of 3 copies of the 7 sequences and its own compute_best batch."""
    import torch
    from sparsernns_amd.fxparray import FxpArray

    t0 = time.perf_counter()
    ds = 1.0
    small, dims = LX.small_run(ds), LX.model(ds)[2]
    eng = LX.engine(ds)
    ws_one = _grouped_claims(eng, dims)
    n = GROUP_B * L_REP
    LX.memory_guard(GROUPS * (n * (eng.d_in + eng.d_out) * 4 + ws_one) + LX.chunk_bytes(small["ref"].size), "forward_batches S1")
    x = LX.repeated(LX.dev(small["xi"]), S1_B // R)
    ref = LX.dev(small["ref"])
    y = eng.forward_batches(FxpArray(x, small["x_bits"], small["x_exp"]), GROUP_B)
    torch.cuda.synchronize()
    assert (y.bits, y.exp) == (small["bits"], small["exp"])
    LX.assert_repeats(y.data, ref, "forward_batches S1")
    _report("forward_batches[S1]", t0, groups=GROUPS, frames=S1_B * L_REP, last_group_ws_offset=(GROUPS - 1) * ws_one)
    del x, y, ref, eng
    LX.release()


def test_inflight_runner_two_grouped_sets_at_s1():
    """The same grouped call through InflightRunner, two sets in flight on their own streams and lanes."""
    import torch
    from sparsernns_amd.engine import InflightRunner

    t0 = time.perf_counter()
    ds, sets = 1.0, 2
    small, dims = LX.small_run(ds), LX.model(ds)[2]
    eng = LX.engine(ds)
    ws_one = _grouped_claims(eng, dims)
    n = GROUP_B * L_REP
    LX.memory_guard(sets * GROUPS * (n * (eng.d_in + eng.d_out) * 4 + ws_one) + LX.chunk_bytes(small["ref"].size),
                    "InflightRunner, two S1 sets")
    ref = LX.dev(small["ref"])
    xs = LX.dev(small["xi"])
    runner = InflightRunner(eng, depth=sets)
    jobs = []
    for _ in range(sets):
        x = LX.repeated(xs, S1_B // R)
        y = torch.empty((S1_B, L_REP, eng.d_out), dtype=torch.int32, device="cuda")
        runner.submit(x, small["x_bits"], small["x_exp"], y, GROUP_B, L_REP, groups=GROUPS)
        jobs.append((x, y))
    runner.drain()
    for s, (_, y) in enumerate(jobs):
        LX.assert_repeats(y, ref, f"in-flight set {s}")
    _report("inflight_two_sets[S1]", t0, groups=GROUPS, frames=sets * S1_B * L_REP)
    del jobs, x, y, xs, ref, runner, eng
    LX.release()


def test_generic_engine_past_2_32_bytes_per_int32_plane():
    """MODEL_FORCE_GENERIC (s5fxp_kernels.hpp: int32 planes, flat indices) at the smallest multiple of 7 sequences whose
    int32 (N, H) planes pass 2^32 bytes."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray

    t0 = time.perf_counter()
    ds = 1.0
    small, dims = LX.small_run(ds), LX.model(ds)[2]
    B = R * (P32 // (4 * dims["H"] * L_REP * R) + 1)
    assert (B - R) * L_REP * dims["H"] * 4 <= P32   # the smallest
    sizes = LX.plane_sizes(B, L_REP, dims, h_bytes=4)
    LX.assert_exceeds(sizes, ("h", "x", "y", "stream"), nbytes=P32)
    eng = LX.engine(ds, _lib.MODEL_FORCE_GENERIC)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 0
    LX.memory_guard(_need(eng, B, L_REP, 4, small["ref"].size), "generic engine")
    x = LX.repeated(LX.dev(small["xi"]), B // R)
    ref = LX.dev(small["ref"])
    t1 = time.perf_counter()
    y = eng.forward(FxpArray(x, small["x_bits"], small["x_exp"]))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert (y.bits, y.exp) == (small["bits"], small["exp"])
    assert int(eng.status[2].item()) == _lib.PATH_GENERIC
    LX.assert_repeats(y.data, ref, "generic engine")
    _report("generic", t0, B=B, frames=B * L_REP, largest_plane=_largest(sizes), forward_s=f"{t2 - t1:.3f}")
    del x, y, ref, eng
    LX.release()


# ---- one long sequence ------------------------------------------------------------------------------------------------------

def _extent_limit_L(P):
    """The largest L stream_extent_ok (s5fxp_api.hip) accepts: ((L + 3) / 4 + 2 * SCAN_DEPTH) * P * 32 < 2^32 - 1."""
    ok = lambda L: ((L + 3) // 4 + 2 * LX.SCAN_DEPTH) * P * 32 < 0xffffffff
    blocks = (0xffffffff - 1) // (32 * P) - 2 * LX.SCAN_DEPTH
    L = 4 * blocks
    assert ok(L) and not ok(L + 1) and 0 < L < P31
    return L


@pytest.mark.parametrize("ds", [1.0, 0.5])
def test_one_sequence_at_the_extent_limit_matches_the_generic_engine(ds):
    """B = 1, L the largest the recurrence kernels' 32-bit buffer extent allows (P = 128: 4.19 M frames; P = 64: 8.39 M):
    repetition cannot help, the independent generic kernels are the reference.  Same y, same status error bits."""
    import torch
    from sparsernns_amd import _lib, synth
    from sparsernns_amd._lib import lib

    t0 = time.perf_counter()
    export, qc, dims = LX.model(ds)
    L = _extent_limit_L(dims["P"])
    sizes = LX.plane_sizes(1, L, dims)
    LX.assert_exceeds(sizes, ("x", "y"), nbytes=P32)
    assert sizes["stream"][1] > P32 - (1 << 20)   # the stream is AT its limit: within 1 MiB of 2^32 bytes
    fused, generic = LX.engine(ds), LX.engine(ds, _lib.MODEL_FORCE_GENERIC)
    need = (L * (2 * dims["d_out"] + 2 * dims["d_in"]) * 4 + lib.s5fxp_workspace_bytes(fused._h, 1, L) +
            lib.s5fxp_workspace_bytes(generic._h, 1, L) + (64 << 20))
    LX.memory_guard(need, f"one sequence of {L} frames")
    # the input: a block of oracle-style rows repeated along time (the recurrence makes the OUTPUT aperiodic)
    blk = 4099
    xf = synth.make_input(1, blk, dims["d_in"], seed=5)
    from oracle import fxp_oracle as O
    fx = O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    xs = torch.from_numpy(np.ascontiguousarray(fx.data.astype(np.int32)[0])).cuda()
    x = xs.repeat((-(-L // blk), 1))[:L].contiguous().view(1, L, dims["d_in"])
    del xs
    ys = []
    words = []
    for eng in (fused, generic):
        y = torch.empty((1, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        t1 = time.perf_counter()
        eng.run_ladder(lambda fl: eng.enqueue(x, fx.bits, fx.exp, y, 1, L, flags=fl), eng.check_status)
        st = eng.check_status()
        words.append((int(st[0]) & ~_lib.ST_REDO, int(st[2]), time.perf_counter() - t1))
        ys.append(y)
    assert words[0][1] == _lib.PATH_FUSED and words[1][1] == _lib.PATH_GENERIC
    assert words[0][0] == words[1][0], "status error bits differ"
    assert (fused.out_bits, fused.out_exp) == (generic.out_bits, generic.out_exp)
    step = 1 << 18
    for r0 in range(0, L, step):
        assert bool((ys[0][0, r0:r0 + step] == ys[1][0, r0:r0 + step]).all()), f"rows {r0} .. {r0 + step} differ"
    _report(f"one_sequence[{ds}]", t0, L=L, largest_plane=_largest(sizes), fused_s=f"{words[0][2]:.3f}", generic_s=f"{words[1][2]:.3f}")
    del x, y, ys, fused, generic, eng
    LX.release()


@pytest.mark.parametrize("ds", [1.0, 0.5])
def test_one_block_above_the_extent_limit_is_refused(ds):
    """Host only: L one 4-step block above the limit returns S5FXP_EBADARG from the three boundaries and from the grouped call,
    before any launch (the pointers are small real buffers, the workspace size is a claim)."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib

    dims = LX.model(ds)[2]
    eng = LX.engine(ds)
    L = _extent_limit_L(dims["P"]) + 4
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.full((1024,), -7, dtype=torch.int32, device="cuda")
    st = eng.lane_status(0, 2)
    st.fill_(-9)
    opts = _lib.ForwardOpts()
    opts.groups = 2
    import ctypes as C
    for fn, q in ((lib.s5fxp_model_forward, lib.s5fxp_workspace_bytes), (lib.s5fxp_model_forward_f32, lib.s5fxp_workspace_bytes_f32),
                  (lib.s5fxp_model_forward_i16, lib.s5fxp_workspace_bytes_i16)):
        assert 0 < q(eng._h, 1, L) < 1 << 62
        for o in (None, C.byref(opts)):
            rc = fn(eng._h, buf.data_ptr(), eng.inp_bits, eng.inp_exp, 1, L, buf.data_ptr(), buf.data_ptr(), 1 << 62, st.data_ptr(),
                    None, o, stream)
            assert rc == _lib.S5FXP_EBADARG, (fn, o is not None, rc)
    torch.cuda.synchronize()
    assert bool((buf == -7).all()) and bool((st == -9).all()), "something was launched"
    del eng
    LX.release()


# ---- the size queries -------------------------------------------------------------------------------------------------------

INT_MAX = 2 ** 31 - 1
SIZE_MAX = 2 ** 64 - 1


def _query_Bs():
    return sorted({2 ** k for k in range(0, 31)} | {2 ** k - 1 for k in range(20, 32)} | {INT_MAX})


@pytest.mark.parametrize("ds", [1.0, 0.5])
def test_size_queries_never_wrap(ds):
    """s5fxp_workspace_bytes and its _f32 / _i16 forms on real handles (fused and generic), s5fxp_clips_workspace_bytes and
    s5fxp_float_workspace_bytes: over B = 2^k up to INT_MAX, at L = 1, 4099 and the extent limit, the answer is 0 or at least the
    Python-integer lower bound (5 B L H 2 bytes for the model's forwards), and once 0 it stays 0 as B grows."""
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib

    dims = LX.model(ds)[2]
    H, P = dims["H"], dims["P"]
    Ls = (1, L_REP, _extent_limit_L(P))
    engines = {"fused": LX.engine(ds), "generic": LX.engine(ds, _lib.MODEL_FORCE_GENERIC)}
    wrapped = []
    for kind, eng in engines.items():
        for qname in ("s5fxp_workspace_bytes", "s5fxp_workspace_bytes_f32", "s5fxp_workspace_bytes_i16"):
            q = getattr(lib, qname)
            for L in Ls:
                was_zero = False
                for B in _query_Bs():
                    got, low = q(eng._h, B, L), 5 * B * L * H * 2
                    if got == 0:
                        was_zero = True
                        # 0 is owed only when the size cannot be told: never below a generous upper bound of the true size
                        assert 16 * low > SIZE_MAX or B * L * (H + P + dims["d_in"]) * 64 > SIZE_MAX, (kind, qname, B, L)
                    elif got < low or was_zero:
                        wrapped.append((kind, qname, B, L, got, low))
    assert not wrapped, f"{len(wrapped)} answers wrapped, e.g. (engine, query, B, L, got, lower bound) {wrapped[:4]}"
    # the clip scratch: 4 n Lmax H bytes
    eng = engines["fused"]
    for Lmax in (1, L_REP, 1 << 20):
        was_zero = False
        for n in _query_Bs():
            got, true = lib.s5fxp_clips_workspace_bytes(eng._h, n, Lmax), 4 * n * Lmax * H
            assert got == (true if true <= SIZE_MAX else 0) and not (was_zero and got), (n, Lmax, got, true)
            was_zero = was_zero or got == 0
    del engines, eng
    LX.release()


def test_forwards_refuse_a_size_that_does_not_fit_before_any_launch():
    """(B, L) whose workspace does not fit a size_t, and a grouped call whose G-fold does not: S5FXP_EWORKSPACE (the clip
    entries: S5FXP_EBADARG, as for any workspace that is too small) whatever workspace_bytes claims, and nothing is launched."""
    import ctypes as C
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib

    ds = 1.0
    dims = LX.model(ds)[2]
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.full((1024,), -7, dtype=torch.int32, device="cuda")
    Llim = _extent_limit_L(dims["P"])
    claim = 1 << 63
    for flags in (0, _lib.MODEL_FORCE_GENERIC):
        eng = LX.engine(ds, flags)
        st = eng.lane_status(0, 2)
        st.fill_(-9)
        assert lib.s5fxp_workspace_bytes(eng._h, INT_MAX, Llim) == 0
        opts = _lib.ForwardOpts()
        opts.groups = INT_MAX
        B1 = 1 << 20
        one = lib.s5fxp_workspace_bytes(eng._h, B1, Llim)
        assert one > 0 and one * INT_MAX > SIZE_MAX
        for fn in (lib.s5fxp_model_forward, lib.s5fxp_model_forward_f32, lib.s5fxp_model_forward_i16):
            rc = fn(eng._h, buf.data_ptr(), eng.inp_bits, eng.inp_exp, INT_MAX, Llim, buf.data_ptr(), buf.data_ptr(), claim,
                    st.data_ptr(), None, None, stream)
            assert rc == _lib.S5FXP_EWORKSPACE, (flags, fn, rc)
            rc = fn(eng._h, buf.data_ptr(), eng.inp_bits, eng.inp_exp, B1, Llim, buf.data_ptr(), buf.data_ptr(), SIZE_MAX,
                    st.data_ptr(), None, C.byref(opts), stream)
            assert rc == _lib.S5FXP_EWORKSPACE, (flags, fn, "grouped", rc)
        # the layer entry, at an L its own extent check passes
        rc = lib.s5fxp_layer_forward(eng._h, 0, buf.data_ptr(), 16, 8, INT_MAX, Llim, buf.data_ptr(), None, buf.data_ptr(), claim,
                                     st.data_ptr(), None, None, stream)
        assert rc == _lib.S5FXP_EWORKSPACE, (flags, "layer", rc)
        torch.cuda.synchronize()
        assert bool((buf == -7).all()) and bool((st == -9).all()), "something was launched"
        del eng
    LX.release()


# ---- many clips, many step groups -------------------------------------------------------------------------------------------

SENTINEL = -123456789
CLIP_LENS = (L_REP, 0, 1, L_REP + 901, 33)   # cycled; the fourth is above Lmax and is clamped to it


def test_clips_past_2_32_bytes_of_y():
    """s5fxp_model_clips: n clips of Lmax = 4099 frames with n * Lmax * 1028 > 2^32 (and n * Lmax * 768 > 2^32 bytes of
    scratch); lengths cycle through CLIP_LENS, contents
    through the 7 sequences (period 35).  Every clip equals the oracle's B = 1 run of its content and length, padding rows of y
    keep their sentinel, and every clip's status words equal those of the first period."""
    import torch
    from oracle import cref
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib

    t0 = time.perf_counter()
    ds, Lmax = 1.0, L_REP
    export, qc, dims = LX.model(ds)
    small = LX.small_run(ds)
    period = R * len(CLIP_LENS)
    k = P32 // (period * Lmax * dims["H"] * 4) + 1   # the clips' int16 scratch (4 n Lmax H bytes) passes 2^32 bytes as well
    n = k * period
    assert n * Lmax * dims["d_out"] * 4 > P32 and n * Lmax * dims["d_in"] * 4 > P32
    eng = LX.engine(ds)
    assert eng.clips_ok(Lmax)
    ws = lib.s5fxp_clips_workspace_bytes(eng._h, n, Lmax)
    assert ws == 4 * n * Lmax * dims["H"] and ws > P32
    LX.memory_guard(n * Lmax * (dims["d_in"] + dims["d_out"]) * 4 + ws + LX.COPIES_PER_CHUNK * period * Lmax * dims["d_out"],
                    f"{n} clips of {Lmax} frames")
    # the expected period: clip e has content e % 7 and length CLIP_LENS[e % 5]
    cm = cref.CModel(export)
    runs = {}
    want = np.full((period, Lmax, dims["d_out"]), SENTINEL, dtype=np.int32)
    lens = np.array([CLIP_LENS[e % len(CLIP_LENS)] for e in range(period)], dtype=np.int32)
    for e in range(period):
        c, ln = e % R, min(int(lens[e]), Lmax)
        if ln and (c, ln) not in runs:
            y1, b1, e1, _ = cm.forward(small["xi"][c, :ln], small["x_bits"], small["x_exp"])
            assert (b1, e1) == (eng.out_bits, eng.out_exp)
            runs[(c, ln)] = y1
        if ln:
            want[e, :ln] = runs[(c, ln)]
    xs = LX.dev(small["xi"])
    x = LX.repeated(xs[torch.arange(period, device="cuda") % R], k)
    lens_d = LX.repeated(torch.from_numpy(lens).cuda(), k)
    y = torch.full((n, Lmax, dims["d_out"]), SENTINEL, dtype=torch.int32, device="cuda")
    t1 = time.perf_counter()
    eng.clips(x, lens_d, y, x_bits=small["x_bits"], x_exp=small["x_exp"])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    st = eng.lane_status(0, n)[:n * _lib.STATUS_WORDS].view(k, period, _lib.STATUS_WORDS)
    assert bool((st == st[:1]).all()), "status words differ between the periods"
    st0 = st[0].cpu().numpy()
    assert not (st0[:, 0] & (_lib.ST_NEGSHIFT | _lib.ST_NEGEXP | _lib.ST_WIDE_INPUT)).any(), st0[:, 0]
    assert (st0[lens > 0, 2] == _lib.PATH_CLIP).all()
    LX.assert_repeats(y, torch.from_numpy(want).cuda(), "clips")
    _report("clips", t0, n=n, y_bytes=n * Lmax * dims["d_out"] * 4, scratch_bytes=ws, launch_s=f"{t2 - t1:.3f}")
    del x, y, xs, lens_d, st, eng
    LX.release()


STEP_B, STEP_L = 4, 8   # 32 rows per group


def _step_small(eng, cm, small, dims):
    """Seven groups of (STEP_B, STEP_L) rows with a carry left by an earlier chunk: x, carry in, and -- checked against the
    oracle here -- y, carry out and the status words of one Engine.step."""
    import torch
    from sparsernns_amd import _lib
    xi = small["xi"]
    cut = lambda r0: np.ascontiguousarray(np.stack([xi[g, r0 + 100 * g:r0 + 100 * g + STEP_B * STEP_L] for g in range(R)])
                                          .reshape(R, STEP_B, STEP_L, dims["d_in"]))
    warm, xs = cut(0), cut(50)
    shape = (R, eng.n_layers, 2, STEP_B, eng.P)
    zero = torch.zeros(shape, dtype=torch.int32, device="cuda")
    carry = torch.empty(shape, dtype=torch.int32, device="cuda")
    eng.step(torch.from_numpy(warm).cuda(), zero, B=STEP_B, L=STEP_L, groups=R, x_bits=small["x_bits"], x_exp=small["x_exp"],
             state_out=carry)
    x = torch.from_numpy(xs).cuda()
    out = torch.empty(shape, dtype=torch.int32, device="cuda")
    y = eng.step(x, carry, B=STEP_B, L=STEP_L, groups=R, x_bits=small["x_bits"], x_exp=small["x_exp"], state_out=out)
    torch.cuda.synchronize()
    st = eng.lane_status(0, R)[:R * _lib.STATUS_WORDS].clone()
    assert int(carry.abs().max()) > 0 and not bool((st.view(R, -1)[:, 0] & ~_lib.ST_REDO).any())
    cin = carry.cpu().numpy()
    for g in range(R):
        s = np.ascontiguousarray(cin[g])
        ref = cm.forward(xs[g], small["x_bits"], small["x_exp"], state=s)[0]
        assert np.array_equal(y[g].cpu().numpy(), ref) and np.array_equal(out[g].cpu().numpy(), s), f"small step, group {g}"
    return x, carry, y, out, st


def test_step_groups_past_2_32_bytes():
    """s5fxp_model_step: G groups of 32 rows with G * 32 * 1028 > 2^32 (one workgroup each), carry in and out; contents cycle
    through 7 groups.  y, the carry and all status words equal the 7-group run's, which is held to the oracle.  Then
    s5fxp_model_step_ragged once at the same n, slots permuted."""
    import torch
    from oracle import cref
    from sparsernns_amd import _lib

    t0 = time.perf_counter()
    ds = 1.0
    export, qc, dims = LX.model(ds)
    small = LX.small_run(ds)
    eng = LX.engine(ds)
    assert eng.step_ok(STEP_B, STEP_L)
    rows = STEP_B * STEP_L
    k = P32 // (R * rows * dims["d_out"] * 4) + 1
    G = k * R
    assert G * rows * dims["d_out"] * 4 > P32 and G * rows * dims["d_in"] * 4 > P32
    carry_bytes = G * eng.n_layers * 2 * STEP_B * eng.P * 4
    LX.memory_guard(G * rows * (dims["d_in"] + 2 * dims["d_out"]) * 4 + 4 * carry_bytes + G * _lib.STATUS_WORDS * 8, f"{G} step groups")
    xs, cin, ys, cout, sts = _step_small(eng, cref.CModel(export), small, dims)
    x, state = LX.repeated(xs, k), LX.repeated(cin, k)
    out = torch.full_like(state, SENTINEL)
    t1 = time.perf_counter()
    y = eng.step(x, state, B=STEP_B, L=STEP_L, groups=G, x_bits=small["x_bits"], x_exp=small["x_exp"], state_out=out)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    LX.assert_repeats(y, ys, "step y")
    LX.assert_repeats(out, cout, "step carry out")
    LX.assert_repeats(state, cin, "step carry in (must be left alone)")
    LX.assert_repeats(eng.lane_status(0, G)[:G * _lib.STATUS_WORDS].view(G, -1), sts.view(R, -1), "step status words")
    _report("step", t0, G=G, y_bytes=G * rows * dims["d_out"] * 4, carry_bytes=carry_bytes, launch_s=f"{t2 - t1:.3f}")
    del y, out

    # ragged, once: entry e keeps its carry in slot perm[e]; rows cycle with the content, so every period is the same work
    t0 = time.perf_counter()
    nrows = np.array([STEP_L, 5, 0, STEP_L, 1, STEP_L, 3])
    pool_s = eng.pool(R, STEP_B)
    pool_s.state.copy_(cin)
    ys_r = pool_s.push_ragged(np.arange(R), FxpArrayOf(xs, small), nrows).data.clone()
    cs_r = pool_s.state.clone()
    g = torch.Generator(device="cpu").manual_seed(7)
    perm = torch.randperm(G, generator=g)
    pool = eng.pool(G, STEP_B)
    pool.state[perm.cuda()] = state
    del state
    t1 = time.perf_counter()
    y = pool.push_ragged(perm.numpy(), FxpArrayOf(x, small), np.tile(nrows, k)).data
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    written = (torch.arange(STEP_L, device="cuda")[None, :] < torch.from_numpy(nrows).cuda()[:, None])[:, None, :, None]   # (R, 1, L, 1)
    yk = y.view(k, R, STEP_B, STEP_L, dims["d_out"])
    for c0 in range(0, k, 1024):
        assert bool(((yk[c0:c0 + 1024] == ys_r[None]) | ~written[None]).all()), f"ragged y, copies from {c0}"
    LX.assert_repeats(pool.state[perm.cuda()], cs_r, "ragged carry")
    _report("step_ragged", t0, n=G, launch_s=f"{t2 - t1:.3f}")
    del x, y, yk, pool, pool_s, eng
    LX.release()


def FxpArrayOf(data, small):
    from sparsernns_amd.fxparray import FxpArray
    return FxpArray(data, small["x_bits"], small["x_exp"], True)
