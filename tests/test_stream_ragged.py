"""Stream sessions that start, stop and idle on their own (include/s5fxp.h s5fxp_push_desc): the ragged step kernel
(csrc/s5fxp_step.hpp k_model_step_ragged), the two ragged audio kernels (csrc/audio_stream.hpp), SessionPool.push_ragged and
audio.SessionDenoiser.

Every comparison is exact (np.array_equal / torch.equal): the step against the C oracle (oracle/cref.py) run per entry on the
CPU and against the lock-step entry (Engine.step, groups = 1) on the GPU, the audio kernels against the batch kernels over the
whole signal, SessionDenoiser against one StreamDenoiser(model, 1) per session fed the same chunks."""
import ctypes as C

import numpy as np
import pytest

import test_audio_kernels as AK
import test_stream_step as SS

gpu = pytest.mark.gpu
HOP = 128
SENT = 0x7ABCDEF          # y's sentinel (int32); as float32 bits a finite number no output equals
NEW_SYMBOLS = ("s5fxp_push_desc_check", "s5fxp_model_step_ragged", "s5fxp_model_step_ragged_f32", "s5fxp_stream_stft_ragged",
               "s5fxp_stream_mask_istft_ragged")


def _desc(rows):
    """rows: (slot, rows, flags[, hops, h4[, reserved0]]) per entry -> a ctypes array of s5fxp_push_desc."""
    from sparsernns_amd import _lib
    arr = (_lib.PushDesc * max(len(rows), 1))()
    for d, r in zip(arr, rows):
        d.slot, d.rows, d.flags = r[0], r[1], r[2]
        if len(r) > 3:
            d.hops, d.h4 = r[3], r[4]
        if len(r) > 5:
            d.reserved[1] = r[5]
    return arr


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_version():
    import os
    from sparsernns_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s5fxp.h")).read()
    assert _lib.lib.s5fxp_version() >= 110
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and name + "(" in header, name
    assert (_lib.PUSH_FRESH, _lib.PUSH_ZEROS, _lib.PUSH_FINAL) == (1, 2, 4) and C.sizeof(_lib.PushDesc) == 32
    for word in ("S5FXP_PUSH_FRESH = 1", "S5FXP_PUSH_ZEROS = 2", "S5FXP_PUSH_FINAL = 4", "s5fxp_push_desc;"):
        assert word in header, word


def test_push_desc_check():
    from sparsernns_amd import _lib
    chk, E, U = _lib.lib.s5fxp_push_desc_check, _lib.S5FXP_EBADARG, _lib.S5FXP_EUNSUPPORTED
    FR, ZE, FI = _lib.PUSH_FRESH, _lib.PUSH_ZEROS, _lib.PUSH_FINAL

    def run(rows, n_slots=6, Lmax=4, cmax=4, audio=0, n=None):
        return chk(_desc(rows), len(rows) if n is None else n, n_slots, Lmax, cmax, audio)

    # the step's fields alone
    assert run([(5, 0, 0), (0, 1, FR), (3, 3, 0), (2, 4, 0)]) == 0
    assert chk(None, 1, 6, 4, 4, 0) == E                       # null array
    assert run([(0, 1, 0)], n=0) == E                          # n < 1
    assert run([(6, 1, 0)]) == E and run([(-1, 1, 0)]) == E    # slot outside 0 .. n_slots-1
    assert run([(1, 1, 0), (2, 1, 0), (1, 0, 0)]) == E         # a slot twice
    assert run([(0, 5, 0)]) == E and run([(0, -1, 0)]) == E    # rows outside 0 .. Lmax
    assert run([(0, 1, 8)]) == E                               # unknown flag bits
    assert run([(0, 1, 0, 0, 0, 1)]) == E                      # nonzero reserved
    # hops / h4 are not looked at without `audio`
    assert run([(0, 1, 0, 77, 9)]) == 0
    # with the audio kernels' fields
    good = [(0, 0, FR, 1, 0), (1, 4, 0, 4, 4), (2, 2, ZE | FI, 2, 4), (3, 1, FR, 2, 0), (4, 3, 0, 3, 2)]
    assert run(good, audio=1) == 0
    assert run([(0, 1, 0, 0, 4)], audio=1) == E and run([(0, 4, 0, 5, 0)], Lmax=5, audio=1) == E   # hops outside 1 .. cmax
    assert run([(0, 1, 0, 1, 4)], cmax=0, audio=1) == E and run([(0, 1, 0, 1, 4)], cmax=33, Lmax=33, audio=1) == E
    assert run([(0, 1, 0, 1, 5)], audio=1) == E and run([(0, 1, 0, 1, -1)], audio=1) == E           # h4 outside 0 .. 4
    assert run([(0, 2, FR, 2, 1)], audio=1) == E                                                    # FRESH with h4 != 0
    assert run([(0, 2, 0, 2, 0)], audio=1) == E and run([(0, 1, 0, 2, 3)], audio=1) == E            # rows != hops - (h4 == 0)
    assert run([(0, 2, ZE | FI, 2, 3)], audio=1) == U and run([(0, 1, FR | FI, 2, 0)], audio=1) == U  # FINAL below 4 hops
    assert run([(0, 2, ZE | FI, 2, 3), (0, 1, 0, 1, 4)], audio=1) == E                              # a bad entry wins
    assert run([(0, 32, 0, 32, 4)], Lmax=32, cmax=32, audio=1) == 0


def test_launch_entries_check_arguments_before_any_device_access():
    """The codes come back for pointers that are not device memory at all: nothing was launched or dereferenced."""
    from sparsernns_amd import _lib
    L, bad, E = _lib.lib, C.c_void_p(64), _lib.S5FXP_EBADARG
    for step in (L.s5fxp_model_step_ragged, L.s5fxp_model_step_ragged_f32):
        # m, x, x_bits, x_exp, n, B, Lmax, y, desc, state, n_slots, status, stream
        assert step(None, bad, 16, 14, 1, 1, 1, bad, bad, bad, 1, bad, None) == E    # null model
        assert step(bad, bad, 16, 14, 1, 1, 1, bad, None, bad, 1, bad, None) == E    # null desc
        assert step(bad, bad, 16, 14, 1, 1, 1, bad, bad, None, 1, bad, None) == E    # null state
        assert step(bad, bad, 16, 14, 1, 1, 1, bad, bad, bad, 0, bad, None) == E     # n_slots < 1
        assert step(bad, bad, 16, 14, 0, 1, 1, bad, bad, bad, 1, bad, None) == E     # n < 1
        assert step(bad, bad, 16, 14, 1, 3, 11, bad, bad, bad, 1, bad, None) == E    # B * Lmax > 32
        assert step(bad, bad, 16, 14, 1, 1, 33, bad, bad, bad, 1, bad, None) == E
    # audio, n, cmax, desc, sub, state, n_slots, x, stream
    f = L.s5fxp_stream_stft_ragged
    assert f(bad, 1, 1, None, 0.0, bad, 1, bad, None) == E and f(bad, 1, 1, bad, 0.0, None, 1, bad, None) == E
    assert f(bad, 0, 1, bad, 0.0, bad, 1, bad, None) == E and f(bad, 1, 1, bad, 0.0, bad, 0, bad, None) == E
    assert f(bad, 1, 0, bad, 0.0, bad, 1, bad, None) == E and f(bad, 1, 33, bad, 0.0, bad, 1, bad, None) == E
    assert f(bad, 1, 1, bad, 0.0, bad, 1, None, None) == E
    # mask, n, cmax, desc, state, n_slots, out, cleaned_mag, stream
    b = L.s5fxp_stream_mask_istft_ragged
    assert b(bad, 1, 1, None, bad, 1, bad, None, None) == E and b(bad, 1, 1, bad, None, 1, bad, None, None) == E
    assert b(bad, 0, 1, bad, bad, 1, bad, None, None) == E and b(bad, 1, 1, bad, bad, 0, bad, None, None) == E
    assert b(bad, 1, 0, bad, bad, 1, bad, None, None) == E and b(bad, 1, 33, bad, bad, 1, bad, None, None) == E
    assert b(bad, 1, 1, bad, bad, 1, None, None, None) == E


# Three staggered sessions of 20 hops each: (first tick, schedule, ticks at which the session has nothing to push).  Session 0
# idles at tick 1 and ends at tick 4 while session 1 pushes; session 2 ends at tick 7 while session 1 pushes.
PLAN = ((0, [14, 1, 5], (1,)), (2, [1] * 20, ()), (5, [4, 16], ()))


def _ticks(plan):
    """-> per tick, the (session, chunk index or None for `finish`) pairs of that tick."""
    todo = [list(range(len(sched))) + [None] for _, sched, _ in plan]
    out, t = [], 0
    while any(todo):
        out.append([(s, todo[s].pop(0)) for s, (t0, _, idle) in enumerate(plan) if todo[s] and t >= t0 and t not in idle])
        t += 1
    return out


def _run_sessions(d, signals, plan, slots, check=True):
    """Drives SessionDenoiser `d`: session s lives in slot slots[s].  -> per session [out, x, mask, cleaned_mag] lists."""
    import torch
    got = [[[] for _ in range(4)] for _ in plan]
    at = [0] * len(plan)
    for tick in _ticks(plan):
        push = [(s, k) for s, k in tick if k is not None]
        fin = [s for s, k in tick if k is None]
        if not push and not fin:
            continue
        counts = [plan[s][1][k] for s, k in push]
        hops = None
        if push:
            cmax = max(counts)
            hops = torch.full((len(push), cmax * HOP), float("nan"), device=signals[0].device)   # the tails are never read
            for e, ((s, _), c) in enumerate(zip(push, counts)):
                hops[e, :c * HOP] = signals[s][at[s] * HOP:(at[s] + c) * HOP]
                at[s] += c
        out, n_out, x, mask, cm, frames = d.push([slots[s] for s, _ in push], hops, counts=counts if push else None,
                                                 finish=[slots[s] for s in fin], check=check, details=True)
        for e, s in enumerate([s for s, _ in push] + fin):
            got[s][0].append(out[e, :int(n_out[e]) * HOP].clone())
            for j, t in enumerate((x, mask, cm)):
                got[s][1 + j].append(t[e, :int(frames[e])].clone())
    return [[torch.cat(p) for p in g] for g in got]


def _run_alone(model, signal, schedule):
    """One StreamDenoiser(model, 1) fed the same chunks -> [out, x, mask, cleaned_mag]."""
    import torch
    from sparsernns_amd import audio
    d, at, parts = audio.StreamDenoiser(model, 1), 0, [[] for _ in range(4)]
    for c in list(schedule) + [None]:
        if c is None:
            r = d.finish(details=True)
        else:
            r = d.push(signal[None, at * HOP:(at + c) * HOP].contiguous(), details=True)
            at += c
        for p, t in zip(parts, r):
            p.append(t[0].clone())
    return [torch.cat(p) for p in parts]


def test_cpu_session_denoiser_equals_one_stream_denoiser_per_session():
    import torch
    from sparsernns_amd import audio
    sig = [torch.from_numpy(AK._audio(1, 20 * HOP, 0.05, seed=70 + s)[0]) for s in range(3)]
    slots = [2, 0, 3]
    d = audio.SessionDenoiser(AK._StubModel(), 4)
    got = _run_sessions(d, sig, PLAN, slots)
    assert list(d.hops) == [22, 0, 22, 22]
    for s, (_, sched, _) in enumerate(PLAN):
        want = _run_alone(AK._StubModel(), sig[s], sched)
        assert tuple(got[s][0].shape) == (20 * HOP,) and tuple(got[s][1].shape) == (21, 257)
        for g, w in zip(got[s], want):
            assert torch.equal(g, w), s


def test_session_denoiser_host_errors():
    import torch
    from sparsernns_amd import audio
    d = audio.SessionDenoiser(AK._StubModel(), 3)
    hop = torch.zeros(1, HOP)
    with pytest.raises(RuntimeError):
        d.finish([0])                                   # nothing was ever pushed
    out, n_out = d.push([0, 2], torch.zeros(2, 4 * HOP), counts=[4, 3])
    assert tuple(out.shape) == (2, 5 * HOP) and list(n_out) == [1, 0] and list(d.hops) == [4, 0, 3]
    with pytest.raises(NotImplementedError):
        d.finish([2])                                   # three hops: below 512 samples
    with pytest.raises(NotImplementedError):
        d.push([0], hop, finish=[2])
    out, n_out = d.push([2], hop, finish=[0])           # slot 0 ends while slot 2 pushes: rows two hops wide
    assert tuple(out.shape) == (2, 3 * HOP) and list(n_out) == [1, 3]
    with pytest.raises(RuntimeError):
        d.push([0], hop)                                # ended: needs start()
    with pytest.raises(RuntimeError):
        d.finish([0])
    d.start([0])
    assert list(d.hops) == [0, 0, 4]
    assert list(d.push([0], hop)[1]) == [0]
    for bad in (dict(ids=[1, 1], hops=torch.zeros(2, HOP)), dict(ids=[1], hops=hop, finish=[1]), dict(ids=[3], hops=hop),
                dict(ids=[1], hops=torch.zeros(1, HOP + 1)), dict(ids=[1], hops=torch.zeros(1, 33 * HOP)),
                dict(ids=[1], hops=torch.zeros(2, HOP)), dict(ids=[1], hops=hop, counts=[2]), dict(ids=[1], hops=hop, counts=[0]),
                dict(ids=[1], hops=hop.double()), dict(ids=[], hops=None)):
        with pytest.raises(ValueError):
            d.push(**bad)
    assert list(d.hops) == [1, 0, 4]                    # a refused push changes nothing


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU: the step kernel
# ---------------------------------------------------------------------------------------------------------------------
def _ragged(eng, x, bits, exp, entries, state, sentinel=True):
    """x: np (n,B,Lmax,d_in) int32 / float32; entries: (slot, rows, flags); state: torch (n_slots,nl,2,B,P), in place.
    -> y np (n,B,Lmax,d_out) (prefilled with SENT), status (n,128)."""
    import torch
    from sparsernns_amd import _lib
    n, B, Lmax = x.shape[:3]
    f32 = x.dtype == np.float32
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    y = torch.full((n, B, Lmax, eng.d_out), SENT, dtype=torch.int32, device="cuda")
    d = np.zeros((n, 8), dtype=np.int32)
    d[:, :3] = entries
    assert _lib.lib.s5fxp_push_desc_check(d.ctypes.data, n, state.shape[0], Lmax, 0, 0) == 0
    dd = torch.from_numpy(d).cuda()
    st = torch.full((n * _lib.STATUS_WORDS,), -1, dtype=torch.int32, device="cuda")
    entry = _lib.lib.s5fxp_model_step_ragged_f32 if f32 else _lib.lib.s5fxp_model_step_ragged
    _lib.check(entry(eng._h, xd.data_ptr(), bits, exp, n, B, Lmax, y.data_ptr(), dd.data_ptr(), state.data_ptr(), state.shape[0],
                     st.data_ptr(), torch.cuda.current_stream().cuda_stream), "ragged step")
    torch.cuda.synchronize()
    return y.cpu().numpy(), st.cpu().numpy().reshape(n, _lib.STATUS_WORDS)


def _fill(eng):
    """The status words of an entry without frames: the kernel's initial fill."""
    w = np.zeros(128, dtype=np.int32)
    w[1], w[2] = eng.out_exp, 3
    for i in range(eng.n_layers):
        w[8 + 8 * i + 5:8 + 8 * i + 8] = (6, eng.P, eng.P)
    return w


def _expect(eng, cm, x, bits, exp, entries, ref_state, lockstep=True):
    """The oracle per entry on ref_state (np, updated in place) -> y (SENT where nothing is written), status (n,128) of the
    lock-step entry with groups = 1 on the same carry (None without `lockstep`)."""
    import torch
    from sparsernns_amd import _lib
    n, B, Lmax = x.shape[:3]
    y = np.full((n, B, Lmax, eng.d_out), SENT, dtype=np.int32)
    sts = []
    for e, (slot, L, flags) in enumerate(entries):
        if flags & _lib.PUSH_FRESH:
            ref_state[slot] = 0
        if L == 0:
            sts.append(_fill(eng))
            continue
        xe = np.ascontiguousarray(x[e][:, :L])
        before = ref_state[slot].copy()
        st = np.ascontiguousarray(ref_state[slot])
        y[e][:, :L] = cm.forward(xe, bits, exp, state=st)[0]
        ref_state[slot] = st
        if lockstep:
            carry = torch.from_numpy(before[None]).cuda()
            yl, stl = SS._step(eng, xe[None], bits, exp, carry, lane=("lockstep", 0))
            assert np.array_equal(yl[0], y[e][:, :L]) and np.array_equal(carry.cpu().numpy()[0], ref_state[slot])
            sts.append(stl[0])
    return y, (np.stack(sts) if lockstep else None)


CASES = {"1x4": (1, 4, [(5, 0), (0, 1), (3, 3), (2, 4)]), "2x16": (2, 16, [(5, 16), (0, 5), (3, 0), (2, 1)])}


@gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("ds", [0.25, 0.5, 1.0])
def test_ragged_step_matches_oracle_and_lockstep_entry(ds, case):
    import torch
    from sparsernns_amd import _lib
    model, qc, dims, cm = SS._synth(ds)
    eng = model.engine()
    B, Lmax, first = CASES[case]
    n_slots, FR = 6, _lib.PUSH_FRESH
    rows = [r for _, r in first]
    pushes = [[(s, r, 0) for s, r in first],                                          # carry: the sentinel below
              [(2, rows[1], 0), (0, rows[3], FR), (4, rows[0], 0), (5, rows[2], 0)],  # slot 0: FRESH over a carry that is not zero
              [(3, rows[3], 0), (0, rows[2], 0), (2, 0, FR), (1, rows[0], 0), (5, rows[1], FR)]]  # slot 2: FRESH without frames
    ref_state = np.full((n_slots, eng.n_layers, 2, B, eng.P), -7, dtype=np.int32)     # unnamed slots keep it
    state = torch.from_numpy(ref_state.copy()).cuda()
    for i, entries in enumerate(pushes):
        n = len(entries)
        x, bits, exp = SS._fx(qc, dims, n, B, Lmax, seed=300 + 10 * i)
        if i == 1:
            assert np.abs(ref_state[0]).max() > 7        # the carry FRESH discards is a real one
        if i == 2:
            assert np.abs(ref_state[2]).max() > 7
        want_y, want_st = _expect(eng, cm, x, bits, exp, entries, ref_state)
        y, st = _ragged(eng, x, bits, exp, entries, state)
        assert np.array_equal(y, want_y), (ds, case, i, int(np.count_nonzero(y != want_y)))   # rows and untouched padding
        assert np.array_equal(state.cpu().numpy(), ref_state), (ds, case, i)                   # named and unnamed slots
        assert np.array_equal(st, want_st), (ds, case, i, np.argwhere(st != want_st)[:8])
    assert not ref_state[2].any() and (ref_state[[0, 1, 3, 4, 5]] != -7).any()


@gpu
def test_padding_frames_cannot_be_seen():
    import torch
    from sparsernns_amd import _lib
    model, qc, dims, cm = SS._synth(0.5)
    eng = model.engine()
    B, Lmax, first = CASES["2x16"]
    entries = [(s, r, 0) for s, r in first]
    x, bits, exp = SS._fx(qc, dims, 4, B, Lmax, seed=410)
    xf = SS.synth.make_input(4 * B, Lmax, dims["d_in"], seed=411).reshape(4, B, Lmax, -1)
    pad = np.zeros((4, 1, Lmax, 1), dtype=bool)
    for e, (_, r, _) in enumerate(entries):
        pad[e, :, r:] = True
    for base, fills in ((x, (2 ** 30,)), (xf, (np.nan, 1e30))):
        b, e_ = (bits, exp) if base.dtype == np.int32 else (qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"])
        runs = []
        for fill in (None,) + fills:
            xi = base.copy() if fill is None else np.where(pad, np.asarray(fill, dtype=base.dtype), base)
            state = torch.full((6, eng.n_layers, 2, B, eng.P), 3, dtype=torch.int32, device="cuda")
            y, st = _ragged(eng, xi, b, e_, entries, state)
            runs.append((y, st, state.cpu().numpy()))
        for y, st, s in runs[1:]:
            assert np.array_equal(y, runs[0][0]) and np.array_equal(st, runs[0][1]) and np.array_equal(s, runs[0][2])
        assert not (runs[0][1][:, 0] & _lib.ST_WIDE_INPUT).any() and (runs[0][0] != SENT).any()


@gpu
@pytest.mark.parametrize("ds", [0.25, 0.5, 1.0])
def test_float_entry_is_from_fp_ragged_step_to_float(ds):
    import torch
    from sparsernns_amd._lib import check, lib
    model, qc, dims, cm = SS._synth(ds)
    eng = model.engine()
    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    B, Lmax, first = CASES["2x16"]
    entries = [(s, r, 0) for s, r in first]
    sa = torch.zeros((6, eng.n_layers, 2, B, eng.P), dtype=torch.int32, device="cuda")
    sb = sa.clone()
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(3):
        xf = SS.synth.make_input(4 * B, Lmax, dims["d_in"], seed=60 + i, scale=(1.0, 6.0, 0.0)[i]).reshape(4, B, Lmax, -1)
        xd = torch.from_numpy(xf).cuda()
        xi = torch.empty(xd.shape, dtype=torch.int32, device="cuda")
        check(lib.s5fxp_from_fp(xd.data_ptr(), xi.data_ptr(), xd.numel(), bits, exp, 0, stream))
        yi, sti = _ragged(eng, xi.cpu().numpy(), bits, exp, entries, sa)
        yd = torch.from_numpy(yi).cuda()
        want = torch.empty(yd.shape, dtype=torch.float32, device="cuda")
        check(lib.s5fxp_to_float(yd.data_ptr(), want.data_ptr(), yd.numel(), eng.out_exp, stream))
        got, stf = _ragged(eng, xf, bits, exp, entries, sb)
        torch.cuda.synchronize()
        valid = yi != SENT
        assert np.array_equal(valid, got != SENT) and valid.any()       # got: the float bits as int32
        assert np.array_equal(got[valid], want.cpu().numpy().view(np.int32)[valid]), (ds, i)
        assert torch.equal(sa, sb) and np.array_equal(sti, stf)
    assert sa.any().item()


@gpu
def test_wide_states_and_wide_input():
    import torch
    from sparsernns_amd import SessionPool, _lib
    from sparsernns_amd.fxparray import FxpArray
    model, qc, dims, cm = SS._synth(0.5)
    eng = model.engine()
    B, Lmax, first = CASES["2x16"]
    entries = [(s, r, 0) for s, r in first]
    n_slots = 6
    x, bits, exp = SS._fx(qc, dims, 4, B, Lmax, seed=520)
    start = np.zeros((n_slots, eng.n_layers, 2, B, eng.P), dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(5))
    start[0] = rng.integers(-2 ** 26, 2 ** 26, start[0].shape, dtype=np.int64).astype(np.int32)   # entry 1's slot
    # (a) a planted 27-bit carry: WIDE_STATE for that entry only, everything exact
    ref_state = start.copy()
    want_y, want_st = _expect(eng, cm, x, bits, exp, entries, ref_state)
    state = torch.from_numpy(start.copy()).cuda()
    y, st = _ragged(eng, x, bits, exp, entries, state)
    assert np.array_equal(y, want_y) and np.array_equal(state.cpu().numpy(), ref_state) and np.array_equal(st, want_st)
    assert [int(w & _lib.ST_WIDE_STATE) for w in st[:, 0]] == [0, _lib.ST_WIDE_STATE, 0, 0]
    # (b) entry 0's input times 6, and -- these inputs peak at 186, so times 6 alone stays within 16 bits -- its first sequence
    # lifted by 40000 as test_stream_step.py does: beyond 16 bits.  Its rows and its slot stay as they were, the others are exact
    xw = x.copy()
    xw[0] *= 6
    xw[0][0] += 40000
    assert np.abs(xw[0]).max() > 32767 and np.abs(xw[1:]).max() <= 32767
    carry5 = rng.integers(-1000, 1000, start[5].shape, dtype=np.int64).astype(np.int32)
    start[5] = carry5
    ref_state = start.copy()
    want_y, _ = _expect(eng, cm, xw, bits, exp, entries, ref_state, lockstep=False)   # the oracle serves entry 0 as well
    state = torch.from_numpy(start.copy()).cuda()
    y, st = _ragged(eng, xw, bits, exp, entries, state)
    assert [int(w & _lib.ST_WIDE_INPUT) for w in st[:, 0]] == [_lib.ST_WIDE_INPUT, 0, 0, 0]
    assert (y[0] == SENT).all() and np.array_equal(state[5].cpu().numpy(), carry5)
    assert np.array_equal(y[1:], want_y[1:])
    got_state = state.cpu().numpy()
    assert np.array_equal(got_state[:5], ref_state[:5])
    w0 = _fill(eng)
    w0[0] = _lib.ST_WIDE_INPUT
    assert np.array_equal(st[0], w0)
    # (c) the pool serves that entry through the generic twin, from the intact carry
    pool = SessionPool(eng, n_slots, B)
    pool.state.copy_(torch.from_numpy(start))
    out = pool.push_ragged([s for s, _, _ in entries], FxpArray(xw, bits, exp), [r for _, r, _ in entries])
    got = out.numpy()
    for e, (_, r, _) in enumerate(entries):
        assert np.array_equal(got[e][:, :r], want_y[e][:, :r]), e
    assert np.array_equal(pool.state.cpu().numpy(), ref_state) and pool.last_path == _lib.PATH_GENERIC
    assert list(pool.frames) == [5, 0, 1, 0, 0, 16]


@gpu
@pytest.mark.parametrize("n", [600, 300, 4])
def test_all_three_workgroup_sizes(n):
    """n = 600 entries: 128 threads; 300: 256; 4: 512 (step_entry's rule on n).  One frame each, slots a permutation."""
    import torch
    model, qc, dims, cm = SS._synth(0.25)
    eng = model.engine()
    perm = np.random.Generator(np.random.PCG64(n)).permutation(n)
    x, bits, exp = SS._scaled_groups(qc, dims, n, 1, 1, seed=77)
    rng = np.random.Generator(np.random.PCG64(9))
    start = rng.integers(-3000, 3000, (n, eng.n_layers, 2, 1, eng.P), dtype=np.int64).astype(np.int32)
    lock = torch.from_numpy(np.ascontiguousarray(start[perm])).cuda()       # group e owns the carry of slot perm[e]
    want_y, want_st = SS._step(eng, x, bits, exp, lock, lane=("lockstep", n))
    state = torch.from_numpy(start.copy()).cuda()
    y, st = _ragged(eng, x, bits, exp, [(int(s), 1, 0) for s in perm], state)
    assert np.array_equal(y, want_y) and np.array_equal(st, want_st)
    assert np.array_equal(state.cpu().numpy()[perm], lock.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU: the audio kernels alone
# ---------------------------------------------------------------------------------------------------------------------
# (slot, first tick, schedule): slot 1 serves a second signal after its first has ended, with FRESH and no clearing launch;
# session 1 ends at tick 3 while sessions 0 and 2 push samples.  Schedules: F = 0, the 16-frame tile boundary, the 32-hop maximum.
RAW = ((0, 0, [1, 1, 1, 1, 3]), (1, 1, [17, 16]), (2, 2, [32, 32, 6]), (1, 5, [4, 3]))
FSENT = 12345.0


def _raw_run(signals, masks, sub, use_mask=True):
    """-> per session [x, out, cleaned_mag] over all its pushes, and the final state tensor (4 slots, slot 3 never named)."""
    import torch
    from sparsernns_amd import _lib
    L = _lib.lib
    n_slots = 4
    state = torch.full((n_slots, L.s5fxp_stream_audio_state_bytes() // 4), FSENT, dtype=torch.float32, device="cuda")
    got = [[[] for _ in range(3)] for _ in RAW]
    at, h = [0] * len(RAW), [0] * len(RAW)
    stream = torch.cuda.current_stream().cuda_stream
    for tick in _ticks([(t0, sched, ()) for _, t0, sched in RAW]):
        n = len(tick)
        cs = [2 if k is None else RAW[s][2][k] for s, k in tick]
        cmax = max(cs)
        audio = torch.full((n, cmax * HOP), float("nan"), device="cuda")
        mask = torch.full((n, cmax, 257), float("nan"), device="cuda")
        d = np.zeros((n, 8), dtype=np.int32)
        meta = []
        for e, ((s, k), c) in enumerate(zip(tick, cs)):
            final = k is None
            F, O = c - (h[s] == 0), min(c, max(0, h[s] + c - 3)) + final
            flags = (_lib.PUSH_FRESH if h[s] == 0 else 0) | ((_lib.PUSH_ZEROS | _lib.PUSH_FINAL) if final else 0)
            d[e, :5] = (RAW[s][0], F, flags, c, min(h[s], 4))
            if not final:   # a finishing entry's audio row stays NaN: ZEROS never reads it
                audio[e, :c * HOP] = signals[s][at[s] * HOP:(at[s] + c) * HOP]
                at[s] += c
            k0 = max(h[s] - 1, 0)
            mask[e, :F] = masks[s][k0:k0 + F]
            meta.append((s, F, O))
            h[s] += c
        assert L.s5fxp_push_desc_check(d.ctypes.data, n, n_slots, cmax, cmax, 1) == 0
        dd = torch.from_numpy(d).cuda()
        x = torch.full((n, cmax, 257), FSENT, device="cuda")
        out = torch.full((n, (cmax + 1) * HOP), FSENT, device="cuda")
        cm = torch.full((n, cmax, 257), FSENT, device="cuda")
        _lib.check(L.s5fxp_stream_stft_ragged(audio.data_ptr(), n, cmax, dd.data_ptr(), sub, state.data_ptr(), n_slots, x.data_ptr(),
                                              stream), "front")
        _lib.check(L.s5fxp_stream_mask_istft_ragged(mask.data_ptr() if use_mask else None, n, cmax, dd.data_ptr(), state.data_ptr(),
                                                    n_slots, out.data_ptr(), cm.data_ptr(), stream), "back")
        torch.cuda.synchronize()
        for e, (s, F, O) in enumerate(meta):
            assert (x[e, F:] == FSENT).all() and (cm[e, F:] == FSENT).all() and (out[e, O * HOP:] == FSENT).all(), (s, F, O)
            for p, t in zip(got[s], (x[e, :F], out[e, :O * HOP], cm[e, :F])):
                p.append(t.clone())
    return [[torch.cat(p) for p in g] for g in got], state


@gpu
def test_ragged_audio_kernels_equal_the_batch_kernels():
    import torch
    from sparsernns_amd import audio
    sig, msk = [], []
    for s, (_, _, sched) in enumerate(RAW):
        T = HOP * sum(sched)
        sig.append(torch.from_numpy(AK._audio(1, T, (1.0, 0.02)[s % 2], seed=80 + s)[0]).cuda())
        msk.append(torch.from_numpy(AK._mask(1, T, seed=90 + s)[0]).cuda())
    got, state = _raw_run(sig, msk, audio.STFT_MAG_MEAN)
    assert (state[3] == FSENT).all() and not (state[:3] == FSENT).all(dim=1).any()
    for s in range(len(RAW)):
        x, out, cm = got[s]
        want_out, want_cm = audio.mask_istft(sig[s][None], msk[s][None], cleaned_mag=True)
        assert torch.equal(x, audio.stft_mag(sig[s][None])[0]), s
        assert torch.equal(out, want_out[0]) and torch.equal(cm, want_cm[0]), s
    # NULL mask = zero mask = the round trip
    null, _ = _raw_run(sig, msk, 0.0, use_mask=False)
    zero, _ = _raw_run(sig, [torch.zeros_like(m) for m in msk], 0.0)
    for s in range(len(RAW)):
        for a, b in zip(null[s], zero[s]):
            assert torch.equal(a, b), s
        assert torch.equal(null[s][1], audio.mask_istft(sig[s][None], None)[0]) and torch.equal(null[s][2], null[s][0])


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU: with the model
# ---------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(dim_scale):
    if dim_scale not in _MODELS:
        _MODELS[dim_scale] = AK._model(dim_scale)[0]
    return _MODELS[dim_scale]


@gpu
@pytest.mark.parametrize("dim_scale", [0.5, 0.25])
def test_session_denoiser_with_the_model(dim_scale):
    import torch
    from sparsernns_amd import audio
    model = _model(dim_scale)
    sig = [(0.02 * torch.randn(20 * HOP, generator=torch.Generator().manual_seed(40 + s))).cuda() for s in range(3)]
    slots = [2, 0, 3]
    d = audio.SessionDenoiser(model, 4)
    got = _run_sessions(d, sig, PLAN, slots)
    for s, (_, sched, _) in enumerate(PLAN):
        want = _run_alone(model, sig[s], sched)
        assert tuple(got[s][0].shape) == (20 * HOP,) and tuple(got[s][1].shape) == (21, 257)
        for g, w in zip(got[s], want):
            assert torch.equal(g, w), (dim_scale, s)
        assert got[s][2].abs().max() > 0
    # start() on every slot: the second run reproduces the first, nothing is cleared in between
    d.start(range(4))
    again = _run_sessions(d, sig, PLAN, slots)
    for a, b in zip(got, again):
        for t, u in zip(a, b):
            assert torch.equal(t, u)


@gpu
def test_no_allocation_in_steady_state():
    import torch
    from sparsernns_amd import audio
    d = audio.SessionDenoiser(_model(0.5), 3)
    hops = (0.02 * torch.randn(2, HOP, generator=torch.Generator().manual_seed(6))).cuda()
    for _ in range(6):   # the first pushes create the buffers (and both pinned descriptor buffers)
        d.push([2, 0], hops)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(20):
        out, n_out = d.push([2, 0], hops)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert tuple(out.shape) == (2, 2 * HOP) and list(n_out) == [1, 1]
