"""What every entry of the C ABI does with the memory the caller owns (include/s5fxp.h: "written completely by the kernel",
"overwritten by the call", "never read"): a result depends on the inputs alone, whatever the workspace, the status words, the
outputs, the trace planes, the padding rows and the unnamed state slots held before the call.

1. Poison fills.  Every byte of those buffers is 0x00 (the control), 0x7F, 0x80 or 0xFF before the call (caller_memory.FILLS);
   what the header makes the caller initialise -- stats and hist zeroed, state_in, the audio state of a running stream -- stays
   as the header says.  Every output the header defines is the reference's -- the C oracle (oracle/cref.py) bit for bit, or the
   float64 / NumPy statement of the float, audio and stage entries at the bound its own test file derives -- and bit for bit the
   same at all four fills, float entries included: no kernel here accumulates floats in a data-dependent order (observers are
   atomic max on bits, histograms integer adds, the score and stage sums fixed-order doubles).
2. Guard bands.  The workspace is a slice of exactly the queried number of bytes on a 256-byte boundary with 64 KiB of sentinel
   either side; status, state_out, trace planes, scores and records likewise with 4 KiB.  Guards intact, outputs right, and at
   least one workspace byte changed (the slice was the one used).
3. Call history.  A loud batch, a quiet one and a quiet shorter one through the same buffers with nothing cleared, against a
   fresh engine that sees the quiet ones only.
4. The harness can fail: a poisoned stats array comes back as the fill, a poisoned state_in changes the output as the oracle says.

Models, inputs and oracle results are those the suite already builds (test_variant_matrix._work, test_clips._synth /
_edge_case, the float references of float_model_ref.py); where an engine caches a buffer the test fills the cached tensor in
place and asserts afterwards that the call used it (data_ptr unchanged).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import float_model_ref as R
import test_audio_kernels as AK
import test_audio_score as AS
import test_clips as TC
import test_float_fq as FQ
import test_float_fq_step as FQS
import test_float_hist as FH
import test_gpu_parity as GP
import test_score_clips as SC
import test_stage_err as ST
import test_stream_ragged as SR
import test_stream_step as SS
import test_variant_matrix as VM
from caller_memory import FILLS, Buffers, FloatBuffers, fill_id, is_fill, poison, poison_at, poisoned, same_bytes, same_results
from oracle import fxp_oracle as O
from sparsernns_amd import synth

gpu = pytest.mark.gpu
fills = pytest.mark.parametrize("fill", FILLS, ids=fill_id)
POISON = 0x7F   # the fill of the cases that run at one fill only
WIDE = ("Bu_re", "Bu_im", "xs_re", "xs_im")   # the trace planes of P columns; the others have H

_CONTROL = {}


def _vs_control(key, fill, got, run_control):
    """``got`` at ``fill`` against the same call at fill 0x00, run once per key and kept."""
    if key not in _CONTROL:
        _CONTROL[key] = got if fill == 0 else run_control()
    same_results(got, _CONTROL[key], str(key))


def _host(t):
    return None if t is None else t.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# 1a. s5fxp_model_forward, _f32, _i16 on the fused path
# ----------------------------------------------------------------------------------------------------------------------
FWD_WORKLOADS = ("A_ragged", "B_frames33x1", "B_frames1x7", "C_grouped", "D_dim10", "F_bnsb", "G_overflow", "H_traced", "I_widesig05")
DS_WORKLOADS = {"S_dim025": 0.25, "S_dim075": 0.75}   # one model each at B = 3, L = 61
SWITCH_CASES = [pytest.param(s, w, id=f"{s}-{w}") for s in VM.SWITCHES for w in FWD_WORKLOADS
                if s != "default" and (s, w) not in VM.NO_EFFECT]


@functools.lru_cache(maxsize=None)
def _ds_work(name):
    model, qc, dims, cm = TC._synth(DS_WORKLOADS[name])
    B, L = 3, 61
    fx = VM._input(qc, dims, B, L, seed=61, scale=1.0)
    ref, rb, re_, rtr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
    tops = [max(int(np.abs(t["xs_re"]).max()), int(np.abs(t["xs_im"]).max())) for t in rtr]
    return dict(qc=qc, dims=dims, export=model.export(), B=B, L=L, G=1, x=fx.data, bits=fx.bits, exp=fx.exp, ref=ref, out=(rb, re_),
                rtr=rtr, tops=tops)


def _work(name):
    return _ds_work(name) if name in DS_WORKLOADS else VM._work(name)


def _flag_sets(name):
    """The four forward flag sets where test_variant_matrix.FLAG_SETS lists the workload (and for the two dim_scale models, whose
    int16 rungs run nowhere else in this file); the default, self-contained forward otherwise."""
    from sparsernns_amd import _lib
    if name in VM.FLAG_SETS or name in DS_WORKLOADS:
        return (_lib.FWD_DEFER_REDO, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, 0, _lib.FWD_EXACT)
    return (0,)


_ENGINES = {}


def _default_engine(name, monkeypatch, generic=False):
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine
    key = (name, generic)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(_work(name)["export"], flags=_lib.MODEL_FORCE_GENERIC) if generic else VM._engine(_work(name), "default", monkeypatch)
    return _ENGINES[key]


def _boundary_x(work, io):
    """The rows of the workload at one of the three model boundaries: the same integers as int32, as the float32 that quantises
    to them (FLOOR of an exact value) or narrowed to int16."""
    import torch
    x = work["x"]
    if io == "float32":
        assert np.abs(x.astype(np.int64)).max() < 2 ** 24
        return torch.from_numpy(np.ldexp(x.astype(np.float32), -work["exp"])).cuda()
    if io == "int16":
        assert np.abs(x.astype(np.int64)).max() < 2 ** 15
        return torch.from_numpy(x.astype(np.int16)).cuda()
    return torch.from_numpy(x).cuda()


def _boundary_y(work, io):
    ref, (rb, re_) = work["ref"], work["out"]
    if io == "float32":
        assert np.abs(ref.astype(np.int64)).max() < 2 ** 24 and 0 <= re_ <= 31
        return np.ldexp(ref.astype(np.float32), -re_)
    if io == "int16":
        assert rb <= 16
        return ref.astype(np.int16)
    return ref


def _forward(eng, work, io, flags, fill, traces=False, lane=0, bands=False):
    """One forward with every buffer it writes poisoned: the lane's workspace and status words (the engine's cached tensors,
    filled in place; with ``bands`` slices of exactly the queried size between guard bands, planted in the engine's cache), y,
    state_out and the trace planes.  -> host copies: y, st (G, 128), sout, tr."""
    import torch
    from sparsernns_amd import _lib
    dtype = getattr(torch, io)
    lane = "bands" if bands else lane   # a lane of its own: the planted slices leave with it
    dims, B, L, G = work["dims"], work["B"], work["L"], work["G"]
    nl, H, P, W = dims["n_layers"], dims["H"], dims["P"], _lib.STATUS_WORDS
    buf = Buffers(fill, bands)
    x = _boundary_x(work, io)
    y = buf((G * B, L, dims["d_out"]), dtype)
    sin = torch.from_numpy(work["state_in"]).cuda() if "state_in" in work else None
    sout = buf(tuple(sin.shape), torch.int32) if sin is not None else None
    tr = [{k: buf((B, L, P if k in WIDE else H), torch.int32) for k in _lib.TRACE_FIELDS} for _ in range(nl)] if traces else None
    need = G * eng._IO[dtype][0](eng._h, B, L)
    if bands:
        eng._wsl[lane] = ((B, L, G, dtype), buf.workspace(need))
        eng._status[lane] = buf((G * W,), torch.int32)
    ws, st = poison(eng.workspace(B, L, lane, G, dtype), fill), poison(eng.lane_status(lane, G), fill)
    assert ws.numel() == need and ws.data_ptr() % 256 == 0
    eng.enqueue(x, work["bits"], work["exp"], y, B, L, traces=tr, flags=flags, lane=lane, state_in=sin, state_out=sout, groups=G)
    torch.cuda.synchronize()
    assert (eng.workspace(B, L, lane, G, dtype).data_ptr(), eng.lane_status(lane, G).data_ptr()) == (ws.data_ptr(), st.data_ptr())
    got = dict(y=_host(y), st=_host(st[:G * W]).reshape(G, W), sout=_host(sout), tr=[{k: _host(v) for k, v in d.items()} for d in tr] if tr else None)
    buf.check(ws)
    if bands:
        del eng._wsl[lane], eng._status[lane]
    if sin is not None:
        assert np.array_equal(_host(sin), work["state_in"]), "state_in is only ever read"
    return got


def _check_forward(name, work, eng, got, io, flags, generic=False):
    """``got`` against the oracle results of the workload.  A deferred forward that reports ST_REDO has no output by contract
    (tests/test_dim_scales.py _check_flags): its y, carry and traces are dropped from ``got``, its status words stay."""
    from sparsernns_amd import _lib
    G, B, L, nl = work["G"], work["B"], work["L"], work["dims"]["n_layers"]
    redo = False
    for g in range(G):
        w = got["st"][g]
        assert w[2] == (_lib.PATH_GENERIC if generic else _lib.PATH_FUSED), (name, g, w[:8])
        assert not (w[0] & (_lib.ST_NEGSHIFT | _lib.ST_NEGEXP | _lib.ST_WIDE_INPUT)), (name, g, w[:8])
        redo |= bool(w[0] & _lib.ST_REDO)
    if name == "G_overflow":   # the workload is there for the gated exact kernels: its states must be seen to leave 16 bits
        assert max(work["tops"]) > 32767 and got["st"][0][0] & _lib.ST_WIDE_STATE, (name, work["tops"], got["st"][0][:8])
    if not (flags & _lib.FWD_DEFER_REDO) or name in VM.FLAG_SETS:
        assert not redo, (name, flags)
    elif flags == _lib.FWD_DEFER_REDO and "tops" in work:
        bounds = [_lib.lib.s5fxp_model_recurrence_xmax(eng._h, i) for i in range(nl)]
        if all(t <= b for t, b in zip(work["tops"], bounds)):
            assert not redo, (name, work["tops"], bounds)
    if redo:
        got.update(y=None, sout=None, tr=None)
        return
    assert same_bytes(got["y"], _boundary_y(work, io)), (name, io, flags, "y")
    for g in range(G):
        w = got["st"][g]
        assert w[1] == 0, (name, g, w[:8])   # the header: only the step and clip kernels store the output exponent
        if G == 1:
            assert [int(w[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in work["rtr"]], (name, flags)
            if not generic:
                assert [int(w[8 + 8 * i + VM._pre_s5_word(work["export"], i)]) for i in range(nl)] == [t["pre_s5_exp"] for t in work["rtr"]], (name, flags)
        else:
            assert [int(w[8 + 8 * i + 4]) for i in range(nl)] == work["res_exps"][g], (name, g)
    if got["sout"] is not None:
        assert np.array_equal(got["sout"], work["state_out"]), (name, "state_out")
    if got["tr"] is not None:
        for i in range(nl):
            for k, ck in VM.TRACE_MAP.items():
                assert np.array_equal(got["tr"][i][k], work["rtr"][i][ck]), (name, i, k)


def _forward_checked(name, eng, io, flags, fill, generic=False, bands=False):
    work = _work(name)
    got = _forward(eng, work, io, flags, fill, traces=name == "H_traced", bands=bands)
    _check_forward(name, work, eng, got, io, flags, generic)
    return got


@gpu
@fills
@pytest.mark.parametrize("name", FWD_WORKLOADS + tuple(DS_WORKLOADS))
def test_fused_forward(name, fill, monkeypatch):
    from sparsernns_amd import _lib
    eng = _default_engine(name, monkeypatch)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    for flags in _flag_sets(name):
        got = _forward_checked(name, eng, "int32", flags, fill)
        _vs_control(("forward", name, "int32", flags), fill, got, lambda: _forward_checked(name, eng, "int32", flags, 0))


@gpu
@fills
@pytest.mark.parametrize("io", ["float32", "int16"])
@pytest.mark.parametrize("name", ["A_ragged", "C_grouped"])
def test_fused_forward_at_the_float32_and_int16_boundaries(name, io, fill, monkeypatch):
    """The header: status words and state_out are bit for bit the int32 entry's, whose control they are compared with."""
    eng = _default_engine(name, monkeypatch)
    for flags in _flag_sets(name):
        got = _forward_checked(name, eng, io, flags, fill)
        _vs_control(("forward", name, io, flags), fill, got, lambda: _forward_checked(name, eng, io, flags, 0))
        key = ("forward", name, "int32", flags)
        if key not in _CONTROL:
            _CONTROL[key] = _forward_checked(name, eng, "int32", flags, 0)
        same_results({k: got[k] for k in ("st", "sout")}, {k: _CONTROL[key][k] for k in ("st", "sout")}, f"{name} {io} against int32")


@gpu
@pytest.mark.parametrize("switch,name", SWITCH_CASES)
def test_fused_forward_under_every_switch(switch, name, monkeypatch):
    """Every experiment switch that can take effect on the workload (test_variant_matrix.NO_EFFECT rules the others out), at
    fill 0x7F against the same engine at fill 0x00: other kernels, other tile walks, other plane distances."""
    eng = VM._engine(_work(name), switch, monkeypatch)
    for flags in _flag_sets(name):
        control = _forward_checked(name, eng, "int32", flags, 0)
        same_results(_forward_checked(name, eng, "int32", flags, POISON), control, f"{switch} {name} {flags}")


# ----------------------------------------------------------------------------------------------------------------------
# 1b. the generic forward (its _f32 and _i16 forms stage xi and yi behind the int workspace) and s5fxp_layer_forward
# ----------------------------------------------------------------------------------------------------------------------
@gpu
@fills
@pytest.mark.parametrize("io", ["int32", "float32", "int16"])
def test_generic_forward(io, fill, monkeypatch):
    from sparsernns_amd import _lib
    eng = _default_engine("A_ragged", monkeypatch, generic=True)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 0
    got = _forward_checked("A_ragged", eng, io, 0, fill, generic=True)
    _vs_control(("generic", io), fill, got, lambda: _forward_checked("A_ragged", eng, io, 0, 0, generic=True))
    if ("generic", "int32") not in _CONTROL:
        _CONTROL[("generic", "int32")] = _forward_checked("A_ragged", eng, "int32", 0, 0, generic=True)
    assert np.array_equal(got["st"], _CONTROL[("generic", "int32")]["st"])


@functools.lru_cache(maxsize=None)
def _layer_case():
    """test_gpu_parity's layer-by-layer case on tiny_bnsb: the oracle's input and output of every layer, and its traces."""
    from oracle import cref
    from sparsernns_amd.fxpmodel import build_regression_model
    cfg, B, L, scale = GP.CASES["tiny_bnsb"]
    md, qc, dims = GP._make(cfg)
    model = build_regression_model(md, qc, dims["n_layers"])
    fx = GP._input(qc, dims, B, L, seed=11, scale=scale)
    inter = {}
    O.RegressionModel(md, qc, dims["n_layers"])(fx, inter)
    fl = O.flatten_intermediates(inter)
    rtr = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp, trace=True)[3]
    hs = [fl["encoder_output_relu"]] + [fl[f"layers_{i}.output"] for i in range(dims["n_layers"])]
    return model.engine(), dims, B, L, hs, rtr


def _layer_forward(i, fill, bands=False, lane=0):
    import torch
    from sparsernns_amd import _lib
    eng, dims, B, L, hs, rtr = _layer_case()
    H, P, W = dims["H"], dims["P"], _lib.STATUS_WORDS
    lane = "bands" if bands else lane
    buf = Buffers(fill, bands)
    h, want = hs[i], hs[i + 1]
    x = torch.from_numpy(np.ascontiguousarray(h.data, dtype=np.int32)).cuda()
    y, e = buf((B, L, H), torch.int32), buf((1,), torch.int32)
    planes = {k: buf((B, L, P if k in WIDE else H), torch.int32) for k in _lib.TRACE_FIELDS}
    tr = (_lib.LayerTrace * 1)()
    for k, t in planes.items():
        setattr(tr[0], k, t.data_ptr())
    need = _lib.lib.s5fxp_workspace_bytes(eng._h, B, L)
    if bands:
        eng._wsl[lane] = ((B, L, 1, torch.int32), buf.workspace(need))
        eng._status[lane] = buf((W,), torch.int32)
    ws, st = poison(eng.workspace(B, L, lane), fill), poison(eng.lane_status(lane), fill)
    assert ws.numel() == need
    _lib.check(_lib.lib.s5fxp_layer_forward(eng._h, i, x.data_ptr(), h.bits, h.exp, B, L, y.data_ptr(), e.data_ptr(), ws.data_ptr(), need,
                                            st.data_ptr(), C.cast(tr, C.POINTER(_lib.LayerTrace)), None, torch.cuda.current_stream().cuda_stream),
               "s5fxp_layer_forward")
    torch.cuda.synchronize()
    assert (eng.workspace(B, L, lane).data_ptr(), eng.lane_status(lane).data_ptr()) == (ws.data_ptr(), st.data_ptr())
    got = dict(y=_host(y), e=_host(e), st=_host(st[:W]), tr={k: _host(t) for k, t in planes.items()})
    buf.check(ws)
    if bands:
        del eng._wsl[lane], eng._status[lane]
    assert np.array_equal(got["y"], want.data) and int(got["e"][0]) == want.exp == int(got["st"][8 + 8 * i + 4]), (i, got["e"], want.exp)
    assert got["st"][2] == _lib.PATH_GENERIC and got["st"][1] == 0 and not (got["st"][0] & (_lib.ST_NEGSHIFT | _lib.ST_NEGEXP)), got["st"][:8]
    for k, ck in GP.TRACE_MAP.items():
        assert np.array_equal(got["tr"][k], rtr[i][ck]), (i, k)
    return got


@gpu
@fills
@pytest.mark.parametrize("layer", [0, 1, 2])
def test_layer_forward(layer, fill):
    _vs_control(("layer", layer), fill, _layer_forward(layer, fill), lambda: _layer_forward(layer, 0))


# ----------------------------------------------------------------------------------------------------------------------
# 1c. s5fxp_model_step, _f32, _ragged, _ragged_f32: G = 3, B = 2, L = 5
# ----------------------------------------------------------------------------------------------------------------------
def _as_float(x, exp):
    return np.ldexp(x.astype(np.float32), -exp)


@functools.lru_cache(maxsize=None)
def _step_case(ds):
    model, qc, dims, cm = TC._synth(ds)
    G, B, L = 3, 2, 5
    x, bits, exp = SS._fx(qc, dims, G, B, L, seed=520)
    rng = np.random.Generator(np.random.PCG64(52))
    state = rng.integers(-3000, 3000, (G, dims["n_layers"], 2, B, dims["P"]), dtype=np.int64).astype(np.int32)
    after = state.copy()
    ref, ye, exps, _ = SS._oracle(cm, x, bits, exp, after)
    return x, bits, exp, state, after, ref, ye, exps


def _step(ds, f32, fill, lane="step"):
    import torch
    from sparsernns_amd import _lib
    model, qc, dims, cm = TC._synth(ds)
    eng, export = model.engine(), model.export()
    x, bits, exp, state, after, ref, ye, exps = _step_case(ds)
    G, B, L = x.shape[:3]
    nl, P, W = eng.n_layers, eng.P, _lib.STATUS_WORDS
    xd = torch.from_numpy(_as_float(x, exp) if f32 else x).cuda()
    y = poisoned((G, B, L, eng.d_out), xd.dtype, fill)
    sin, sout = torch.from_numpy(state).cuda(), poisoned(state.shape, torch.int32, fill)
    st = poison(eng.lane_status(lane, G), fill)
    eng.step(xd, sin, y, B, L, G, bits, exp, state_out=sout, lane=lane)
    torch.cuda.synchronize()
    assert eng.lane_status(lane, G).data_ptr() == st.data_ptr()
    got = dict(y=_host(y), sout=_host(sout), st=_host(st[:G * W]).reshape(G, W))
    assert same_bytes(got["y"], _as_float(ref, ye) if f32 else ref), (ds, f32, "y")
    assert np.array_equal(got["sout"], after) and np.array_equal(_host(sin), state), (ds, f32, "carry")
    for g in range(G):
        w = got["st"][g]
        assert w[2] == _lib.PATH_STEP and w[1] == ye and not (w[0] & (_lib.ST_NEGSHIFT | _lib.ST_NEGEXP | _lib.ST_WIDE_INPUT)), (ds, g, w[:8])
        for i in range(nl):
            assert (w[8 + 8 * i + 5], w[8 + 8 * i + 6], w[8 + 8 * i + 7]) == (6, P, P), (ds, g, i)
            assert w[8 + 8 * i + TC._bn_word(export, i)] == exps[g][i][0] and w[8 + 8 * i + 4] == exps[g][i][1], (ds, g, i)
    return got


@gpu
@fills
@pytest.mark.parametrize("ds", TC.SHAPES)
def test_step(ds, fill):
    for f32 in (False, True):
        _vs_control(("step", ds, f32), fill, _step(ds, f32, fill), lambda: _step(ds, f32, 0))
    a, b = _CONTROL[("step", ds, False)], _CONTROL[("step", ds, True)]
    assert np.array_equal(a["st"], b["st"]) and np.array_equal(a["sout"], b["sout"])


# (slot, rows, flags): slot 3 runs all five frames on its carry, slot 0 has no frames, slot 1 starts FRESH over whatever it
# held; nobody names slot 2
def _ragged_entries():
    from sparsernns_amd import _lib
    return [(3, 5, 0), (0, 0, 0), (1, 3, _lib.PUSH_FRESH)]


@functools.lru_cache(maxsize=None)
def _ragged_case(ds):
    model, qc, dims, cm = TC._synth(ds)
    B, Lmax, n_slots = 2, 5, 4
    entries = _ragged_entries()
    x, bits, exp = SS._fx(qc, dims, len(entries), B, Lmax, seed=530)
    rng = np.random.Generator(np.random.PCG64(53))
    carry = rng.integers(-3000, 3000, (n_slots, dims["n_layers"], 2, B, dims["P"]), dtype=np.int64).astype(np.int32)
    return x, bits, exp, carry


def _ragged(ds, f32, fill):
    """The carries of slots 1 (FRESH) and 2 (unnamed), the frames of x beyond an entry's rows, y and the status words hold the
    fill.  Reference: the oracle per entry; for the status words the lock-step entry at groups = 1 on the same carry, as
    tests/test_stream_ragged.py takes it."""
    import torch
    from sparsernns_amd import _lib
    model, qc, dims, cm = TC._synth(ds)
    eng = model.engine()
    x, bits, exp, carry = _ragged_case(ds)
    entries = _ragged_entries()
    n, B, Lmax = x.shape[:3]
    W = _lib.STATUS_WORDS
    state = torch.from_numpy(carry).cuda()
    poison(state[1], fill), poison(state[2], fill)
    start = _host(state)
    xd = torch.from_numpy(_as_float(x, exp) if f32 else x).cuda()
    y = poisoned((n, B, Lmax, eng.d_out), xd.dtype, fill)
    want_y, want_state, want_st = _host(y), start.copy(), []
    for e, (slot, rows, flags) in enumerate(entries):
        poison_at(xd, (e, slice(None), slice(rows, None)), fill)
        s0 = np.zeros_like(start[slot]) if flags & _lib.PUSH_FRESH else start[slot].copy()
        if rows == 0:
            want_state[slot] = s0
            want_st.append(SR._fill(eng))
            continue
        xe = np.ascontiguousarray(x[e][:, :rows])
        s1 = s0.copy()
        ye, _, yexp, _ = cm.forward(xe, bits, exp, state=s1)
        want_y[e][:, :rows] = _as_float(ye, yexp) if f32 else ye
        want_state[slot] = s1
        want_st.append(SS._step(eng, xe[None], bits, exp, torch.from_numpy(s0[None]).cuda(), lane=("lockstep", 0))[1][0])
    d = np.zeros((n, 8), dtype=np.int32)
    d[:, :3] = entries
    assert _lib.lib.s5fxp_push_desc_check(d.ctypes.data, n, state.shape[0], Lmax, 0, 0) == 0
    dd = torch.from_numpy(d).cuda()
    st = poisoned((n * W,), torch.int32, fill)
    entry = _lib.lib.s5fxp_model_step_ragged_f32 if f32 else _lib.lib.s5fxp_model_step_ragged
    _lib.check(entry(eng._h, xd.data_ptr(), bits, exp, n, B, Lmax, y.data_ptr(), dd.data_ptr(), state.data_ptr(), state.shape[0],
                     st.data_ptr(), torch.cuda.current_stream().cuda_stream), "ragged step")
    torch.cuda.synchronize()
    got = dict(y=_host(y), state=_host(state), st=_host(st).reshape(n, W))
    assert same_bytes(got["y"], want_y), (ds, f32, "y rows, and the fill behind them")
    assert np.array_equal(got["state"], want_state), (ds, f32, "named and unnamed slots")
    assert is_fill(got["state"][2], fill)
    assert np.array_equal(got["st"], np.stack(want_st)), (ds, f32, np.argwhere(got["st"] != np.stack(want_st))[:8])
    got["state"] = got["state"][[0, 1, 3]]   # the unnamed slot keeps the fill, which differs from fill to fill
    got["y"] = [got["y"][e][:, :rows] for e, (_, rows, _) in enumerate(entries)]
    return got


@gpu
@fills
@pytest.mark.parametrize("ds", TC.SHAPES)
def test_ragged_step(ds, fill):
    for f32 in (False, True):
        _vs_control(("ragged", ds, f32), fill, _ragged(ds, f32, fill), lambda: _ragged(ds, f32, 0))


# ----------------------------------------------------------------------------------------------------------------------
# 1d. s5fxp_model_clips, _f32: the tile-edge launch of tests/test_clips.py, Lmax = 100
# ----------------------------------------------------------------------------------------------------------------------
def _clips_launch(eng, x, lens, bits, exp, states, fill, lane="clips", bands=False, keep=False):
    """x (n, Lmax, d_in) host, int32 or float32, rows beyond a clip's length poisoned here; states (n, nl, 2, P) or None.
    ``keep``: the call history tests -- nothing is filled, y and the carry out are the lane's tensors of the call before."""
    import torch
    from sparsernns_amd import _lib
    n, Lmax, W = x.shape[0], x.shape[1], _lib.STATUS_WORDS
    lane = "bands" if bands else lane
    buf = Buffers(fill, bands)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for e, L in enumerate(lens):
        if not keep:
            poison_at(xd, (e, slice(L, None)), fill)
    need = _lib.lib.s5fxp_clips_workspace_bytes(eng._h, n, Lmax)
    if keep:
        y, sout = keep
    else:
        y, sout = buf((n, Lmax, eng.d_out), xd.dtype), buf((n, eng.n_layers, 2, eng.P), torch.int32)
    if bands:
        eng._wsl[("clips", lane)] = ((n, Lmax), buf.workspace(need))
        eng._status[lane] = buf((n * W,), torch.int32)
    ws, st = eng._clips_workspace(n, Lmax, lane), eng.lane_status(lane, n)
    if not keep:
        poison(ws, fill), poison(st, fill)
    assert ws.numel() == need
    sin = torch.from_numpy(np.ascontiguousarray(states)).cuda() if states is not None else None
    eng.clips(xd, torch.tensor(list(lens), dtype=torch.int32, device="cuda"), y, sin, sout, bits, exp, lane=lane)
    torch.cuda.synchronize()
    assert (eng._clips_workspace(n, Lmax, lane).data_ptr(), eng.lane_status(lane, n).data_ptr()) == (ws.data_ptr(), st.data_ptr())
    got = dict(y=_host(y), sout=_host(sout), st=_host(st[:n * W]).reshape(n, W))
    buf.check(ws)
    if bands:
        del eng._wsl[("clips", lane)], eng._status[lane]
    return got


def _check_clips(eng, export, got, clips, states, refs, f32, fill, tag):
    """test_clips._check with the fill where it has its sentinel: rows from len_e on keep every byte they had."""
    from sparsernns_amd import _lib
    nl, P = eng.n_layers, eng.P
    for e, clip in enumerate(clips):
        L, w = len(clip), got["st"][e]
        assert w[2] == _lib.PATH_CLIP and w[1] == eng.out_exp, (tag, e, w[:8])
        if fill is not None:
            assert is_fill(got["y"][e, L:], fill), (tag, e, "rows beyond len were written")
        for i in range(nl):
            assert (w[8 + 8 * i + 5], w[8 + 8 * i + 6], w[8 + 8 * i + 7]) == (6, P, P), (tag, e, i)
        sin = np.zeros((nl, 2, P), dtype=np.int32) if states is None else states[e]
        if L == 0:
            assert w[0] == 0 and not any(w[8 + 8 * i + j] for i in range(nl) for j in range(5)), (tag, e, w[:32])
            assert np.array_equal(got["sout"][e], sin), (tag, e, "carry of an empty clip")
            continue
        ref, ye, exps, sref, _ = refs[e]
        assert not (w[0] & (_lib.ST_NEGSHIFT | _lib.ST_NEGEXP | _lib.ST_WIDE_INPUT)) and w[1] == ye, (tag, e, w[:8])
        assert same_bytes(got["y"][e, :L], _as_float(ref, ye) if f32 else ref), (tag, e, L)
        assert np.array_equal(got["sout"][e], sref), (tag, e, L, "carry")
        for i in range(nl):
            assert w[8 + 8 * i + TC._bn_word(export, i)] == exps[i][0] and w[8 + 8 * i + 4] == exps[i][1], (tag, e, i)


def _clips(ds, f32, fill, bands=False):
    model, qc, dims, cm = TC._synth(ds)
    eng = model.engine()
    clips, bits, exp, states, refs = TC._edge_case(ds)
    x = TC._pad(clips, 100)
    got = _clips_launch(eng, _as_float(x, exp) if f32 else x, TC.EDGE_LENS, bits, exp, states, fill, bands=bands)
    _check_clips(eng, model.export(), got, clips, states, refs, f32, fill, (ds, f32, fill))
    got["y"] = [got["y"][e, :L] for e, L in enumerate(TC.EDGE_LENS)]   # behind them: the fill
    return got


@gpu
@fills
@pytest.mark.parametrize("ds", TC.SHAPES)
def test_clips(ds, fill):
    """The workspace of the empty clip is poisoned like the rest; with 0xFF the float entry's padding rows are NaN."""
    for f32 in (False, True):
        _vs_control(("clips", ds, f32), fill, _clips(ds, f32, fill), lambda: _clips(ds, f32, 0))
    a, b = _CONTROL[("clips", ds, False)], _CONTROL[("clips", ds, True)]
    assert np.array_equal(a["st"], b["st"]) and np.array_equal(a["sout"], b["sout"])


# ----------------------------------------------------------------------------------------------------------------------
# 1e. the float model: forward, _hist, _fq (all sites on; recurrence="step"), _clips, _clips_fq
# ----------------------------------------------------------------------------------------------------------------------
FLOAT_CASE = (3, 61, 12)   # (B, L, seed)
RECIPE = "w8a16"           # synth.make_model(dim): the model of tests/test_float_model.py, under test_float_fq's cached engine
FLOAT_DIMS = (0.25, 0.5, 0.75, 1.0)
FQ_DIMS = (0.25, 1.0)      # the two ends, as tests/test_float_fq_step.py's MODEL_GRID


def _no_nan(stats, hist, what):
    """With fill 0xFF every poisoned float is a NaN: none may reach an observer or bin 63 of a histogram (the inputs here put
    no value at or above 2^23 into any tensor)."""
    assert not np.isnan(stats).any(), what
    if hist is not None:
        assert not hist[:, 63].any(), (what, np.nonzero(hist[:, 63]))


def _check_hist(t, dims, N):
    """test_float_hist.check_rows_equal_planes on planes of our own: every row is exp_hist of the device's plane."""
    from sparsernns_amd import floatmodel
    keys = floatmodel.stat_keys(dims["n_layers"])
    hist = dict(zip(keys, t["hist"]))
    want = FH.device_planes(t, dims["n_layers"])
    assert set(hist) == set(want) | {"encoder.out"}
    for k, plane in want.items():
        assert np.array_equal(hist[k], floatmodel.exp_hist(plane)), k
    counts = FH.element_counts(dims, N)
    assert [int(hist[k].sum()) for k in keys] == [counts[k] for k in keys]


def _float_forward(dim, fill):
    """All four (trace, hist) forms.  The traced form with the histogram is held to float_model_ref's stage bounds, the observers'
    absmax rule and the histogram rule; the other three must equal it bit for bit, as the header says of each."""
    import torch
    md, _, dims = FQ.model(dim, RECIPE)
    eng = FQ.engine(dim, RECIPE)
    B, L = FLOAT_CASE[:2]
    x = FQ.make_x(dims, FLOAT_CASE, RECIPE)
    xd = torch.from_numpy(x).cuda()
    b = FloatBuffers(eng, B, L, fill, trace=True, hist=True)
    b.call(xd)
    t = b.planes(x)
    R.check_stages(md, dims["n_layers"], x, t)
    R.check_observers(md, dims["n_layers"], x, t)
    _check_hist(t, dims, B * L)
    _no_nan(t["stats"], t["hist"], (dim, fill))
    assert not np.isnan(t["out"]).any()
    for trace, hist in ((True, False), (False, True), (False, False)):
        o = FloatBuffers(eng, B, L, fill, trace=trace, hist=hist)
        o.call(xd)
        if trace:
            t2 = o.planes(x)
            same_results({k: v for k, v in t.items() if k != "hist"}, t2, f"traced without hist, dim {dim}")
        r = o.result()
        assert same_bytes(r["y"], t["out"]) and same_bytes(r["stats"], t["stats"]), (dim, trace, hist)
        assert r["hist"] is None or np.array_equal(r["hist"], t["hist"]), (dim, trace, hist)
    del t["x"]
    return t


@gpu
@fills
@pytest.mark.parametrize("dim", FLOAT_DIMS)
def test_float_forward_and_hist(dim, fill):
    _vs_control(("float", dim), fill, _float_forward(dim, fill), lambda: _float_forward(dim, 0))


@functools.lru_cache(maxsize=None)
def _fq_spec(dim, mode):
    """None, every site on ("scan"), or every site on with the state sites stepping ("step")."""
    from sparsernns_amd import floatmodel as F
    if mode is None or mode == "scan":
        return FQ.full_spec(dim, RECIPE) if mode else None
    _, qc, dims = FQ.model(dim, RECIPE)
    return F.fq_spec(qc, dims["n_layers"], recurrence="step")


def _float_fq(dim, mode, fill):
    import torch
    dims = FQ.model(dim, RECIPE)[2]
    eng = FQ.engine(dim, RECIPE)
    B, L = FLOAT_CASE[:2]
    x = FQ.make_x(dims, FLOAT_CASE, RECIPE)
    xd = torch.from_numpy(x).cuda()
    spec = _fq_spec(dim, mode)
    b = FloatBuffers(eng, B, L, fill, trace=True)
    b.call(xd, fq=spec)
    t = b.planes(x)
    if mode == "scan":
        FQ.check_all_sites_on(dim, FLOAT_CASE, RECIPE, t=t)
    else:
        FQS.check_all_sites_on_in_step_mode(dim, FLOAT_CASE, RECIPE, t=t)
    _no_nan(t["stats"], None, (dim, mode, fill))
    o = FloatBuffers(eng, B, L, fill, trace=False)
    o.call(xd, fq=spec)
    r = o.result()
    assert same_bytes(r["y"], t["out"]) and same_bytes(r["stats"], t["stats"]), (dim, mode)
    del t["x"]
    return t


@gpu
@fills
@pytest.mark.parametrize("mode", ["scan", "step"])
@pytest.mark.parametrize("dim", FQ_DIMS)
def test_float_forward_fq(dim, mode, fill):
    _vs_control(("float fq", dim, mode), fill, _float_fq(dim, mode, fill), lambda: _float_fq(dim, mode, 0))


@functools.lru_cache(maxsize=None)
def _float_clip_refs(dim, fq):
    """Per clip of the EDGE_LENS launch what the rectangular forward gives it alone (tests/test_float_clips.py's reference),
    through FloatEngine's own buffers: (y, stats bits, hist) or None for the empty clip.  ``fq``: None, "scan", "step"."""
    import torch
    _, _, dims = FQ.model(dim, RECIPE)
    eng = FQ.engine(dim, RECIPE)
    x = synth.make_input(len(TC.EDGE_LENS), 100, dims["d_in"], seed=77)
    xd = torch.from_numpy(x).cuda()
    spec = _fq_spec(dim, fq)
    per = []
    for e, n in enumerate(TC.EDGE_LENS):
        if not n:
            per.append(None)
            continue
        se, he = eng.new_stats(), None if fq else eng.new_hist()
        ye = eng.forward_device(xd[e:e + 1, :n].contiguous(), se, hist_dev=he, fq=spec)
        per.append((_host(ye[0]), _host(se).view(np.uint32), _host(he)))
    return x, per


def _float_clips(dim, fq, fill, bands=False):
    import torch
    eng = FQ.engine(dim, RECIPE)
    x, per = _float_clip_refs(dim, fq)
    n, Lmax = x.shape[:2]
    xd = torch.from_numpy(x).cuda()
    for e, L in enumerate(TC.EDGE_LENS):
        poison_at(xd, (e, slice(L, None)), fill)   # NaN rows at 0xFF
    lens = torch.tensor(TC.EDGE_LENS, dtype=torch.int32, device="cuda")
    spec = _fq_spec(dim, fq)
    live = [p for p in per if p is not None]
    out = {}
    for hist in ((False,) if fq else (True, False)):
        b = FloatBuffers(eng, n, Lmax, fill, trace=False, hist=hist)
        buf = _band_float(b, fill) if bands else Buffers(fill)
        b.call(xd, lens=lens, fq=spec)
        r = b.result()
        buf.check(b.ws)
        for e, (L, p) in enumerate(zip(TC.EDGE_LENS, per)):
            assert is_fill(r["y"][e, L:], fill), (dim, e, "rows beyond len were written")
            assert p is None or same_bytes(r["y"][e, :L], p[0]), (dim, fq, e, L)
        assert np.array_equal(r["stats"].view(np.uint32), np.maximum.reduce([p[1] for p in live])), (dim, fq, "observers")
        if hist:
            assert np.array_equal(r["hist"], sum(p[2] for p in live)), (dim, "histograms")
        _no_nan(r["stats"], r["hist"], (dim, fq, fill))
        out[hist] = dict(y=[r["y"][e, :L] for e, L in enumerate(TC.EDGE_LENS)], stats=r["stats"], hist=r["hist"])
    if not fq:
        assert same_bytes(out[True]["stats"], out[False]["stats"]) and all(same_bytes(a, c) for a, c in zip(out[True]["y"], out[False]["y"]))
    return out


def _band_float(b, fill):
    """Moves every buffer of a FloatBuffers between guard bands, the workspace a slice of exactly the queried size; returns the
    Buffers whose ``check`` holds them."""
    import torch
    buf = Buffers(fill, bands=True)
    b.ws = buf.workspace(b.need).view(torch.float32)
    del b.cached
    b.y = buf.like(b.y)
    if b.tr is not None:
        b.tr = buf.like(b.tr)
    if b.stats is not None:
        b.stats = buf.like(b.stats).zero_()
    if b.hist is not None:
        b.hist = buf.like(b.hist).zero_()
    return buf


@gpu
@fills
@pytest.mark.parametrize("dim", FLOAT_DIMS)
def test_float_clips(dim, fill):
    _vs_control(("float clips", dim), fill, _float_clips(dim, None, fill), lambda: _float_clips(dim, None, 0))


@gpu
@fills
@pytest.mark.parametrize("mode", ["scan", "step"])
@pytest.mark.parametrize("dim", FQ_DIMS)
def test_float_clips_fq(dim, mode, fill):
    _vs_control(("float clips fq", dim, mode), fill, _float_clips(dim, mode, fill), lambda: _float_clips(dim, mode, 0))


# ----------------------------------------------------------------------------------------------------------------------
# 1f. audio: the scored inverse, its clips form, the stream kernels from hops_before == 0 and their ragged forms
# ----------------------------------------------------------------------------------------------------------------------
SCORE_CASES = [(1, 512), (3, 1700)]   # one tile with both cover edges; a second tile of one hop, three sequences


def _score(case, lam, fill, mask, mask_exp=None, bands=False):
    """s5fxp_mask_istft_score[_i16] with the workspace, the three scores and both planes poisoned -> host copies."""
    import torch
    from sparsernns_amd import _lib
    B, T = case
    nd, cd, md, out_ref, cm_ref, _ = AS.device_case(B, T)
    wb = _lib.lib.s5fxp_score_workspace_bytes(B, T)
    buf = Buffers(fill, bands)
    ws, scores = buf.workspace(wb), buf((3, B), torch.float32)
    out, cm = buf(tuple(out_ref.shape), torch.float32), buf(tuple(cm_ref.shape), torch.float32)
    tail = (B, T, lam, out.data_ptr(), cm.data_ptr(), ws.data_ptr(), wb, scores[1].data_ptr(), scores[2].data_ptr(), scores[0].data_ptr(),
            torch.cuda.current_stream().cuda_stream)
    if mask_exp is None:
        _lib.check(_lib.lib.s5fxp_mask_istft_score(nd.data_ptr(), cd.data_ptr(), mask.data_ptr(), *tail), "s5fxp_mask_istft_score")
    else:
        _lib.check(_lib.lib.s5fxp_mask_istft_score_i16(nd.data_ptr(), cd.data_ptr(), mask.data_ptr(), mask_exp, *tail), "s5fxp_mask_istft_score_i16")
    torch.cuda.synchronize()
    buf.check(ws)
    return dict(loss=_host(scores[0]), si=_host(scores[1]), mse=_host(scores[2]), out=_host(out), cm=_host(cm))


def _check_score(case, lam, got):
    """tests/test_audio_score.py's float64 statement on the unchanged entries' planes, at that file's bounds."""
    _, _, _, out_ref, cm_ref, planes = AS.device_case(*case)
    ls, si, mse = AS.ref_scores(*planes, lam)
    assert np.all(np.abs(si) <= 40.0), si
    assert np.abs(got["si"].astype(np.float64) - si).max() <= 1e-4
    assert (np.abs(got["mse"].astype(np.float64) - mse) / mse).max() <= 1e-6
    again = np.float64(lam) * got["mse"].astype(np.float64) + (100.0 - got["si"].astype(np.float64))
    assert np.abs(got["loss"].astype(np.float64) - again).max() <= 1e-5
    assert same_bytes(got["out"], out_ref) and same_bytes(got["cm"], cm_ref)


def _score_all(case, fill):
    import torch
    md = AS.device_case(*case)[2]
    mi = torch.round(md * 2.0 ** 14).to(torch.int16)
    mf = mi.to(torch.float32) / 2.0 ** 14
    out = {}
    for lam in AS.LAMS:
        out[lam] = _score(case, lam, fill, md)
        _check_score(case, lam, out[lam])
    # the int16 mask at exponent 14 = the float entry on to_float(mask), bit for bit (test_audio_score.test_int16_mask)
    out["i16"] = _score(case, 0.001, fill, mi, mask_exp=14)
    same_results(out["i16"], _score(case, 0.001, fill, mf), "int16 mask against the float entry")
    return out


@gpu
@fills
@pytest.mark.parametrize("case", SCORE_CASES, ids=AS._ids)
def test_score(case, fill):
    _vs_control(("score", case), fill, _score_all(case, fill), lambda: _score_all(case, 0))


SCORE_CLIPS = ((5000, 777, 100, 1664), 5000)   # four tiles, one tile, no frames (T < 512), exactly one tile; Tmax allows four


def _score_clips(lam, fill, bands=False):
    """The audio, the clean audio and the mask behind each clip, the workspace (tiles nobody writes included), the scores and
    both planes hold the fill.  Reference: tests/test_score_clips.py's -- the batch entry on each clip alone, bit for bit."""
    import torch
    from sparsernns_amd import _lib
    Ts, Tmax = SCORE_CLIPS
    nz0, cl0, mk0, s, ref, out_ref, cm_ref = SC._device_case(Ts, Tmax)
    nz, cl, mk = nz0.clone(), cl0.clone(), mk0.clone()
    n, Lmax = len(Ts), SC._frames(Tmax)
    lens = [SC._frames(SC._clamp(T, Tmax)) for T in Ts]
    # (n, Tmax) rows: the samples behind a clip, byte for byte
    for t in (nz, cl):
        v = t.view(torch.uint8).view(n, Tmax, 4)
        for e, T in enumerate(Ts):
            v[e, SC._clamp(T, Tmax):] = fill
    for e, L in enumerate(lens):
        poison_at(mk, (e, slice(L, None)), fill)
    wb = _lib.lib.s5fxp_score_clips_workspace_bytes(n, Tmax)
    assert wb == 48 * n * -(-(Lmax - 1) // 13)
    buf = Buffers(fill, bands)
    ws, scores = buf.workspace(wb), buf((3, n), torch.float32)
    out, cm = buf((n, (Lmax - 1) * 128), torch.float32), buf((n, Lmax, 257), torch.float32)
    _lib.check(_lib.lib.s5fxp_mask_istft_score_clips(nz.data_ptr(), cl.data_ptr(), mk.data_ptr(), n, Tmax, s.data_ptr(), lam, out.data_ptr(),
                                                     cm.data_ptr(), ws.data_ptr(), wb, scores[1].data_ptr(), scores[2].data_ptr(),
                                                     scores[0].data_ptr(), torch.cuda.current_stream().cuda_stream), "s5fxp_mask_istft_score_clips")
    torch.cuda.synchronize()
    buf.check(ws)
    SC._check_scores((scores[0], scores[1], scores[2]), ref[lam], Ts, ("poisoned", fill))
    got = dict(scores=_host(scores), out=[], cm=[])
    for e, L in enumerate(lens):
        hops = max(L - 1, 0) * 128
        assert is_fill(out[e, hops:], fill) and is_fill(cm[e, L:], fill), (e, "the planes were written behind the clip")
        assert torch.equal(out[e, :hops], out_ref[e, :hops]) and torch.equal(cm[e, :L], cm_ref[e, :L]), e
        got["out"].append(_host(out[e, :hops]))
        got["cm"].append(_host(cm[e, :L]))
    return got


@gpu
@fills
def test_score_clips(fill):
    for lam in AS.LAMS:
        _vs_control(("score clips", lam), fill, _score_clips(lam, fill), lambda: _score_clips(lam, 0))


HOP = 128
STREAM_PUSHES = (17, 16)   # hops per push: F = 16 frames each, the 16-frame tile boundary of tests/test_stream_ragged.py


@functools.lru_cache(maxsize=None)
def _stream_signals():
    """Two signals of 33 hops, their masks, and the batch kernels' planes of the whole signals (the reference)."""
    import torch
    from sparsernns_amd import audio
    T = HOP * sum(STREAM_PUSHES)
    sig = torch.from_numpy(np.concatenate([AK._audio(1, T, amp, seed=80 + s) for s, amp in enumerate((1.0, 0.02))])).cuda()
    msk = torch.from_numpy(np.concatenate([AK._mask(1, T, seed=90 + s) for s in range(2)])).cuda()
    out, cm = audio.mask_istft(sig, msk, cleaned_mag=True)
    return sig, msk, audio.stft_mag(sig), out, cm


def _stream_lockstep(fill, streams=(0, 1), pushes=3):
    """s5fxp_stream_stft and s5fxp_stream_mask_istft from hops_before == 0.  The header makes the caller zero a fresh stream's
    state, so the state starts as zeros and is carried; x, out and cleaned_mag of every push hold the fill.
    -> (host copies of x, out and cleaned_mag over the pushes, the state tensor after them)."""
    import torch
    from sparsernns_amd import _lib, audio
    L = _lib.lib
    sig, msk, x_ref, out_ref, cm_ref = (t[list(streams)] for t in _stream_signals())
    S = len(streams)
    state = torch.zeros(S, L.s5fxp_stream_audio_state_bytes() // 4, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    xs, outs, cms, h = [], [], [], 0
    for c, final in [(c, 0) for c in STREAM_PUSHES][:pushes] + ([(2, 1)] if pushes > len(STREAM_PUSHES) else []):
        F, Ohops = L.s5fxp_stream_frames(h, c), L.s5fxp_stream_out_hops(h, c, final)
        k0 = max(h - 1, 0)
        a = None if final else sig[:, h * HOP:(h + c) * HOP].contiguous()
        m = msk[:, k0:k0 + F].contiguous()
        x, cm = poisoned((S, F, 257), torch.float32, fill), poisoned((S, F, 257), torch.float32, fill)
        out = poisoned((S, Ohops * HOP), torch.float32, fill)
        _lib.check(L.s5fxp_stream_stft(a.data_ptr() if a is not None else None, S, c, h, audio.STFT_MAG_MEAN, state.data_ptr(), x.data_ptr(),
                                       stream), "s5fxp_stream_stft")
        _lib.check(L.s5fxp_stream_mask_istft(m.data_ptr(), S, c, h, final, state.data_ptr(), out.data_ptr(), cm.data_ptr(), stream),
                   "s5fxp_stream_mask_istft")
        torch.cuda.synchronize()
        xs.append(x), outs.append(out), cms.append(cm)
        h += c
    x, out, cm = torch.cat(xs, dim=1), torch.cat(outs, dim=1), torch.cat(cms, dim=1)
    nf, nh = x.shape[1], out.shape[1]
    assert torch.equal(x, x_ref[:, :nf]) and torch.equal(cm, cm_ref[:, :nf]) and torch.equal(out, out_ref[:, :nh]), fill
    return dict(x=_host(x), out=_host(out), cm=_host(cm)), state


@gpu
@fills
def test_stream_kernels_from_the_first_hop(fill):
    got, _ = _stream_lockstep(fill)
    assert got["x"].shape[1] == sum(STREAM_PUSHES) + 1 and got["out"].shape[1] == HOP * sum(STREAM_PUSHES)   # the whole signal
    _vs_control("stream", fill, got, lambda: _stream_lockstep(0)[0])


def _stream_ragged(fill):
    """One ragged push: entry 0 starts signal 1 FRESH in slot 2, whose state holds the fill; entry 1 continues signal 0 in slot 0
    with its second push; nobody names slot 1, which holds the fill.  The audio and mask rows behind an entry's hops and frames,
    x, out and cleaned_mag hold the fill.  Reference: the batch kernels' planes of the whole signals."""
    import torch
    from sparsernns_amd import _lib, audio
    L = _lib.lib
    sig, msk, x_ref, out_ref, cm_ref = _stream_signals()
    c0, c1 = STREAM_PUSHES
    _, first = _stream_lockstep(0, streams=(0,), pushes=1)   # signal 0 after its first push
    n_slots, n, cmax = 3, 2, max(STREAM_PUSHES)
    state = poisoned((n_slots, first.shape[1]), torch.float32, fill)
    state[0] = first[0]
    d = np.zeros((n, 8), dtype=np.int32)
    d[0, :5] = (2, c0 - 1, _lib.PUSH_FRESH, c0, 0)
    d[1, :5] = (0, c1, 0, c1, 4)
    assert L.s5fxp_push_desc_check(d.ctypes.data, n, n_slots, cmax, cmax, 1) == 0
    dd = torch.from_numpy(d).cuda()
    a, m = poisoned((n, cmax * HOP), torch.float32, fill), poisoned((n, cmax, 257), torch.float32, fill)
    a[0, :c0 * HOP], a[1, :c1 * HOP] = sig[1, :c0 * HOP], sig[0, c0 * HOP:(c0 + c1) * HOP]
    m[0, :c0 - 1], m[1, :c1] = msk[1, :c0 - 1], msk[0, c0 - 1:c0 - 1 + c1]
    x, cm = poisoned((n, cmax, 257), torch.float32, fill), poisoned((n, cmax, 257), torch.float32, fill)
    out = poisoned((n, (cmax + 1) * HOP), torch.float32, fill)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.s5fxp_stream_stft_ragged(a.data_ptr(), n, cmax, dd.data_ptr(), audio.STFT_MAG_MEAN, state.data_ptr(), n_slots, x.data_ptr(), stream),
               "s5fxp_stream_stft_ragged")
    _lib.check(L.s5fxp_stream_mask_istft_ragged(m.data_ptr(), n, cmax, dd.data_ptr(), state.data_ptr(), n_slots, out.data_ptr(), cm.data_ptr(), stream),
               "s5fxp_stream_mask_istft_ragged")
    torch.cuda.synchronize()
    assert is_fill(state[1], fill), "a slot nobody names was touched"
    # (signal, first frame, frames, first output hop, output hops) of the two entries
    O0, O1 = int(L.s5fxp_stream_out_hops(0, c0, 0)), int(L.s5fxp_stream_out_hops(c0, c1, 0))
    parts = [(1, 0, c0 - 1, 0, O0), (0, c0 - 1, c1, O0, O1)]
    # what a push of c hops leaves of a slot's state: its newest c + 3 hops and the three segments; the older hops keep their
    # bytes (the fill in slot 2) and are never read before a longer push has rewritten them
    floats = first.shape[1]
    got = dict(state=[_host(state[slot, (32 - c) * HOP:]) for slot, c in ((2, c0), (0, c1))], x=[], out=[], cm=[])
    assert floats == 35 * HOP + 3 * 512 and is_fill(state[2, :(32 - c0) * HOP], fill)
    for e, (s, k0, F, o0, Oh) in enumerate(parts):
        assert is_fill(x[e, F:], fill) and is_fill(cm[e, F:], fill) and is_fill(out[e, Oh * HOP:], fill), (e, "written behind the entry")
        assert torch.equal(x[e, :F], x_ref[s, k0:k0 + F]) and torch.equal(cm[e, :F], cm_ref[s, k0:k0 + F]), e
        assert torch.equal(out[e, :Oh * HOP], out_ref[s, o0 * HOP:(o0 + Oh) * HOP]), e
        got["x"].append(_host(x[e, :F])), got["cm"].append(_host(cm[e, :F])), got["out"].append(_host(out[e, :Oh * HOP]))
    return got


@gpu
@fills
def test_ragged_stream_kernels_with_a_fresh_entry(fill):
    _vs_control("stream ragged", fill, _stream_ragged(fill), lambda: _stream_ragged(0))


# ----------------------------------------------------------------------------------------------------------------------
# 1g. s5fxp_stage_err
# ----------------------------------------------------------------------------------------------------------------------
STAGE_PAIRS = ("1x1x48 exp0", "2x70x96 exp15 relu", "1x3x1367 f32")   # the smallest pair, a box with the ReLU, two workgroups


@functools.lru_cache(maxsize=None)
def _stage_pairs():
    import torch
    from sparsernns_amd import verify
    cases = ST._cases()
    pairs = [verify.pair(view(torch.from_numpy(a).cuda()), view(torch.from_numpy(b).cuda()), a_exp, relu)
             for a, b, a_exp, relu, view in (cases[k] for k in STAGE_PAIRS)]
    return pairs, verify.stage_errors_host(pairs)


def _stage_err(fill, bands=False):
    import torch
    from sparsernns_amd import verify
    pairs, want = _stage_pairs()
    call = verify.StageCall(pairs)
    buf = Buffers(fill, bands)
    if bands:
        call.ws, call.rec = buf.workspace(call.ws.numel()), buf.like(call.rec)
    ptrs = (poison(call.ws, fill).data_ptr(), poison(call.rec, fill).data_ptr())
    call.enqueue()
    torch.cuda.synchronize()
    assert (call.ws.data_ptr(), call.rec.data_ptr()) == ptrs
    buf.check(call.ws)
    got = call.records()
    for name, g, w in zip(STAGE_PAIRS, got, want):
        ST.assert_record(g, w, (name, fill))
    return dict(rec=_host(call.rec))


@gpu
@fills
def test_stage_err(fill):
    _vs_control("stage", fill, _stage_err(fill), lambda: _stage_err(0))


# ----------------------------------------------------------------------------------------------------------------------
# 2. guard bands at exactly the queried size, one case per entry family, fill 0x7F
# ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ["fused", "fused carry", "fused traced", "generic f32", "layer", "clips", "float traced", "float clips",
                                    "score", "score clips", "stage"])
def test_guard_bands(family, monkeypatch):
    from sparsernns_amd import _lib
    if family == "fused":
        _forward_checked("A_ragged", _default_engine("A_ragged", monkeypatch), "int32", _lib.FWD_DEFER_REDO, POISON, bands=True)
    elif family == "fused carry":
        _forward_checked("C_grouped", _default_engine("C_grouped", monkeypatch), "int32", 0, POISON, bands=True)
    elif family == "fused traced":
        _forward_checked("H_traced", _default_engine("H_traced", monkeypatch), "int32", 0, POISON, bands=True)
    elif family == "generic f32":
        _forward_checked("A_ragged", _default_engine("A_ragged", monkeypatch, generic=True), "float32", 0, POISON, generic=True, bands=True)
    elif family == "layer":
        _layer_forward(1, POISON, bands=True)
    elif family == "clips":
        _clips(0.5, False, POISON, bands=True)
    elif family == "float traced":
        _float_traced_in_bands(0.5)
    elif family == "float clips":
        _float_clips(0.5, None, POISON, bands=True)
    elif family == "score":
        _check_score(SCORE_CASES[1], 0.001, _score(SCORE_CASES[1], 0.001, POISON, AS.device_case(*SCORE_CASES[1])[2], bands=True))
    elif family == "score clips":
        _score_clips(0.001, POISON, bands=True)
    else:
        _stage_err(POISON, bands=True)


def _float_traced_in_bands(dim):
    import torch
    md, _, dims = FQ.model(dim, RECIPE)
    eng = FQ.engine(dim, RECIPE)
    B, L = FLOAT_CASE[:2]
    x = FQ.make_x(dims, FLOAT_CASE, RECIPE)
    b = FloatBuffers(eng, B, L, POISON, trace=True, hist=True)
    buf = _band_float(b, POISON)
    b.call(torch.from_numpy(x).cuda())
    buf.check(b.ws)
    t = b.planes(x)
    R.check_stages(md, dims["n_layers"], x, t)
    R.check_observers(md, dims["n_layers"], x, t)
    _check_hist(t, dims, B * L)


# ----------------------------------------------------------------------------------------------------------------------
# 3. call history: loud, quiet, quiet and shorter through the same buffers, nothing cleared; a fresh engine sees the quiet ones
# ----------------------------------------------------------------------------------------------------------------------
LOUD, QUIET = 6.0, 0.25
SHORT_L = 203


HISTORY_MODELS = {"overflow": VM.WORKLOADS["G_overflow"][0], "bench": VM.CFG1}


@functools.lru_cache(maxsize=None)
def _history_batches(model):
    """The G_overflow workload's input (scale 6: states leave 16 bits), then scale 0.25 at the same shape and at a smaller L, each
    with the oracle's results -- on that workload's model, or on the bench model (a bit of state headroom), whose pair kernel
    holds the quiet batches' states within its bound."""
    _, B, L, scale = VM.WORKLOADS["G_overflow"]
    assert scale == LOUD
    qc, dims, export, cm = VM._model(HISTORY_MODELS[model])
    out = []
    for Lq, seed, s in ((L, 11 + L, LOUD), (L, 901, QUIET), (SHORT_L, 902, QUIET)):
        fx = VM._input(qc, dims, B, Lq, seed=seed, scale=s)
        ref, rb, re_, rtr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
        tops = [max(int(np.abs(t["xs_re"]).max()), int(np.abs(t["xs_im"]).max())) for t in rtr]
        assert max(tops) > 32767 if s == LOUD else max(tops) <= 32766, (model, s, tops)
        out.append(dict(x=fx.data, ref=ref, rtr=rtr, tops=tops, L=Lq))
    return export, dims, B, fx.bits, fx.exp, (rb, re_), out


def _history_engine(export, dims, B, Lmax, traced, zero):
    """(engine, its buffers at the largest shape): workspace, status words, y and the trace planes, flat."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine
    eng = Engine(export)
    mk = torch.zeros if zero else torch.empty
    bufs = dict(ws=eng.workspace(B, Lmax), y=mk(B * Lmax * dims["d_out"], dtype=torch.int32, device="cuda"),
                tr=[{k: mk(B * Lmax * (dims["P"] if k in WIDE else dims["H"]), dtype=torch.int32, device="cuda") for k in _lib.TRACE_FIELDS}
                    for _ in range(dims["n_layers"])] if traced else None)
    if zero:
        bufs["ws"].zero_()
    return eng, bufs


def _history_run(eng, bufs, dims, B, batch, bits, exp, flags):
    """One forward in the prefix of the buffers; returns host copies of y, the 128 status words and the traces."""
    import torch
    from sparsernns_amd import _lib
    L = batch["L"]
    need = _lib.lib.s5fxp_workspace_bytes(eng._h, B, L)
    eng._wsl[0] = ((B, L, 1, torch.int32), bufs["ws"][:need])
    y = bufs["y"][:B * L * dims["d_out"]].view(B, L, dims["d_out"])
    tr = [{k: t[:B * L * (dims["P"] if k in WIDE else dims["H"])].view(B, L, -1) for k, t in d.items()} for d in bufs["tr"]] if bufs["tr"] else None
    st = eng.lane_status(0)
    eng.enqueue(torch.from_numpy(batch["x"]).cuda(), bits, exp, y, B, L, traces=tr, flags=flags)
    torch.cuda.synchronize()
    assert eng.workspace(B, L).data_ptr() == bufs["ws"].data_ptr() and eng.lane_status(0).data_ptr() == st.data_ptr()
    return dict(y=_host(y), st=_host(st[:_lib.STATUS_WORDS]), tr=[{k: _host(v) for k, v in d.items()} for d in tr] if tr else None)


@gpu
@pytest.mark.parametrize("model,variant", [("overflow", "default"), ("overflow", "default traced"), ("bench", "default"), ("bench", "defer_redo")])
def test_history_of_the_batch_forward(model, variant):
    from sparsernns_amd import _lib
    export, dims, B, bits, exp, (rb, re_), batches = _history_batches(model)
    traced = variant == "default traced"
    flags = _lib.FWD_DEFER_REDO if variant == "defer_redo" else 0
    Lmax = batches[0]["L"]
    used, used_bufs = _history_engine(export, dims, B, Lmax, traced, zero=False)
    fresh, fresh_bufs = _history_engine(export, dims, B, Lmax, traced, zero=True)
    nl = dims["n_layers"]
    bounds = [_lib.lib.s5fxp_model_recurrence_xmax(used._h, i) for i in range(nl)]
    for n, batch in enumerate(batches):
        got = _history_run(used, used_bufs, dims, B, batch, bits, exp, flags)
        w = got["st"]
        assert w[2] == _lib.PATH_FUSED and not (w[0] & (_lib.ST_NEGSHIFT | _lib.ST_NEGEXP | _lib.ST_WIDE_INPUT)), (variant, n, w[:8])
        if n == 0:   # the loud batch: states beyond 16 bits, so beyond every fast kernel's bound
            assert w[0] & _lib.ST_WIDE_STATE, (variant, w[:8])
            if flags:
                assert w[0] & _lib.ST_REDO, (variant, w[:8])
                continue
            assert not (w[0] & _lib.ST_REDO)
        else:        # the quiet ones stay inside 16 bits, and inside the bound the model reports for its optimistic kernel
            assert not flags or all(t <= b for t, b in zip(batch["tops"], bounds)), (batch["tops"], bounds)
            assert not (w[0] & (_lib.ST_REDO | _lib.ST_WIDE_STATE)), (variant, n, w[:8])
        assert np.array_equal(got["y"], batch["ref"]), (variant, n, int(np.count_nonzero(got["y"] != batch["ref"])))
        assert w[1] == 0 and [int(w[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in batch["rtr"]], (variant, n)
        assert [int(w[8 + 8 * i + VM._pre_s5_word(export, i)]) for i in range(nl)] == [t["pre_s5_exp"] for t in batch["rtr"]], (variant, n)
        if traced:
            for i in range(nl):
                for k, ck in VM.TRACE_MAP.items():
                    assert np.array_equal(got["tr"][i][k], batch["rtr"][i][ck]), (variant, n, i, k)
        if n:
            same_results(got, _history_run(fresh, fresh_bufs, dims, B, batch, bits, exp, flags), f"{variant}, batch {n}: against the fresh engine")


@gpu
def test_history_of_the_clip_launch():
    """A loud set of clips, then a quiet set with other lengths, through the same workspace, status words, y and carry out."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine
    model, qc, dims, cm = TC._synth(0.5)
    export = model.export()
    sets = []
    for scale, lens, seed in ((LOUD, TC.EDGE_LENS, 940), (QUIET, TC.EDGE_LENS[::-1], 960)):
        parts = [TC._fx(qc, dims, L, seed=seed + e, scale=scale) for e, L in enumerate(lens)]
        clips, bits, exp = [p[0] for p in parts], parts[0][1], parts[0][2]
        sets.append((lens, clips, bits, exp, [TC._oracle_clip(cm, c, bits, exp, None) if len(c) else None for c in clips]))
    used, fresh = Engine(export), Engine(export)
    n = len(TC.EDGE_LENS)
    keep = (torch.empty((n, 100, used.d_out), dtype=torch.int32, device="cuda"),
            torch.empty((n, used.n_layers, 2, used.P), dtype=torch.int32, device="cuda"))
    for k, (lens, clips, bits, exp, refs) in enumerate(sets):
        got = _clips_launch(used, TC._pad(clips, 100), lens, bits, exp, None, None, lane=0, keep=keep)
        _check_clips(used, export, got, clips, None, refs, False, None, ("history", k))
        # the loud set is loud and the quiet one quiet: states beyond 16 bits in every clip of a tile or more, in none afterwards
        tops = [int(TC._row_state_max(r[4]).max()) if r else 0 for r in refs]
        wide = [bool(w[0] & _lib.ST_WIDE_STATE) for w in got["st"]]
        assert wide == [t > 32767 for t in tops] and sum(wide) == (6 if k == 0 else 0), (k, tops, wide)
    zeros = (torch.zeros_like(keep[0]), torch.zeros_like(keep[1]))
    fresh._clips_workspace(n, 100, 0).zero_()
    want = _clips_launch(fresh, TC._pad(clips, 100), lens, bits, exp, None, None, lane=0, keep=zeros)
    for key in ("sout", "st"):
        assert np.array_equal(got[key], want[key]), key
    for e, L in enumerate(lens):
        assert np.array_equal(got["y"][e, :L], want["y"][e, :L]), e


@gpu
def test_history_of_the_float_forward_without_stats():
    import torch
    from sparsernns_amd import floatmodel
    dim = 0.5
    md, _, dims = FQ.model(dim, RECIPE)
    used, fresh = floatmodel.FloatEngine(md, dims["n_layers"]), floatmodel.FloatEngine(md, dims["n_layers"])
    B, L = FLOAT_CASE[:2]
    y_used = torch.empty(B * L * 257, dtype=torch.float32, device="cuda")
    for n, (Lb, scale, seed) in enumerate(((L, LOUD, 970), (L, QUIET, 971), (33, QUIET, 972))):
        x = synth.make_input(B, Lb, dims["d_in"], seed=seed, scale=scale)
        xd = torch.from_numpy(x).cuda()
        b = FloatBuffers(used, B, Lb, None, trace=False, stats=False, y=y_used[:B * Lb * 257].view(B, Lb, 257))
        b.call(xd)
        assert b.ws.data_ptr() == used._ws[False].data_ptr()   # the one workspace, a prefix of it for the shorter batch
        y = b.result()["y"]
        y64 = R.forward_f64(md, x, dims["n_layers"])
        assert np.abs(y - y64).max() <= 1e-4 * np.abs(y64).max(), (n, float(np.abs(y - y64).max()))   # test_float_model.py's end-to-end bound
        if n:
            f = FloatBuffers(fresh, B, Lb, 0, trace=False, stats=False)
            f.call(xd)
            assert same_bytes(y, f.result()["y"]), n


@gpu
def test_history_of_a_session_pool():
    """Three sessions stream loud chunks; then session 1 is released and started FRESH and session 2 goes on, both with quiet
    chunks, in one ragged push through the pool's status words and output buffer."""
    import torch
    from sparsernns_amd import SessionPool, _lib
    from sparsernns_amd.engine import Engine
    from sparsernns_amd.fxparray import FxpArray
    model, qc, dims, cm = TC._synth(0.5)
    export = model.export()
    nl, P, Lmax = dims["n_layers"], dims["P"], 4
    pool = SessionPool(Engine(export), 3)
    for k in range(3):
        x, bits, exp = SS._fx(qc, dims, 3, 1, Lmax, seed=980 + k, scale=LOUD)
        pool.push(FxpArray(x[:, 0], bits, exp))
        assert pool.last_path == _lib.PATH_STEP
    carry = _host(pool.state)
    # the loud stream was loud: the carries the released slot 1 and the continuing slot 2 hold have left 16 bits
    assert np.abs(carry[1]).max() > 32767 and np.abs(carry[2]).max() > 32767, [int(np.abs(c).max()) for c in carry]
    ids, rows = [1, 2], [4, 3]
    xq, bits, exp = SS._fx(qc, dims, 2, 1, Lmax, seed=990, scale=QUIET)
    y = pool.push_ragged(ids, FxpArray(xq[:, 0].copy(), bits, exp), rows, fresh=[1]).numpy()
    st = _host(pool.engine.lane_status(pool._lane, 2))[:2 * _lib.STATUS_WORDS]
    other = SessionPool(Engine(export), 3)
    other.state.copy_(torch.from_numpy(carry).cuda())
    y2 = other.push_ragged(ids, FxpArray(xq[:, 0].copy(), bits, exp), rows, fresh=[1]).numpy()
    st2 = _host(other.engine.lane_status(other._lane, 2))[:2 * _lib.STATUS_WORDS]
    for e, (slot, L) in enumerate(zip(ids, rows)):
        s = np.zeros((nl, 2, 1, P), dtype=np.int32) if slot == 1 else carry[slot].copy()
        ref = cm.forward(np.ascontiguousarray(xq[e, :, :L]), bits, exp, state=s)[0]
        assert np.array_equal(y[e, :L], ref[0]) and np.array_equal(y2[e, :L], ref[0]), e
        assert np.array_equal(_host(pool.state)[slot], s) and np.array_equal(_host(other.state)[slot], s), e
    assert np.array_equal(st, st2)
    assert np.array_equal(_host(pool.state)[0], carry[0])


# ----------------------------------------------------------------------------------------------------------------------
# 4. the harness can fail
# ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_poison_reaches_memory_the_kernels_read(monkeypatch):
    """stats is only ever raised, so an array filled with 0x7F (3.39e38) comes back as the fill; a state_in of 0x7F bytes is a
    carry the forward must start from -- its output is the oracle's on that carry and not the zero-carry one."""
    import torch
    from sparsernns_amd import _lib
    dims = FQ.model(0.25, RECIPE)[2]
    eng = FQ.engine(0.25, RECIPE)
    B, L = FLOAT_CASE[:2]
    b = FloatBuffers(eng, B, L, POISON, trace=False)
    poison(b.stats, POISON)
    b.call(torch.from_numpy(FQ.make_x(dims, FLOAT_CASE, RECIPE)).cuda())
    assert is_fill(b.stats, POISON) and not is_fill(b.y, POISON)

    work = _work("A_ragged")
    qc, wdims, export, cm = VM._model(VM.CFG1)
    iengine = _default_engine("A_ragged", monkeypatch)
    Bw, Lw = work["B"], work["L"]
    carry = np.full((wdims["n_layers"], 2, Bw, wdims["P"]), 0x7F7F7F7F, dtype=np.int32)
    after = carry.copy()
    ref = cm.forward(work["x"], work["bits"], work["exp"], state=after)[0]
    assert not np.array_equal(ref, work["ref"])
    sin = poisoned(carry.shape, torch.int32, POISON)
    assert np.array_equal(_host(sin), carry)
    y, sout = poisoned(ref.shape, torch.int32, POISON), poisoned(carry.shape, torch.int32, POISON)
    iengine.enqueue(torch.from_numpy(work["x"]).cuda(), work["bits"], work["exp"], y, Bw, Lw, state_in=sin, state_out=sout)
    st = iengine.check_status()
    assert st[2] == _lib.PATH_FUSED and not (st[0] & (_lib.ST_NEGSHIFT | _lib.ST_NEGEXP | _lib.ST_WIDE_INPUT | _lib.ST_REDO)), st[:8]
    assert np.array_equal(_host(y), ref) and not np.array_equal(_host(y), work["ref"])
    assert np.array_equal(_host(sout), after)
