"""The clip kernel with trace planes (include/s5fxp.h s5fxp_model_clips_traced[_f32], csrc/s5fxp_clip_body.inc with CLIP_TRACE;
DESIGN.md §4x): one launch, and rows t < len of all eleven planes of every layer are bit for bit what a forward of that clip
alone stores.  The reference is the C oracle (oracle/cref.py CModel.forward(trace=True, state=...)), run per clip on the CPU
and shared with tests/test_clips.py (its clip lists, models and inputs); for one shape also Engine.forward(traces=True) on the
clip alone.  Every plane is pre-filled with a sentinel: rows from len on, and every row of a clip that stops with
ST_WIDE_INPUT, must still hold it.  y, the carry and the status words are compared with the untraced launch's, np.array_equal.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_clips as TC
from test_clips import EDGE_LENS, SENTINEL, _fx, _oracle_clip, _pad, _synth

gpu = pytest.mark.gpu
ORACLE_KEY = dict(pre_s5="pre_s5", u="u", Bu_re="bu_re", Bu_im="bu_im", xs_re="xs_re", xs_im="xs_im", ys="ys", out2="out2",
                  out2_sigmoid="sigmoid", post_GLU="post_glu", residadd="residadd")
SYMBOLS = ("s5fxp_model_clips_traced", "s5fxp_model_clips_traced_f32")


# ------------------------------------------------------------------------------------------------------------------
# not GPU: the ABI surface
# ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_at_version_115():
    from sparsernns_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "s5fxp.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and hasattr(_lib.lib, name), name
    assert _lib.lib.s5fxp_version() == 115 and "#define S5FXP_VERSION 115" in hdr
    assert set(ORACLE_KEY) == set(_lib.TRACE_FIELDS) and C.sizeof(_lib.LayerTrace) == 88
    assert _lib.CLIPS_TRACED_MAX_LAYERS == 8 and "more than 8 layers" in hdr


def test_argument_checks_without_a_device():
    from sparsernns_amd import _lib

    lib = _lib.lib
    buf = (C.c_int32 * 4096)()
    p = C.addressof(buf)
    tr = (_lib.LayerTrace * 1)()
    for entry in (lib.s5fxp_model_clips_traced, lib.s5fxp_model_clips_traced_f32):
        call = lambda m=None, x=p, n=1, Lmax=4, lens=p, y=p, ws=p, wsb=16384, st=p, tr=tr: entry(
            m, x, 16, 14, n, Lmax, lens, y, None, None, ws, wsb, st, tr, None)
        assert call() == _lib.S5FXP_EBADARG   # null model
        for kw in (dict(n=0), dict(n=-3), dict(Lmax=0), dict(Lmax=-1), dict(x=None), dict(y=None), dict(lens=None), dict(ws=None),
                   dict(st=None), dict(wsb=0), dict(tr=None)):
            assert call(**kw) == _lib.S5FXP_EBADARG, kw


# ------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------
def _planes(eng, n, Lmax):
    import torch
    from sparsernns_amd import _lib
    return [{k: torch.full((n, Lmax, eng.P if k in ("Bu_re", "Bu_im", "xs_re", "xs_im") else eng.H), SENTINEL, dtype=torch.int32,
                           device="cuda") for k in _lib.TRACE_FIELDS} for _ in range(eng.n_layers)]


def _launch_traced(eng, x, lens, bits, exp, state=None, lane=2, drop=()):
    """TC._launch on the traced entry: y, a separate state_out and all planes pre-filled with the sentinel.  `drop`: plane
    names handed in as NULL.  Returns y, carry out, status (n, 128), traces as NumPy."""
    import torch
    from sparsernns_amd import _lib
    n = x.shape[0]
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    y = torch.full((n, x.shape[1], eng.d_out), SENTINEL, dtype=torch.int32, device="cuda")
    if x.dtype == np.float32:
        y = y.view(torch.float32)
    sin = torch.from_numpy(np.ascontiguousarray(state)).cuda() if state is not None else None
    sout = torch.full((n, eng.n_layers, 2, eng.P), SENTINEL, dtype=torch.int32, device="cuda")
    planes = _planes(eng, n, x.shape[1])
    given = [{k: v for k, v in pl.items() if k not in drop} for pl in planes]
    y2, tr = eng.clips_traced(xd, torch.tensor(list(lens), dtype=torch.int32, device="cuda"), y, sin, sout, bits, exp, lane=lane,
                              traces=given)
    assert y2 is y and tr is given
    torch.cuda.synchronize()
    st = eng.lane_status(lane, n).cpu().numpy()[:n * _lib.STATUS_WORDS].reshape(n, _lib.STATUS_WORDS).copy()
    return y.cpu().numpy(), sout.cpu().numpy(), st, [{k: v.cpu().numpy() for k, v in pl.items()} for pl in planes]


def _check_traces(traces, clips, refs, tag, untouched=()):
    """Rows < len of every plane against the oracle's trace of the clip alone; rows >= len (all rows of `untouched` clips and of
    empty ones) still the sentinel."""
    for e, clip in enumerate(clips):
        L = len(clip) if e not in untouched else 0
        for i, pl in enumerate(traces):
            for k, got in pl.items():
                assert np.all(got[e, L:] == SENTINEL), (tag, e, i, k, "rows beyond len were written")
                if L:
                    want = refs[e][4][i][ORACLE_KEY[k]]
                    assert np.array_equal(got[e, :L], want), (tag, e, i, k, int(np.count_nonzero(got[e, :L] != want)))


def _same_as_untraced(eng, x, lens, bits, exp, state, got, tag):
    y, sout, st = TC._launch(eng, x, lens, bits, exp, state, lane=0)
    assert np.array_equal(got[0].view(np.int32), y.view(np.int32)), (tag, "y")
    assert np.array_equal(got[1], sout), (tag, "carry")
    assert np.array_equal(got[2], st), (tag, "status")


# ------------------------------------------------------------------------------------------------------------------
# 1. tile edges, with a carry and from state_in = NULL; against the oracle and the untraced launch
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ds", (0.25, 0.5, 1.0))   # the ragged and the full channel tile; 1.0: P = 128, the widest state tile
def test_tile_edges(ds):
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    clips, bits, exp, states, refs = TC._edge_case(ds)
    x = _pad(clips, 100, fill=0x7fffffff)   # padding rows are never read
    got = _launch_traced(eng, x, EDGE_LENS, bits, exp, states)
    TC._check(eng, cm, model.export(), got[:3], clips, bits, exp, states, refs, (ds, "traced edges"))
    _check_traces(got[3], clips, refs, (ds, "edges"))
    _same_as_untraced(eng, x, EDGE_LENS, bits, exp, states, got, (ds, "edges"))
    if ds == 0.5:   # from a zero carry (state_in NULL), and with planes left out
        zrefs = [_oracle_clip(cm, c, bits, exp, None) if len(c) else None for c in clips]
        drop = ("u", "Bu_im", "xs_re", "out2", "residadd")
        got = _launch_traced(eng, x, EDGE_LENS, bits, exp, None, drop=drop)
        TC._check(eng, cm, model.export(), got[:3], clips, bits, exp, None, zrefs, (ds, "traced edges, zero carry"))
        kept = [{k: v for k, v in pl.items() if k not in drop} for pl in got[3]]
        _check_traces(kept, clips, zrefs, (ds, "zero carry"))
        for pl in got[3]:   # a NULL plane is not written anywhere
            assert all(np.all(pl[k] == SENTINEL) for k in drop)
        _same_as_untraced(eng, x, EDGE_LENS, bits, exp, None, got, (ds, "zero carry"))


@gpu
def test_rows_equal_the_batch_path_traces_of_the_clip_alone():
    import torch
    from sparsernns_amd.fxparray import FxpArray
    model, qc, dims, cm = _synth(0.5)
    eng = model.engine()
    lens = (33, 64, 1)
    parts = [_fx(qc, dims, L, seed=900 + L) for L in lens]
    clips, bits, exp = [p[0] for p in parts], parts[0][1], parts[0][2]
    got = _launch_traced(eng, _pad(clips, 64), lens, bits, exp, None)
    for e, clip in enumerate(clips):
        y, tr = eng.forward(FxpArray(torch.from_numpy(np.ascontiguousarray(clip[None])).cuda(), bits, exp), traces=True)
        torch.cuda.synchronize()
        assert np.array_equal(y.numpy()[0], got[0][e, :lens[e]]), e
        for i in range(eng.n_layers):
            for k, v in tr[i].items():
                assert np.array_equal(v.cpu().numpy()[0], got[3][i][k][e, :lens[e]]), (e, i, k)


# ------------------------------------------------------------------------------------------------------------------
# 2. wide states: a tile takes the four-plane C projection
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ds", (0.5,))
def test_wide_states(ds):
    """tests/test_clips.py::test_wide_states' recipe: clip 0 carries 27-bit values (four state planes in every tile), clip 1 one
    17-bit value in the last layer's fastest-decaying state (four planes in the first tile only), clip 2 stays in 16 bits."""
    from sparsernns_amd import _lib
    model, qc, dims, cm = _synth(ds)
    eng, export = model.engine(), model.export()
    nl, P, L = dims["n_layers"], dims["P"], 70
    parts = [_fx(qc, dims, L, seed=400 + e) for e in range(3)]
    clips, bits, exp = [p[0] for p in parts], parts[0][1], parts[0][2]
    rng = np.random.Generator(np.random.PCG64(5))
    states = np.zeros((3, nl, 2, P), dtype=np.int32)
    states[0] = rng.integers(-2 ** 26, 2 ** 26, states[0].shape, dtype=np.int64).astype(np.int32)
    m, q = export["params"]["encoder"][f"layers_{nl - 1}"]["mixer"], export["qconfig"]["encoder"][f"layers_{nl - 1}"]["mixer"]
    absA = np.hypot(np.asarray(m["A_real"], dtype=np.float64) / 2.0 ** int(q["A_real_exp"]),
                    np.asarray(m["A_imag"], dtype=np.float64) / 2.0 ** int(q["A_imag_exp"]))
    states[1, nl - 1, 0, int(np.argmin(absA))] = 65000
    states[2] = rng.integers(-100, 100, states[2].shape, dtype=np.int64).astype(np.int32)
    refs = [_oracle_clip(cm, c, bits, exp, states[e]) for e, c in enumerate(clips)]
    mx = [TC._row_state_max(r[4]) for r in refs]
    assert all(mx[0][:, t0:t0 + 32].max() > 32767 for t0 in (0, 32, 64)) and mx[1][nl - 1, :32].max() > 32767 and mx[2].max() <= 32767
    got = _launch_traced(eng, _pad(clips, L), [L] * 3, bits, exp, states.copy())
    TC._check(eng, cm, export, got[:3], clips, bits, exp, states, refs, (ds, "traced wide states"), wide_state=[True, True, False])
    _check_traces(got[3], clips, refs, (ds, "wide states"))
    assert got[2][0][0] & _lib.ST_WIDE_STATE


# ------------------------------------------------------------------------------------------------------------------
# 3. a clip with a wide input leaves its planes alone
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_wide_input_clip_leaves_its_planes_untouched():
    from sparsernns_amd import _lib
    ds = 0.5
    model, qc, dims, cm = _synth(ds)
    eng, export = model.engine(), model.export()
    lens = (50, 100, 80)
    parts = [_fx(qc, dims, L, seed=500 + L) for L in lens]
    clips, bits, exp = [p[0].copy() for p in parts], parts[0][1], parts[0][2]
    clips[1][70, 5] = 40000   # beyond 16 bits, in the third tile
    rng = np.random.Generator(np.random.PCG64(12))
    states = rng.integers(-3000, 3000, (3, dims["n_layers"], 2, dims["P"]), dtype=np.int64).astype(np.int32)
    refs = [_oracle_clip(cm, c, bits, exp, states[e]) for e, c in enumerate(clips)]
    x = _pad(clips, 100)
    got = _launch_traced(eng, x, lens, bits, exp, states)
    y, sout, st, traces = got
    assert st[1][0] & _lib.ST_WIDE_INPUT and np.all(y[1] == SENTINEL) and np.all(sout[1] == SENTINEL)
    _check_traces(traces, clips, refs, "wide input", untouched=(1,))
    keep = [0, 2]
    TC._check(eng, cm, export, (y[keep], sout[keep], st[keep]), [clips[0], clips[2]], bits, exp, states[keep], [refs[0], refs[2]],
              "neighbours of a wide input, traced")
    _same_as_untraced(eng, x, lens, bits, exp, states, got, "wide input")


# ------------------------------------------------------------------------------------------------------------------
# 4. the float32 entry
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_float_entry():
    import torch
    from sparsernns_amd import synth
    from sparsernns_amd._lib import check, lib
    ds = 0.25
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    lens = (0, 5, 33, 70)
    n, Lmax = len(lens), 70
    xf = np.stack([synth.make_input(1, Lmax, dims["d_in"], seed=700 + e, scale=(1.0, 6.0, 0.0, 1.0)[e])[0] for e in range(n)])
    xfd = torch.from_numpy(xf).cuda()
    xi = torch.empty(xfd.shape, dtype=torch.int32, device="cuda")
    check(lib.s5fxp_from_fp(xfd.data_ptr(), xi.data_ptr(), xfd.numel(), bits, exp, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    xin = xi.cpu().numpy()
    clips = [xin[e, :L] for e, L in enumerate(lens)]
    refs = [_oracle_clip(cm, c, bits, exp, None) if len(c) else None for c in clips]
    got = _launch_traced(eng, xf, lens, bits, exp, None)
    assert got[0].dtype == np.float32
    _check_traces(got[3], clips, refs, "float entry")
    _same_as_untraced(eng, xf, lens, bits, exp, None, got, "float entry")
    for e, L in enumerate(lens):
        if L:
            assert np.array_equal(got[0][e, :L].view(np.int32), np.ldexp(refs[e][0].astype(np.float32), -eng.out_exp).view(np.int32)), e


# ------------------------------------------------------------------------------------------------------------------
# arguments on a real handle
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_arguments_on_a_real_handle():
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine
    lib = _lib.lib
    model, qc, dims, cm = _synth(0.5)
    eng = model.engine()
    n, Lmax = 2, 40
    x = torch.zeros((n, Lmax, dims["d_in"]), dtype=torch.int32, device="cuda")
    y = torch.zeros((n, Lmax, dims["d_out"]), dtype=torch.int32, device="cuda")
    lens = torch.tensor([40, 7], dtype=torch.int32, device="cuda")
    st = torch.zeros(n * _lib.STATUS_WORDS, dtype=torch.int32, device="cuda")
    need = lib.s5fxp_clips_workspace_bytes(eng._h, n, Lmax)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    tr = (_lib.LayerTrace * eng.n_layers)()   # every plane NULL: legal
    s = torch.cuda.current_stream().cuda_stream
    call = lambda h=eng._h, n=n, Lmax=Lmax, lens=lens.data_ptr(), wsb=need, bits=16, tr=tr: lib.s5fxp_model_clips_traced(
        h, x.data_ptr(), bits, 14, n, Lmax, lens, y.data_ptr(), None, None, ws.data_ptr(), wsb, st.data_ptr(), tr, s)
    assert call(tr=None) == _lib.S5FXP_EBADARG
    assert call(n=0) == _lib.S5FXP_EBADARG and call(Lmax=0) == _lib.S5FXP_EBADARG and call(lens=None) == _lib.S5FXP_EBADARG
    assert call(wsb=need - 1) == _lib.S5FXP_EBADARG and call(bits=0) == _lib.S5FXP_EBADARG and call(bits=33) == _lib.S5FXP_EBADARG
    gen = Engine(model.export(), flags=_lib.MODEL_FORCE_GENERIC)
    assert call(h=gen._h) == _lib.S5FXP_EUNSUPPORTED
    assert call() == _lib.S5FXP_OK
    torch.cuda.synchronize()
    assert int(st[2].item()) == _lib.PATH_CLIP and int(st[_lib.STATUS_WORDS + 2].item()) == _lib.PATH_CLIP
