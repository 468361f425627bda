"""The clip kernel (include/s5fxp.h s5fxp_model_clips, csrc/s5fxp_clip.hpp): n clips of different lengths in one launch, one
workgroup per clip looping over 32-row tiles.  Every GPU comparison is np.array_equal against the C oracle
(oracle/cref.py CModel.forward(x[e, :len], bits, exp, trace=True, state=...)) run per clip on the CPU; where noted also
against the batch path (Engine.enqueue(B=1, L=len)) on the same device.

The oracle's traces carry two of the five per-layer exponents (the BatchNorm output's and the residual add's); those two
status words are compared with the oracle, all five with the batch path.
"""
import functools

import numpy as np
import pytest

from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth

gpu = pytest.mark.gpu
SHAPES = (0.25, 0.5, 0.75, 1.0)
EDGE_LENS = (0, 1, 31, 32, 33, 64, 65, 100)
SENTINEL = -123456789


# ------------------------------------------------------------------------------------------------------------------
# not GPU: the ABI surface
# ------------------------------------------------------------------------------------------------------------------
CLIP_SYMBOLS = ("s5fxp_clips_workspace_bytes", "s5fxp_model_clips_ok", "s5fxp_model_clips", "s5fxp_model_clips_f32")


def test_clip_symbols_version_and_path_code():
    import ctypes as C
    from sparsernns_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in CLIP_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert _lib.lib.s5fxp_version() >= 112
    assert _lib.PATH_CLIP == 4


def test_clip_argument_checks_without_a_device():
    import ctypes as C
    from sparsernns_amd import _lib

    lib = _lib.lib
    buf = (C.c_int32 * 4096)()
    p = C.addressof(buf)
    for entry in (lib.s5fxp_model_clips, lib.s5fxp_model_clips_f32):
        call = lambda m=None, x=p, n=1, Lmax=4, lens=p, y=p, ws=p, wsb=16384, st=p: entry(
            m, x, 16, 14, n, Lmax, lens, y, None, None, ws, wsb, st, None)
        assert call() == _lib.S5FXP_EBADARG   # null model
        for kw in (dict(n=0), dict(n=-3), dict(Lmax=0), dict(Lmax=-1), dict(x=None), dict(y=None), dict(lens=None), dict(ws=None),
                   dict(st=None), dict(wsb=0)):
            assert call(**kw) == _lib.S5FXP_EBADARG, kw
    assert lib.s5fxp_model_clips_ok(None, 1) == -1


def test_clip_workspace_bytes_is_zero_on_bad_arguments():
    from sparsernns_amd import _lib

    lib = _lib.lib
    assert lib.s5fxp_clips_workspace_bytes(None, 1, 1) == 0
    assert lib.s5fxp_clips_workspace_bytes(None, 0, 1) == 0
    assert lib.s5fxp_clips_workspace_bytes(None, 1, 0) == 0


# ------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synth(ds):
    from sparsernns_amd.fxpmodel import build_regression_model
    md, qc, dims = synth.make_model(dim_scale=ds, calib_L=256)
    model = build_regression_model(md, qc, dims["n_layers"])
    return model, qc, dims, cref.CModel(model.export())


def _fx(qc, dims, L, seed, scale=1.0):
    """One clip (L, d_in) int32 at the encoder's input configuration."""
    x = synth.make_input(1, max(L, 1), dims["d_in"], seed=seed, scale=scale)
    f = O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    return f.data[0, :L], f.bits, f.exp


def _pad(clips, Lmax, fill=0):
    x = np.full((len(clips), Lmax, clips[0].shape[-1]), fill, dtype=clips[0].dtype)
    for e, c in enumerate(clips):
        x[e, :len(c)] = c
    return x


def _bn_word(export, i):
    norm = export["params"]["encoder"][f"layers_{i}"]["norm"]
    return 3 if "bias" in norm else (2 if "scale" in norm else 1)


def _oracle_clip(cm, clip, bits, exp, state):
    """state (nl, 2, P) or None, left as it is -> (y, y_exp, [(pre_s5_exp, residadd_exp)], state out (nl, 2, P), traces)."""
    st = np.zeros((cm.n_layers, 2, 1, cm.P), dtype=np.int32) if state is None else state[:, :, None, :].copy()   # the oracle writes it
    y, _, ye, tr = cm.forward(clip, bits, exp, trace=True, state=st)
    return y, ye, [(int(t["pre_s5_exp"]), int(t["residadd_exp"])) for t in tr], st[:, :, 0, :], tr


def _launch(eng, x, lens, bits, exp, state=None, alias=False, lane=0):
    """x np (n, Lmax, d_in) int32 or float32, state np (n, nl, 2, P) or None.  y and a separate state_out are pre-filled with
    sentinels.  Returns y, carry out, status (n, 128)."""
    import torch
    from sparsernns_amd import _lib
    n = x.shape[0]
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    y = torch.full((n, x.shape[1], eng.d_out), SENTINEL, dtype=torch.int32, device="cuda")
    if x.dtype == np.float32:
        y = y.view(torch.float32)
    sin = torch.from_numpy(np.ascontiguousarray(state)).cuda() if state is not None else None
    sout = sin if alias else torch.full((n, eng.n_layers, 2, eng.P), SENTINEL, dtype=torch.int32, device="cuda")
    eng.clips(xd, torch.tensor(list(lens), dtype=torch.int32, device="cuda"), y, sin, sout, bits, exp, lane=lane)
    torch.cuda.synchronize()
    st = eng.lane_status(lane, n).cpu().numpy()[:n * _lib.STATUS_WORDS].reshape(n, _lib.STATUS_WORDS).copy()
    return y.cpu().numpy(), sout.cpu().numpy(), st


def _batch_clip(eng, clip, bits, exp, state, lane=1):
    """The same clip alone through the batch path (a self-contained forward at B = 1, L = len)."""
    import torch
    from sparsernns_amd import _lib
    L = clip.shape[0]
    xd = torch.from_numpy(np.ascontiguousarray(clip[None])).cuda()
    y = torch.empty((1, L, eng.d_out), dtype=torch.int32, device="cuda")
    sin = torch.from_numpy(np.ascontiguousarray(state[:, :, None, :])).cuda() if state is not None else None
    sout = torch.empty((eng.n_layers, 2, 1, eng.P), dtype=torch.int32, device="cuda")
    eng.enqueue(xd, bits, exp, y, 1, L, flags=0, lane=lane, state_in=sin, state_out=sout)
    torch.cuda.synchronize()
    return y.cpu().numpy()[0], sout.cpu().numpy()[:, :, 0, :], eng.lane_status(lane).cpu().numpy()[:_lib.STATUS_WORDS].copy()


def _check(eng, cm, export, got, clips, bits, exp, states, refs, tag, batch=False, wide_state=None):
    """got = (y, carry out, status) of one launch of `clips` (list of (len, d_in)); states: per-clip carry in or None."""
    from sparsernns_amd import _lib
    y, sout, st = got
    nl, P = eng.n_layers, eng.P
    mask = _lib.ST_NEGSHIFT | _lib.ST_NEGEXP | _lib.ST_WIDE_INPUT
    for e, clip in enumerate(clips):
        L, w = len(clip), st[e]
        sin = None if states is None else states[e]
        assert w[2] == _lib.PATH_CLIP and w[1] == eng.out_exp, (tag, e, w[:8])
        assert np.all(y[e, L:] == SENTINEL), (tag, e, "rows beyond len were written")
        for i in range(nl):
            assert (w[8 + 8 * i + 5], w[8 + 8 * i + 6], w[8 + 8 * i + 7]) == (6, P, P), (tag, e, i)
        if L == 0:
            assert w[0] == 0 and not any(w[8 + 8 * i + j] for i in range(nl) for j in range(5)), (tag, e, w[:32])
            assert np.array_equal(sout[e], np.zeros_like(sout[e]) if sin is None else sin), (tag, e, "carry of an empty clip")
            continue
        ref, ye, exps, sref, _ = refs[e]
        assert not (w[0] & mask) and w[1] == ye, (tag, e, w[:8])
        assert np.array_equal(y[e, :L], ref), (tag, e, L, int(np.count_nonzero(y[e, :L] != ref)))
        assert np.array_equal(sout[e], sref), (tag, e, L, "carry")
        for i in range(nl):
            assert w[8 + 8 * i + _bn_word(export, i)] == exps[i][0] and w[8 + 8 * i + 4] == exps[i][1], (tag, e, i, w[8 + 8 * i:16 + 8 * i], exps[i])
        if wide_state is not None:
            assert bool(w[0] & _lib.ST_WIDE_STATE) == wide_state[e], (tag, e, w[0])
        if batch:
            yb, sb, wb = _batch_clip(eng, clip, bits, exp, sin)
            assert np.array_equal(yb, ref) and np.array_equal(sb, sref), (tag, e, "batch path")
            assert wb[2] == _lib.PATH_FUSED and (w[0] & mask) == (wb[0] & mask), (tag, e)
            for i in range(nl):
                assert list(w[8 + 8 * i:13 + 8 * i]) == list(wb[8 + 8 * i:13 + 8 * i]), (tag, e, i)


# ------------------------------------------------------------------------------------------------------------------
# 1. tile edges, 2. padding is invisible
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_case(ds):
    """The 8 clips of the tile-edge launch, their carries in and the oracle's results: computed once, shared by tests 1 and 2."""
    model, qc, dims, cm = _synth(ds)
    parts = [_fx(qc, dims, L, seed=100 + L) for L in EDGE_LENS]
    clips, bits, exp = [p[0] for p in parts], parts[0][1], parts[0][2]
    rng = np.random.Generator(np.random.PCG64(11))
    states = rng.integers(-3000, 3000, (len(clips), dims["n_layers"], 2, dims["P"]), dtype=np.int64).astype(np.int32)
    refs = [_oracle_clip(cm, c, bits, exp, states[e]) if len(c) else None for e, c in enumerate(clips)]
    return clips, bits, exp, states, refs


@gpu
@pytest.mark.parametrize("ds", SHAPES)
def test_tile_edges(ds):
    from sparsernns_amd import _lib
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    assert _lib.lib.s5fxp_model_clips_ok(eng._h, 100) == 1
    clips, bits, exp, states, refs = _edge_case(ds)
    got = _launch(eng, _pad(clips, 100), EDGE_LENS, bits, exp, states)
    _check(eng, cm, model.export(), got, clips, bits, exp, states, refs, (ds, "edges"), batch=True)
    # from a zero carry (state_in NULL) too: the reference's own start
    zrefs = [_oracle_clip(cm, c, bits, exp, None) if len(c) else None for c in clips]
    got = _launch(eng, _pad(clips, 100), EDGE_LENS, bits, exp, None)
    _check(eng, cm, model.export(), got, clips, bits, exp, None, zrefs, (ds, "edges, zero carry"))


@gpu
@pytest.mark.parametrize("ds", SHAPES)
def test_padding_rows_are_never_read(ds):
    from sparsernns_amd import _lib
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    clips, bits, exp, states, refs = _edge_case(ds)
    got = _launch(eng, _pad(clips, 100, fill=0x7fffffff), EDGE_LENS, bits, exp, states)
    assert not (got[2][:, 0] & _lib.ST_WIDE_INPUT).any()
    _check(eng, cm, model.export(), got, clips, bits, exp, states, refs, (ds, "padding 0x7fffffff"))
    plain = _launch(eng, _pad(clips, 100), EDGE_LENS, bits, exp, states, lane=1)
    for a, b in zip(got, plain):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 3. clips are independent
# ------------------------------------------------------------------------------------------------------------------
SCALES = (0.0, 0.05, 1.0, 6.0)


@gpu
@pytest.mark.parametrize("ds", SHAPES)
def test_clips_choose_their_own_exponents(ds):
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    lens = [(40, 70)[e & 1] for e in range(8)]
    parts = [_fx(qc, dims, lens[e], seed=300 + e, scale=SCALES[e // 2]) for e in range(8)]
    clips, bits, exp = [p[0] for p in parts], parts[0][1], parts[0][2]
    refs = [_oracle_clip(cm, c, bits, exp, None) for c in clips]
    # on the CPU, before anything is compared: the scales really lead to different exponents
    e = [refs[2 * k][2] for k in range(4)]
    assert e[2] != e[3] and e[2] not in (e[0], e[1]) and e[3] not in (e[0], e[1]), (ds, e)
    got = _launch(eng, _pad(clips, 70), lens, bits, exp, None)
    _check(eng, cm, model.export(), got, clips, bits, exp, None, refs, (ds, "scales"))
    for k, clip in enumerate(clips):   # each equals its own single-clip launch
        y1, s1, st1 = _launch(eng, clip[None], [lens[k]], bits, exp, None, lane=1)
        assert np.array_equal(y1[0], got[0][k, :lens[k]]) and np.array_equal(s1[0], got[1][k]), (ds, k)
        assert np.array_equal(st1[0], got[2][k]), (ds, k)


# ------------------------------------------------------------------------------------------------------------------
# 4. wide states
# ------------------------------------------------------------------------------------------------------------------
def _row_state_max(tr):
    """max |state| per frame, over all layers -> (n_layers, L)"""
    return np.stack([np.maximum(np.abs(t["xs_re"].astype(np.int64)), np.abs(t["xs_im"].astype(np.int64))).max(axis=-1) for t in tr])


@gpu
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("ds", SHAPES)
def test_wide_states(ds, alias):
    """Clip 0: a planted carry of 27-bit values in every state.  The synthetic models' |A| is 0.95 .. 0.9995, so such a carry is
    still beyond 16 bits after 70 frames: all three tiles take four state planes.  Clip 1 is what reaches the MIXED case: one
    17-bit value planted in the last layer's fastest-decaying state (the last layer: a wide state there reaches no other
    layer's states), which is back inside 16 bits before the first tile ends -- the first tile takes four planes, the later
    tiles two (asserted on the oracle's traces before anything is compared).  Clip 2 has a small carry and never leaves 16 bits."""
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
    mx = [_row_state_max(r[4]) for r in refs]
    assert all(mx[0][:, t0:t0 + 32].max() > 32767 for t0 in (0, 32, 64)), (ds, "27-bit carry")
    assert mx[1][nl - 1, :32].max() > 32767 and mx[1][:, 32:].max() <= 32767, (ds, mx[1][:, :32].max(axis=1), mx[1][:, 32:].max(axis=1))
    assert mx[2].max() <= 32767, ds
    got = _launch(eng, _pad(clips, L), [L] * 3, bits, exp, states.copy(), alias=alias)
    _check(eng, cm, export, got, clips, bits, exp, states, refs, (ds, "wide states", alias), wide_state=[True, True, False])


# ------------------------------------------------------------------------------------------------------------------
# 5. a wide input in a late tile
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ds", (0.5, 1.0))
def test_wide_input_in_a_late_tile(ds):
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    model, qc, dims, cm = _synth(ds)
    eng, export = model.engine(), model.export()
    lens = (50, 100, 80)
    parts = [_fx(qc, dims, L, seed=500 + L) for L in lens]
    clips, bits, exp = [p[0].copy() for p in parts], parts[0][1], parts[0][2]
    clips[1][70, 5] = 40000   # beyond 16 bits, in the third tile (legal in the reference, which only clips on a conversion)
    rng = np.random.Generator(np.random.PCG64(12))
    states = rng.integers(-3000, 3000, (3, dims["n_layers"], 2, dims["P"]), dtype=np.int64).astype(np.int32)
    refs = [_oracle_clip(cm, c, bits, exp, states[e]) for e, c in enumerate(clips)]
    y, sout, st = _launch(eng, _pad(clips, 100), lens, bits, exp, states)
    assert st[1][0] & _lib.ST_WIDE_INPUT and st[1][2] == _lib.PATH_CLIP
    assert np.all(y[1] == SENTINEL) and np.all(sout[1] == SENTINEL)
    keep = [0, 2]
    _check(eng, cm, export, (y[keep], sout[keep], st[keep]), [clips[0], clips[2]], bits, exp, states[keep], [refs[0], refs[2]],
           (ds, "neighbours of a wide input"))
    zrefs = [_oracle_clip(cm, c, bits, exp, None) for c in clips]
    out = eng.forward_clips([FxpArray(c, bits, exp) for c in clips])
    for e in range(3):
        assert out[e].exp == zrefs[e][1] and np.array_equal(out[e].numpy(), zrefs[e][0]), (ds, e)
    out = model.forward_clips([FxpArray(c, bits, exp) for c in clips])
    assert all(np.array_equal(out[e].numpy(), zrefs[e][0]) for e in range(3))


# ------------------------------------------------------------------------------------------------------------------
# 6. more clips than CUs
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_more_clips_than_cus():
    model, qc, dims, cm = _synth(0.5)
    eng = model.engine()
    n = 600
    lens = [e % 4 for e in range(n)]
    pool, bits, exp = _fx(qc, dims, 3 * n, seed=600)
    clips = [pool[3 * e:3 * e + lens[e]] for e in range(n)]
    rng = np.random.Generator(np.random.PCG64(13))
    states = rng.integers(-3000, 3000, (n, dims["n_layers"], 2, dims["P"]), dtype=np.int64).astype(np.int32)
    refs = [_oracle_clip(cm, c, bits, exp, states[e]) if len(c) else None for e, c in enumerate(clips)]
    got = _launch(eng, _pad(clips, 3), lens, bits, exp, states)
    _check(eng, cm, model.export(), got, clips, bits, exp, states, refs, "n = 600")


# ------------------------------------------------------------------------------------------------------------------
# 7. float entry; the carry continues a stream
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ds", SHAPES)
def test_float_entry_and_carry_hand_over(ds):
    import torch
    from sparsernns_amd import SessionPool, _lib
    from sparsernns_amd._lib import check, lib
    from sparsernns_amd.fxparray import FxpArray
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    lens = (0, 5, 33, 70, 64)
    n, Lmax = len(lens), 70
    xf = np.stack([synth.make_input(1, Lmax, dims["d_in"], seed=700 + e, scale=(1.0, 6.0, 0.0, 1.0, 0.3)[e])[0] for e in range(n)])
    xfd = torch.from_numpy(xf).cuda()
    xi = torch.empty(xfd.shape, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    check(lib.s5fxp_from_fp(xfd.data_ptr(), xi.data_ptr(), xfd.numel(), bits, exp, 0, stream))
    torch.cuda.synchronize()
    xin = xi.cpu().numpy()
    yi, si, sti = _launch(eng, xin, lens, bits, exp, None, lane=0)
    yf, sf, stf = _launch(eng, xf, lens, bits, exp, None, lane=1)
    assert yf.dtype == np.float32
    want = np.ldexp(yi.astype(np.float32), -eng.out_exp)
    for e, L in enumerate(lens):
        assert np.array_equal(yf[e, :L].view(np.int32), want[e, :L].view(np.int32)), (ds, e)
        assert np.all(yf[e, L:].view(np.int32) == SENTINEL), (ds, e)
    assert np.array_equal(si, sf) and np.array_equal(sti, stf)
    clips = [xin[e, :L] for e, L in enumerate(lens)]
    refs = [_oracle_clip(cm, c, bits, exp, None) if len(c) else None for c in clips]
    _check(eng, cm, model.export(), (yi, si, sti), clips, bits, exp, None, refs, (ds, "int entry of the float test"))
    outs = eng.forward_clips_float([xf[e, :L] for e, L in enumerate(lens)])
    for e, L in enumerate(lens):
        assert outs[e].dtype == torch.float32 and np.array_equal(outs[e].cpu().numpy().view(np.int32), want[e, :L].view(np.int32)), (ds, e)
    # the carry continues a stream as the oracle does from that state: Engine.step and a SessionPool
    nxt = [_fx(qc, dims, 4, seed=750 + e)[0] for e in range(n)]
    cont = [_oracle_clip(cm, c, bits, exp, si[e]) for e, c in enumerate(nxt)]
    carry = torch.from_numpy(si[:, :, :, None, :].copy()).cuda()
    y = eng.step(torch.from_numpy(np.stack(nxt)[:, None]).cuda(), carry, None, 1, 4, n, bits, exp, lane=2)
    torch.cuda.synchronize()
    for e in range(n):
        assert np.array_equal(y[e, 0].cpu().numpy(), cont[e][0]) and np.array_equal(carry[e, :, :, 0].cpu().numpy(), cont[e][3]), (ds, e)
    pool = SessionPool(eng, n)
    pool.state.copy_(torch.from_numpy(si[:, :, :, None, :].copy()).cuda())
    yp = pool.push(FxpArray(np.stack(nxt), bits, exp))
    assert pool.last_path == _lib.PATH_STEP
    assert np.array_equal(yp.numpy(), np.stack([c[0] for c in cont]))
    assert np.array_equal(pool.state.cpu().numpy()[:, :, :, 0], np.stack([c[3] for c in cont]))


# ------------------------------------------------------------------------------------------------------------------
# 8. up to one tile the clip kernel and the step kernel are the same stages
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ds", (0.25, 1.0))
def test_one_tile_equals_the_step_kernel(ds):
    """The clip kernel is the step body's stages over tiles (one of them a shared function, the others a copy of the text);
    a clip of at most 32 frames is one tile, so Engine.clips and Engine.step(B=1, L=len, groups=1) on the same rows and
    carry must agree in every bit: y, the carry out and all 128 status words but word 2, the path code.  No oracle: one
    kernel is the other's reference, which is what keeps the two copies from drifting."""
    import torch
    from sparsernns_amd import _lib
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    lens = (1, 7, 32)
    parts = [_fx(qc, dims, L, seed=800 + L) for L in lens]
    clips, bits, exp = [p[0] for p in parts], parts[0][1], parts[0][2]
    rng = np.random.Generator(np.random.PCG64(14))
    states = rng.integers(-3000, 3000, (len(lens), dims["n_layers"], 2, dims["P"]), dtype=np.int64).astype(np.int32)
    assert states.any(axis=(1, 2, 3)).all()
    y, sout, st = _launch(eng, _pad(clips, 32), lens, bits, exp, states)
    assert (st[:, 2] == _lib.PATH_CLIP).all()
    for e, (L, clip) in enumerate(zip(lens, clips)):
        carry = torch.from_numpy(states[e][None, :, :, None, :].copy()).cuda()   # (1, nl, 2, B = 1, P), replaced in place
        ys = eng.step(torch.from_numpy(np.ascontiguousarray(clip[None, None])).cuda(), carry, None, 1, L, 1, bits, exp, lane=1)
        torch.cuda.synchronize()
        sts = eng.lane_status(1, 1).cpu().numpy()[:_lib.STATUS_WORDS].copy()
        assert sts[2] == _lib.PATH_STEP, (ds, L, sts[:8])
        assert np.array_equal(ys.cpu().numpy()[0, 0], y[e, :L]), (ds, L, "y")
        assert np.array_equal(carry.cpu().numpy()[0, :, :, 0], sout[e]), (ds, L, "carry")
        keep = np.arange(_lib.STATUS_WORDS) != 2
        assert np.array_equal(sts[keep], st[e][keep]), (ds, L, sts[:32], st[e][:32])


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
    assert need == n * 2 * Lmax * eng.H * 2
    assert lib.s5fxp_clips_workspace_bytes(eng._h, 0, Lmax) == 0 and lib.s5fxp_clips_workspace_bytes(eng._h, n, 0) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = lambda h=eng._h, n=n, Lmax=Lmax, lens=lens.data_ptr(), wsb=need, bits=16: lib.s5fxp_model_clips(
        h, x.data_ptr(), bits, 14, n, Lmax, lens, y.data_ptr(), None, None, ws.data_ptr(), wsb, st.data_ptr(), s)
    assert call(n=0) == _lib.S5FXP_EBADARG and call(Lmax=0) == _lib.S5FXP_EBADARG and call(lens=None) == _lib.S5FXP_EBADARG
    assert call(wsb=need - 1) == _lib.S5FXP_EBADARG and call(bits=0) == _lib.S5FXP_EBADARG and call(bits=33) == _lib.S5FXP_EBADARG
    assert lib.s5fxp_model_clips_ok(eng._h, Lmax) == 1 and lib.s5fxp_model_clips_ok(eng._h, 0) == -1
    gen = Engine(model.export(), flags=_lib.MODEL_FORCE_GENERIC)
    assert lib.s5fxp_model_clips_ok(gen._h, Lmax) == 0 and call(h=gen._h) == _lib.S5FXP_EUNSUPPORTED
    assert call() == _lib.S5FXP_OK
    torch.cuda.synchronize()
    assert int(st[2].item()) == _lib.PATH_CLIP and int(st[_lib.STATUS_WORDS + 2].item()) == _lib.PATH_CLIP
