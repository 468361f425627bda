"""The one-launch streaming step (include/s5fxp.h s5fxp_model_step, csrc/s5fxp_step.hpp) and the pool of stream sessions
(engine.SessionPool).  Every comparison is np.array_equal against the C oracle (oracle/cref.py CModel.forward(..., state=...)) run
per group on the CPU; where noted also against the batch path (Engine.enqueue with state_in / state_out) on the GPU.

Status word [1]: the step writes the decoder's output exponent there, as include/s5fxp.h documents the word; it is compared with
the oracle's output exponent (the batch path's kernels leave that word at zero).
"""
import functools

import numpy as np
import pytest

import contract_models as CM
from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth

gpu = pytest.mark.gpu
SHAPES = (0.25, 0.5, 0.75, 1.0)
CHUNKS = ((1, 1), (1, 4), (4, 1), (3, 7), (2, 16), (1, 32), (32, 1))


# ------------------------------------------------------------------------------------------------------------------
# not GPU: the ABI surface
# ------------------------------------------------------------------------------------------------------------------
def test_step_symbols_and_argument_checks_without_a_device():
    import ctypes as C
    from sparsernns_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("s5fxp_model_step_ok", "s5fxp_model_step", "s5fxp_model_step_f32"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    lib = _lib.lib
    assert lib.s5fxp_version() >= 106
    assert _lib.PATH_STEP == 3 and _lib.STEP_MAX_ROWS == 32
    buf = (C.c_int32 * 512)()
    p = C.addressof(buf)
    assert lib.s5fxp_model_step(None, p, 16, 14, 1, 1, 1, p, None, None, p, None) == _lib.S5FXP_EBADARG
    assert lib.s5fxp_model_step_f32(None, p, 16, 14, 1, 1, 1, p, None, None, p, None) == _lib.S5FXP_EBADARG
    assert lib.s5fxp_model_step_ok(None, 1, 1) == -1


# ------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synth(ds, **kw):
    from sparsernns_amd.fxpmodel import build_regression_model
    cfg = dict(dim_scale=ds, calib_L=256)
    cfg.update(kw)
    md, qc, dims = synth.make_model(**cfg)
    model = build_regression_model(md, qc, dims["n_layers"])
    return model, qc, dims, cref.CModel(model.export())


def _fx(qc, dims, G, B, L, seed, scale=1.0):
    x = synth.make_input(G * B, L, dims["d_in"], seed=seed, scale=scale)
    f = O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    return f.data.reshape(G, B, L, dims["d_in"]), f.bits, f.exp


def _bn_word(export, i):
    norm = export["params"]["encoder"][f"layers_{i}"]["norm"]
    return 3 if "bias" in norm else (2 if "scale" in norm else 1)


def _oracle(cm, x, bits, exp, state):
    """Per-group oracle runs; `state` (G, nl, 2, B, P) is updated in place.  Returns y (G,B,L,d_out), y_exp, per-group
    [(pre_s5_exp, residadd_exp) per layer], max |state| seen in the traces."""
    ys, exps, smax, ye = [], [], 0, None
    for g in range(x.shape[0]):
        st = np.ascontiguousarray(state[g])
        y, _, ye, tr = cm.forward(x[g], bits, exp, trace=True, state=st)
        state[g] = st
        ys.append(y)
        exps.append([(int(t["pre_s5_exp"]), int(t["residadd_exp"])) for t in tr])
        smax = max([smax] + [int(np.abs(t[k].astype(np.int64)).max()) for t in tr for k in ("xs_re", "xs_im")])
    return np.stack(ys), ye, exps, smax


def _step(eng, x, bits, exp, state, lane=0, state_out=None):
    """x: np (G,B,L,d_in) int32 or float32; state: torch carry (in place unless state_out) or None.  Returns y, status (G,128)."""
    import torch
    from sparsernns_amd import _lib
    G, B, L = x.shape[:3]
    y = eng.step(torch.from_numpy(np.ascontiguousarray(x)).cuda(), state, None, B, L, G, bits, exp, state_out=state_out, lane=lane)
    torch.cuda.synchronize()
    st = eng.lane_status(lane, G).cpu().numpy()[:G * _lib.STATUS_WORDS].reshape(G, _lib.STATUS_WORDS).copy()
    return y.cpu().numpy(), st


def _batch(eng, x, bits, exp, state_np, lane=1):
    """The same chunk and carry through the batch path (one grouped, self-contained forward).  Returns y, carry out, status."""
    import torch
    from sparsernns_amd import _lib
    G, B, L = x.shape[:3]
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    y = torch.empty((G, B, L, eng.d_out), dtype=torch.int32, device="cuda")
    sin = torch.from_numpy(np.ascontiguousarray(state_np if G > 1 else state_np[0])).cuda()
    sout = torch.empty_like(sin)
    eng.enqueue(xd.view(G * B, L, -1), bits, exp, y.view(G * B, L, -1), B, L, flags=0, lane=lane, state_in=sin, state_out=sout, groups=G)
    torch.cuda.synchronize()
    st = eng.lane_status(lane, G).cpu().numpy()[:G * _lib.STATUS_WORDS].reshape(G, _lib.STATUS_WORDS).copy()
    return y.cpu().numpy(), sout.cpu().numpy().reshape(state_np.shape), st


def _check_chunk(eng, cm, export, x, bits, exp, carry, ref_state, tag, batch=True):
    """One carried chunk: step vs oracle (y, carry, exponents, status layout) and vs the batch path's status words."""
    from sparsernns_amd import _lib
    nl, P = eng.n_layers, eng.P
    before = ref_state.copy()
    ref, ye, exps, smax = _oracle(cm, x, bits, exp, ref_state)
    y, st = _step(eng, x, bits, exp, carry)
    assert np.array_equal(y, ref), (tag, int(np.count_nonzero(y != ref)))
    assert np.array_equal(carry.cpu().numpy(), ref_state), (tag, "carry")
    mask = _lib.ST_NEGSHIFT | _lib.ST_NEGEXP | _lib.ST_WIDE_INPUT
    for g in range(x.shape[0]):
        w = st[g]
        assert w[2] == _lib.PATH_STEP and w[1] == ye and not (w[0] & mask), (tag, g, w[:8])
        for i in range(nl):
            assert (w[8 + 8 * i + 5], w[8 + 8 * i + 6], w[8 + 8 * i + 7]) == (6, P, P), (tag, g, i)
            assert w[8 + 8 * i + _bn_word(export, i)] == exps[g][i][0] and w[8 + 8 * i + 4] == exps[g][i][1], (tag, g, i, w[8 + 8 * i:16 + 8 * i], exps[g][i])
    if batch:
        yb, sb, stb = _batch(eng, x, bits, exp, before)
        assert np.array_equal(yb, ref) and np.array_equal(sb, ref_state), (tag, "batch path")
        for g in range(x.shape[0]):
            assert stb[g][2] == _lib.PATH_FUSED
            assert (st[g][0] & mask) == (stb[g][0] & mask), (tag, g)
            for i in range(nl):
                assert list(st[g][8 + 8 * i:13 + 8 * i]) == list(stb[g][8 + 8 * i:13 + 8 * i]), (tag, g, i)
    return smax


def _zero_carry(eng, G, B):
    import torch
    shape = (G, eng.n_layers, 2, B, eng.P)
    return torch.zeros(shape, dtype=torch.int32, device="cuda"), np.zeros(shape, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------
# 1. shapes x chunks
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,L", CHUNKS)
@pytest.mark.parametrize("ds", SHAPES)
def test_step_matches_oracle_and_batch_path(ds, B, L):
    from sparsernns_amd import _lib
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    assert _lib.lib.s5fxp_model_step_ok(eng._h, B, L) == 1
    carry, ref_state = _zero_carry(eng, 1, B)
    for i in range(6):
        x, bits, exp = _fx(qc, dims, 1, B, L, seed=1000 * B + 10 * L + i)
        _check_chunk(eng, cm, model.export(), x, bits, exp, carry, ref_state, (ds, B, L, i))
    assert np.abs(ref_state).max() > 0


# ------------------------------------------------------------------------------------------------------------------
# 2. a stream of single frames through the pool
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_pool_of_single_frame_streams():
    from sparsernns_amd import SessionPool, _lib
    from sparsernns_amd.fxparray import FxpArray
    model, qc, dims, cm = _synth(0.5)
    eng = model.engine()
    S, T = 8, 200
    x, bits, exp = _fx(qc, dims, S, 1, T, seed=77)   # (S, 1, T, d_in): session s is sequence s
    pool = SessionPool(eng, S)
    sessions = [eng.stream(1) for _ in range(S)]
    ref_state = np.zeros((S, dims["n_layers"], 2, 1, dims["P"]), dtype=np.int32)
    for t in range(T):
        frame = np.ascontiguousarray(x[:, 0, t:t + 1, :])   # (S, 1, d_in)
        ref, ye, _, _ = _oracle(cm, frame[:, None], bits, exp, ref_state)
        y = pool.push(FxpArray(frame, bits, exp))
        assert pool.last_path == _lib.PATH_STEP
        got = y.numpy()
        assert y.exp == ye and np.array_equal(got, ref[:, 0]), t
        for s in range(S):
            ys = sessions[s].push(FxpArray(frame[s], bits, exp))
            assert np.array_equal(ys.numpy(), got[s]), (t, s)
    assert np.array_equal(pool.state.cpu().numpy(), ref_state)
    assert list(pool.frames) == [T] * S
    for s in range(S):
        assert np.array_equal(sessions[s].state.cpu().numpy(), ref_state[s])


# ------------------------------------------------------------------------------------------------------------------
# 3. groups are independent
# ------------------------------------------------------------------------------------------------------------------
SCALES = (0.0, 0.05, 1.0, 6.0)


def _scaled_groups(qc, dims, G, B, L, seed):
    parts = [_fx(qc, dims, 1, B, L, seed=seed + g, scale=SCALES[g % 4]) for g in range(G)]
    return np.concatenate([p[0] for p in parts]), parts[0][1], parts[0][2]


@gpu
@pytest.mark.parametrize("ds", SHAPES)
def test_groups_choose_their_own_exponents(ds):
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    for G in (1, 5, 256, 300):
        carry, ref_state = _zero_carry(eng, G, 1)
        for i in range(2):
            x, bits, exp = _scaled_groups(qc, dims, G, 1, 1, seed=50 * i)
            if G >= 4 and i == 0:   # on the CPU, before anything is compared: the groups really choose different exponents
                probe = ref_state.copy()
                e = _oracle(cm, x[:4], bits, exp, probe[:4])[2]
                assert e[2] != e[3] and e[2] not in (e[0], e[1]) and e[3] not in (e[0], e[1]), (ds, e)
            _check_chunk(eng, cm, model.export(), x, bits, exp, carry, ref_state, (ds, G, i))


@gpu
def test_pool_reset_touches_only_the_chosen_sessions():
    from sparsernns_amd import SessionPool
    from sparsernns_amd.fxparray import FxpArray
    model, qc, dims, cm = _synth(0.5)
    eng = model.engine()
    S = 5
    pool = SessionPool(eng, S)
    ref_state = np.zeros((S, dims["n_layers"], 2, 1, dims["P"]), dtype=np.int32)
    for i in range(3):
        x, bits, exp = _scaled_groups(qc, dims, S, 1, 3, seed=900 + 10 * i)
        ref = _oracle(cm, x, bits, exp, ref_state)[0]
        assert np.array_equal(pool.push(FxpArray(x[:, 0], bits, exp)).numpy(), ref[:, 0])
        if i == 1:
            pool.reset([1, 3])
            ref_state[[1, 3]] = 0
            got = pool.state.cpu().numpy()
            assert np.array_equal(got, ref_state) and np.abs(got[[0, 2, 4]]).max() > 0
            assert list(pool.frames) == [6, 0, 6, 0, 6]
    pool.reset()
    assert not pool.state.any().item() and not pool.frames.any()


# ------------------------------------------------------------------------------------------------------------------
# 4. wide states
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("how", ["planted_carry", "input_scale_6"])
@pytest.mark.parametrize("ds", SHAPES)
def test_states_beyond_16_bits(ds, how):
    """(a) a planted carry of 27-bit values; (b) an input scale of 6, which on these (2, 16) chunks takes the oracle's
    states beyond 16 bits at all four shapes (42 622 ... 97 569 on the first chunk)."""
    import torch
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    B, L = 2, 16
    carry, ref_state = _zero_carry(eng, 1, B)
    if how == "planted_carry":
        rng = np.random.Generator(np.random.PCG64(5))
        ref_state[:] = rng.integers(-2 ** 26, 2 ** 26, ref_state.shape, dtype=np.int64).astype(np.int32)
        carry.copy_(torch.from_numpy(ref_state))
    smax = 0
    for i in range(3):
        x, bits, exp = _fx(qc, dims, 1, B, L, seed=40 + i, scale=6.0 if how == "input_scale_6" else 1.0)
        probe = ref_state.copy()
        seen = _oracle(cm, x, bits, exp, probe)[3]
        if i == 0:   # on the oracle's traces, before the comparison: the case is not vacuous
            assert seen > (110000 if how == "planted_carry" else 32767), (ds, how, seen)
        smax = max(smax, _check_chunk(eng, cm, model.export(), x, bits, exp, carry, ref_state, (ds, how, i)))
    assert smax > 32767


# ------------------------------------------------------------------------------------------------------------------
# 5. / 6. contract models, padding rows
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(CM.BUILDERS))
def test_contract_models(name):
    from sparsernns_amd import _lib
    c = CM.case(name)
    eng, cm, export = c.engine(), c.c_oracle(), c.export()
    for (B, L) in ((1, 1), (3, 7), (1, 32)):
        assert _lib.lib.s5fxp_model_step_ok(eng._h, B, L) == 1, name
        for kind in CM.INPUTS:
            carry, ref_state = _zero_carry(eng, 1, B)
            for i in range(3):
                x, bits, exp = CM.input_for(c, kind, B, L, seed=3 * L + i)
                _check_chunk(eng, cm, export, x[None], bits, exp, carry, ref_state, (name, kind, B, L, i), batch=False)


@gpu
@pytest.mark.parametrize("name", ["F1_full_ds0.5", "F1_full_ds1.0", "F2_rails_ds1.0", "F3_dims257x272_ds0.5"])
def test_padding_rows_cannot_be_seen(name):
    """R = 31 and R = 1: a zero pad row would be a new minimum (pos_full) or maximum (neg_full) of every reduction."""
    c = CM.case(name)
    eng, cm, export = c.engine(), c.c_oracle(), c.export()
    for (B, L) in ((31, 1), (1, 31), (1, 1)):
        for kind in ("pos_full", "neg_full", "impulse_last"):
            carry, ref_state = _zero_carry(eng, 1, B)
            for i in range(2):
                x, bits, exp = CM.input_for(c, kind, B, L, seed=i)
                _check_chunk(eng, cm, export, x[None], bits, exp, carry, ref_state, (name, kind, B, L, i))


# ------------------------------------------------------------------------------------------------------------------
# 7. float entry, 8. in place
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ds", SHAPES)
def test_float_entry_is_from_fp_step_to_float(ds):
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import check, lib
    model, qc, dims, cm = _synth(ds)
    eng = model.engine()
    bits, exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    G, B, L = 3, 2, 5
    ca, _ = _zero_carry(eng, G, B)
    cb, _ = _zero_carry(eng, G, B)
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(3):
        xf = torch.from_numpy(synth.make_input(G * B, L, dims["d_in"], seed=60 + i, scale=(1.0, 6.0, 0.0)[i]).reshape(G, B, L, -1)).cuda()
        xi = torch.empty(xf.shape, dtype=torch.int32, device="cuda")
        check(lib.s5fxp_from_fp(xf.data_ptr(), xi.data_ptr(), xf.numel(), bits, exp, 0, stream))
        yi = eng.step(xi, ca, None, B, L, G, bits, exp, lane=0)
        want = torch.empty(yi.shape, dtype=torch.float32, device="cuda")
        check(lib.s5fxp_to_float(yi.data_ptr(), want.data_ptr(), yi.numel(), eng.out_exp, stream))
        got = eng.step(xf, cb, None, B, L, G, bits, exp, lane=1)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.cpu().numpy().view(np.int32)), (ds, i)
        assert torch.equal(ca, cb)
        n = G * _lib.STATUS_WORDS
        assert np.array_equal(eng.lane_status(0, G).cpu().numpy()[:n], eng.lane_status(1, G).cpu().numpy()[:n])
        ref = cm.forward(xi[1].cpu().numpy(), bits, exp)[0] if i == 0 else None
        if ref is not None:
            assert np.array_equal(yi[1].cpu().numpy(), ref)


@gpu
def test_carry_in_place_equals_separate_buffers():
    import torch
    model, qc, dims, cm = _synth(0.5)
    eng = model.engine()
    G, B, L = 7, 2, 5
    inplace, _ = _zero_carry(eng, G, B)
    cur, _ = _zero_carry(eng, G, B)
    for i in range(4):
        x, bits, exp = _fx(qc, dims, G, B, L, seed=20 + i)
        ya, sa = _step(eng, x, bits, exp, inplace, lane=0)
        nxt = torch.full_like(cur, -1)
        yb, sb = _step(eng, x, bits, exp, cur, lane=1, state_out=nxt)
        assert np.array_equal(ya, yb) and np.array_equal(sa, sb) and torch.equal(inplace, nxt), i
        cur = nxt
    assert inplace.any().item()


# ------------------------------------------------------------------------------------------------------------------
# 9. recipes
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("recipe", ["w4a8", "sparse"])
def test_recipes(recipe):
    kw = (dict(quantization="w4a8", bn_stats="random", input_scale=300.0) if recipe == "w4a8" else dict(sparsity=0.9))
    scale = 300.0 if recipe == "w4a8" else 1.0
    model, qc, dims, cm = _synth(0.5, **kw)
    eng = model.engine()
    for (B, L) in ((1, 1), (3, 7), (1, 32)):
        carry, ref_state = _zero_carry(eng, 1, B)
        for i in range(4):
            x, bits, exp = _fx(qc, dims, 1, B, L, seed=7 * L + i, scale=scale)
            _check_chunk(eng, cm, model.export(), x, bits, exp, carry, ref_state, (recipe, B, L, i))


# ------------------------------------------------------------------------------------------------------------------
# 10. fallbacks and arguments
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_arguments_on_a_real_handle():
    import torch
    from sparsernns_amd import _lib
    lib = _lib.lib
    model, qc, dims, cm = _synth(0.5)
    eng = model.engine()
    x = torch.zeros((33, dims["d_in"]), dtype=torch.int32, device="cuda")
    y = torch.zeros((33, dims["d_out"]), dtype=torch.int32, device="cuda")
    st = torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = lambda G, B, L, status=st.data_ptr(): lib.s5fxp_model_step(eng._h, x.data_ptr(), 16, 14, G, B, L, y.data_ptr(), None, None, status, s)
    assert call(0, 1, 1) == _lib.S5FXP_EBADARG
    assert call(1, 33, 1) == _lib.S5FXP_EBADARG and call(1, 3, 11) == _lib.S5FXP_EBADARG
    assert call(1, 1, 0) == _lib.S5FXP_EBADARG
    assert call(1, 1, 1, None) == _lib.S5FXP_EBADARG
    assert lib.s5fxp_model_step_ok(eng._h, 33, 1) == 0 and lib.s5fxp_model_step_ok(eng._h, 4, 8) == 1
    assert lib.s5fxp_model_step_ok(eng._h, 0, 1) == -1
    assert call(1, 1, 1) == _lib.S5FXP_OK
    torch.cuda.synchronize()
    assert int(st[2].item()) == _lib.PATH_STEP


@gpu
def test_pool_falls_back_where_the_step_does_not_apply():
    import torch
    from sparsernns_amd import SessionPool, _lib
    from sparsernns_amd.engine import Engine
    from sparsernns_amd.fxparray import FxpArray
    lib = _lib.lib
    model, qc, dims, cm = _synth(0.5)
    S = 3
    # a generic model: the entry refuses, the pool serves it through the generic engine
    gen = Engine(model.export(), flags=_lib.MODEL_FORCE_GENERIC)
    assert lib.s5fxp_model_step_ok(gen._h, 1, 1) == 0
    x, bits, exp = _fx(qc, dims, S, 1, 2, seed=1)
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty((S, 1, 2, dims["d_out"]), dtype=torch.int32, device="cuda")
    st = torch.zeros(S * _lib.STATUS_WORDS, dtype=torch.int32, device="cuda")
    assert lib.s5fxp_model_step(gen._h, xd.data_ptr(), bits, exp, S, 1, 2, yd.data_ptr(), None, None, st.data_ptr(),
                                torch.cuda.current_stream().cuda_stream) == _lib.S5FXP_EUNSUPPORTED
    pool = SessionPool(gen, S)
    ref_state = np.zeros((S, dims["n_layers"], 2, 1, dims["P"]), dtype=np.int32)
    for i in range(3):
        x, bits, exp = _fx(qc, dims, S, 1, 2, seed=10 + i)
        ref = _oracle(cm, x, bits, exp, ref_state)[0]
        assert np.array_equal(pool.push(FxpArray(x[:, 0], bits, exp)).numpy(), ref[:, 0])
        assert pool.last_path == _lib.PATH_GENERIC
        assert np.array_equal(pool.state.cpu().numpy(), ref_state)
    # a fused model: short chunks step, a 40-frame push goes to the batch path, then short chunks step again
    eng = model.engine()
    pool = SessionPool(eng, S)
    ref_state[:] = 0
    for i, L in enumerate((4, 40, 1, 32, 33)):
        x, bits, exp = _fx(qc, dims, S, 1, L, seed=30 + i)
        ref = _oracle(cm, x, bits, exp, ref_state)[0]
        y = pool.push(FxpArray(x[:, 0], bits, exp), check=(i != 2))
        assert np.array_equal(y.numpy(), ref[:, 0]), L
        assert pool.last_path == (_lib.PATH_STEP if L <= 32 else _lib.PATH_FUSED), L
        assert np.array_equal(pool.state.cpu().numpy(), ref_state), L
    pool.check()
    # float chunks: to_float of the same outputs
    xf = synth.make_input(S, 3, dims["d_in"], seed=99)
    fx = O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    ref = _oracle(cm, fx.data[:, None], fx.bits, fx.exp, ref_state)[0]
    yf = pool.push(torch.from_numpy(xf))
    assert yf.dtype == torch.float32 and np.array_equal(yf.cpu().numpy(), np.ldexp(ref[:, 0].astype(np.float32), -eng.out_exp))
    # an input whose values exceed its nominal 16 bits (legal in the reference, which only clips on a conversion): the step
    # reports ST_WIDE_INPUT, the pool serves the chunk through the generic engine
    x, bits, exp = _fx(qc, dims, S, 1, 2, seed=5)
    x = x * 9
    x[1] += 40000
    assert np.abs(x).max() > 32767
    before = pool.state.clone()
    _, stw = _step(eng, x, bits, exp, before.clone(), lane=2)
    assert stw[1][0] & _lib.ST_WIDE_INPUT and stw[1][2] == _lib.PATH_STEP
    ref = _oracle(cm, x, bits, exp, ref_state)[0]
    y = pool.push(FxpArray(x[:, 0], bits, exp))
    assert pool.last_path == _lib.PATH_GENERIC
    assert np.array_equal(y.numpy(), ref[:, 0]) and np.array_equal(pool.state.cpu().numpy(), ref_state)
