"""Stated exponents (include/s5fxp.h s5fxp_model_step_at / _step_ragged_at / _clips_at): the step, ragged step
and clip launches with the five compute_best exponents of every layer given by the caller.  Every GPU comparison is
np.array_equal; the reference of every value is the NumPy oracle with MAX_EXCHANGE forcing each op's maximum to a float
whose intbits gives the stated exponent (tests/pinned_helpers.py).

Models: synth.make_model(calib_L=256) at dim_scale 0.25 and 0.5 (no BatchNorm scale or bias: three ops per layer) and one
contract model with scale and bias, so that all five ops run.  tests/contract_models.py holds no model with a BatchNorm scale
or bias among its families, so the third model is built with that module's own machinery (its ``_calibrate`` with an
``edit_float`` that adds both to the float tree before calibration, wrapped in its ``Case``): the module is imported, not edited.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import contract_models as CM
import pinned_helpers as PH
from oracle import fxp_oracle as O
from sparsernns_amd import synth

gpu = pytest.mark.gpu
MODELS = ("s025", "s05", "bnsb")
LENS = (0, 1, 31, 32, 33, 70)
CHUNKINGS = ([1] * 70, [7] * 10, [32, 32, 6], [5, 32, 1, 32])
SENTINEL = -123456789
NEW_SYMBOLS = ("s5fxp_model_exp_max", "s5fxp_model_exps_check", "s5fxp_model_step_at", "s5fxp_model_step_at_f32",
               "s5fxp_model_step_ragged_at", "s5fxp_model_step_ragged_at_f32", "s5fxp_model_clips_at", "s5fxp_model_clips_at_f32")


# ------------------------------------------------------------------------------------------------------------------
# models, clips and their oracle results (computed once, shared, never written to)
# ------------------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self, om, qc, dims, product):
        self.om, self.qc, self.dims, self._product = om, qc, dims, product
        self.bits, self.exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]

    def product(self):
        return self._product()

    def engine(self):
        return self.product().engine()


@functools.lru_cache(maxsize=None)
def _model(key) -> _Model:
    if key == "bnsb":
        dims = CM._dims(0.5)

        def add_scale_bias(md):
            rng = np.random.Generator(np.random.PCG64(77))
            for l in CM._layers(md, dims):
                H = dims["H"]
                l["norm"]["scale"] = (rng.uniform(0.5, 1.5, H) * rng.choice([-1.0, 1.0], H, p=[0.1, 0.9])).astype(np.float32)
                l["norm"]["bias"] = (0.1 * rng.standard_normal(H)).astype(np.float32)

        md, qc = CM._calibrate(dims, CM.FULL, edit_float=add_scale_bias)
        case = CM.Case("F1_bnsb_ds0.5", md, qc, dims, family="F1")
        return _Model(case.numpy_oracle(), qc, dims, case.model)
    md, qc, dims = synth.make_model(dim_scale={"s025": 0.25, "s05": 0.5}[key], calib_L=256)

    @functools.lru_cache(maxsize=None)
    def product():
        from sparsernns_amd.fxpmodel import build_regression_model
        return build_regression_model(md, qc, dims["n_layers"])

    return _Model(O.RegressionModel(md, qc, dims["n_layers"]), qc, dims, product)


def _clip(m: _Model, L: int, seed: int):
    x = synth.make_input(1, max(L, 1), m.dims["d_in"], seed=seed)
    return O.from_fp(x, m.bits, m.exp, True, O.FLOOR).data[0, :L]


@functools.lru_cache(maxsize=None)
def _clips(key):
    m = _model(key)
    return tuple(_clip(m, L, 40 + i) for i, L in enumerate(LENS))


@functools.lru_cache(maxsize=None)
def _natural(key):
    """Per clip (y, carry, exponents) of the unforced oracle from a zero carry."""
    m = _model(key)
    out = []
    for c in _clips(key):
        y, carry, nat = PH.oracle_run(m.om, c, m.bits, m.exp)
        out.append((y, carry, nat[0] if nat else None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _common(key):
    """The element-wise minimum of the clips' own exponents, and that set 2 tighter per op where legal."""
    m = _model(key)
    emin = np.min([n[2] for n in _natural(key) if n[2] is not None], axis=0).astype(np.int32)
    return emin, PH.shifted(m.om, emin, +2)


@functools.lru_cache(maxsize=None)
def _forced(key, which):
    """Per clip (y, carry) of the oracle at the common exponents (which = 0) / the tighter ones (1), from a zero carry."""
    m = _model(key)
    return tuple(PH.oracle_run(m.om, c, m.bits, m.exp, exps=_common(key)[which])[:2] for c in _clips(key))


def _pad(clips, Lmax, dtype=np.int32):
    x = np.zeros((len(clips), Lmax, clips[0].shape[-1]), dtype=dtype)
    for e, c in enumerate(clips):
        x[e, :len(c)] = c
    return x


def _exps_words(st, nl):
    return st[..., 8:8 + 8 * nl].reshape(st.shape[:-1] + (nl, 8))[..., :5]


# ------------------------------------------------------------------------------------------------------------------
# not GPU
# ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    import os
    import re
    from sparsernns_amd import _lib

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s5fxp.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert _lib.lib.s5fxp_version() == 115


def test_null_arguments_are_refused_without_a_device():
    from sparsernns_amd import _lib

    lib, E = _lib.lib, _lib.S5FXP_EBADARG
    buf = (C.c_int32 * 4096)()
    p = C.addressof(buf)
    assert lib.s5fxp_model_exps_check(None, p) == E
    assert lib.s5fxp_model_exps_check(None, None) == E
    assert lib.s5fxp_model_exp_max(None, 0, 0) == -1
    for exps in (p, None):   # a null model with and without exps; the model comes first, so both are EBADARG
        for entry in (lib.s5fxp_model_step_at, lib.s5fxp_model_step_at_f32):
            assert entry(None, p, 16, 14, 1, 1, 1, p, None, None, p, exps, None) == E
        for entry in (lib.s5fxp_model_step_ragged_at, lib.s5fxp_model_step_ragged_at_f32):
            assert entry(None, p, 16, 14, 1, 1, 1, p, p, p, 1, p, exps, None) == E
        for entry in (lib.s5fxp_model_clips_at, lib.s5fxp_model_clips_at_f32):
            assert entry(None, p, 16, 14, 1, 4, p, p, None, None, p, 16384, p, exps, None) == E


@pytest.mark.parametrize("key", MODELS)
def test_oracle_forcing_the_natural_exponents_reproduces_the_unforced_oracle(key):
    m = _model(key)
    for c, (y, carry, nat) in zip(_clips(key), _natural(key)):
        if nat is None:
            continue
        assert PH.shifts_ok(m.om, nat)
        yf, cf, _ = PH.oracle_run(m.om, c, m.bits, m.exp, exps=nat)
        assert np.array_equal(yf, y) and np.array_equal(cf, carry)


@pytest.mark.parametrize("delta", [+1, -1])
def test_oracle_forced_exponents_are_chunk_invariant(delta):
    """The premise, on the CPU at dim_scale 0.25: at stated exponents -- the 70-frame clip's own, moved one up / one down per
    op inside the legal range -- the chunkings give the whole-clip forward's y and carry bit for bit."""
    m = _model("s025")
    clip, nat = _clips("s025")[-1], _natural("s025")[-1][2]
    e = PH.shifted(m.om, nat, delta)
    assert not np.array_equal(e, nat)
    yw, cw, _ = PH.oracle_run(m.om, clip, m.bits, m.exp, exps=e)
    for ch in ([1] * 70, [7] * 10, [32, 32, 6]):
        yc, cc, _ = PH.oracle_run(m.om, clip, m.bits, m.exp, exps=e, chunks=ch)
        assert np.array_equal(yc, yw) and np.array_equal(cc, cw), ch
    # and the gap this closes: each chunk on its own exponents does not give the whole-clip forward
    yn, _, _ = PH.oracle_run(m.om, clip, m.bits, m.exp, chunks=[7] * 10)
    assert not np.array_equal(yn, _natural("s025")[-1][0])


# ------------------------------------------------------------------------------------------------------------------
# GPU: launch helpers (raw entries, caller-owned memory)
# ------------------------------------------------------------------------------------------------------------------
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host_exps(exps):
    return None if exps is None else np.ascontiguousarray(np.asarray(exps, dtype=np.int32))


def _clips_raw(eng, x, lens, bits, exp, exps, state=None, fill=None, want_rc=0):
    """One launch of s5fxp_model_clips[_at][_f32] on caller memory.  exps None: the unpinned entry.  fill: the byte every output,
    the status and the workspace hold before the launch (default: int32 sentinels in y and the carry out).
    Returns y, carry out, status (n, 128) as numpy."""
    import torch
    from sparsernns_amd import _lib
    n, Lmax = x.shape[0], x.shape[1]
    f32 = x.dtype == np.float32
    xd, ld = _t(x), _t(np.asarray(lens, dtype=np.int32))
    y = torch.full((n, Lmax, eng.d_out), SENTINEL, dtype=torch.int32, device="cuda")
    sout = torch.full((n, eng.n_layers, 2, eng.P), SENTINEL, dtype=torch.int32, device="cuda")
    st = torch.full((n, _lib.STATUS_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    ws = torch.zeros(_lib.lib.s5fxp_clips_workspace_bytes(eng._h, n, Lmax), dtype=torch.uint8, device="cuda")
    if fill is not None:
        for t in (y, sout, st, ws):
            t.view(torch.uint8).fill_(fill)
    sin = _t(state) if state is not None else None
    e = _host_exps(exps)
    name = "s5fxp_model_clips" + ("" if e is None else "_at") + ("_f32" if f32 else "")
    tail = () if e is None else (e.ctypes.data,)
    rc = getattr(_lib.lib, name)(eng._h, xd.data_ptr(), bits, exp, n, Lmax, ld.data_ptr(), y.data_ptr(),
                                 sin.data_ptr() if sin is not None else None, sout.data_ptr(), ws.data_ptr(), ws.numel(),
                                 st.data_ptr(), *tail, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == want_rc, (name, rc)
    yy = y.view(torch.float32) if f32 else y
    return yy.cpu().numpy(), sout.cpu().numpy(), st.cpu().numpy()


def _step_raw(eng, x, bits, exp, exps, state, fill=None, want_rc=0):
    """One launch of s5fxp_model_step[_at][_f32]: x (G, B, L, d_in), state (G, nl, 2, B, P) or None -> y, carry out, status."""
    import torch
    from sparsernns_amd import _lib
    G, B, L = x.shape[:3]
    f32 = x.dtype == np.float32
    xd = _t(x)
    y = torch.full((G, B, L, eng.d_out), SENTINEL, dtype=torch.int32, device="cuda")
    sout = torch.full((G, eng.n_layers, 2, B, eng.P), SENTINEL, dtype=torch.int32, device="cuda")
    st = torch.full((G, _lib.STATUS_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    if fill is not None:
        for t in (y, sout, st):
            t.view(torch.uint8).fill_(fill)
    sin = _t(state) if state is not None else None
    e = _host_exps(exps)
    name = "s5fxp_model_step" + ("" if e is None else "_at") + ("_f32" if f32 else "")
    tail = () if e is None else (e.ctypes.data,)
    rc = getattr(_lib.lib, name)(eng._h, xd.data_ptr(), bits, exp, G, B, L, y.data_ptr(), sin.data_ptr() if sin is not None else None,
                                 sout.data_ptr(), st.data_ptr(), *tail, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == want_rc, (name, rc)
    yy = y.view(torch.float32) if f32 else y
    return yy.cpu().numpy(), sout.cpu().numpy(), st.cpu().numpy()


def _to_float(y, out_exp):
    return np.ldexp(y.astype(np.float32), -out_exp).astype(np.float32)


def _as_float_input(clips, exp):
    """Float rows whose fxp_from_fp FLOOR at `exp` is exactly the int rows (a 16-bit integer over 2^exp is exact in float32)."""
    return [np.ldexp(c.astype(np.float32), -exp).astype(np.float32) for c in clips]


# ------------------------------------------------------------------------------------------------------------------
# GPU 1: own exponents reproduce the unpinned forward
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("with_state", [False, True], ids=["zero_carry", "carry"])
@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
@pytest.mark.parametrize("key", MODELS)
def test_own_exponents_reproduce_the_unpinned_forward(key, f32, with_state):
    m = _model(key)
    eng, nl = m.engine(), m.dims["n_layers"]
    assert eng.clips_ok(max(LENS)) and np.array_equal(eng.exp_max(), PH.exp_max(m.om))
    clips = list(_clips(key))
    rows = _as_float_input(clips, m.exp) if f32 else clips
    x = _pad(rows, max(LENS), np.float32 if f32 else np.int32)
    state = None
    if with_state:
        rng = np.random.default_rng(3)
        state = rng.integers(-3000, 3000, size=(len(clips), nl, 2, eng.P)).astype(np.int32)
    y0, c0, s0 = _clips_raw(eng, x, LENS, m.bits, m.exp, None, state)
    if not with_state and not f32:   # the unpinned launch is the oracle's, exponent words included
        for e, (yn, cn, nat) in enumerate(_natural(key)):
            assert np.array_equal(y0[e, :LENS[e]], yn)
            if nat is not None:
                assert np.array_equal(_exps_words(s0[e], nl), nat) and np.array_equal(c0[e], cn)
    some = _exps_words(s0[-1], nl)
    for e, L in enumerate(LENS):
        own = _exps_words(s0[e], nl) if L else some   # the empty clip chose nothing: any legal set leaves it alone
        y1, c1, s1 = _clips_raw(eng, x[e:e + 1], [L], m.bits, m.exp, own, None if state is None else state[e:e + 1])
        assert np.array_equal(y1[0].view(np.int32), y0[e].view(np.int32)), (e, L)
        assert np.array_equal(c1[0], c0[e]) and np.array_equal(s1[0], s0[e]), (e, L)


# ------------------------------------------------------------------------------------------------------------------
# GPU 2: common exponents, against the oracle
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", [0, 1], ids=["minimum", "two_tighter"])
@pytest.mark.parametrize("key", MODELS)
def test_common_exponents_equal_the_forced_oracle(key, which):
    m = _model(key)
    eng, nl = m.engine(), m.dims["n_layers"]
    exps = _common(key)[which]
    eng.check_exps(exps)
    ref = _forced(key, which)
    if which:   # not vacuous: at the tighter set the oracle itself gives other values than on the clips' own exponents
        assert not np.array_equal(exps, _common(key)[0])
        assert any(not np.array_equal(r[0], n[0]) for r, n in zip(ref, _natural(key)))
    clips = list(_clips(key))
    Lmax = max(LENS) + 3
    x = _pad(clips, Lmax)
    y, carry, st = _clips_raw(eng, x, LENS, m.bits, m.exp, exps)
    words = np.where(PH.exp_max(m.om) >= 0, exps, 0)
    for e, L in enumerate(LENS):
        assert np.array_equal(y[e, :L], ref[e][0]), (e, L)
        assert np.all(y[e, L:] == SENTINEL), (e, L)   # padding rows, and every row of the empty clip
        assert np.array_equal(carry[e], ref[e][1]), (e, L)
        assert (st[e, 0] & ~4) == 0 and st[e, 1] == eng.out_exp and st[e, 2] == 4
        assert np.array_equal(_exps_words(st[e], nl), words if L else np.zeros_like(words)), (e, L)
    # the f32 entry is from_fp -> the int entry -> to_float
    xf = _pad(_as_float_input(clips, m.exp), Lmax, np.float32)
    yf, cf, sf = _clips_raw(eng, xf, LENS, m.bits, m.exp, exps)
    for e, L in enumerate(LENS):
        assert np.array_equal(yf[e, :L], _to_float(y[e, :L], eng.out_exp)), (e, L)
        assert np.all(yf[e, L:].view(np.int32) == SENTINEL)
    assert np.array_equal(cf, carry) and np.array_equal(sf, st)


# ------------------------------------------------------------------------------------------------------------------
# GPU 3: chunk invariance on the device
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", [0, 1], ids=["minimum", "two_tighter"])
@pytest.mark.parametrize("key", MODELS)
def test_steps_over_any_chunking_equal_the_whole_clip(key, which):
    m = _model(key)
    eng, nl, P = m.engine(), m.dims["n_layers"], m.dims["P"]
    exps = _common(key)[which]
    a, b = _clips(key)[-1], _clip(m, 70, 91)
    yw, cw, _ = _clips_raw(eng, np.stack([a, b]), [70, 70], m.bits, m.exp, exps)
    assert np.array_equal(yw[0], _forced(key, which)[-1][0])
    for ch in CHUNKINGS:
        state, ys, at = np.zeros((1, nl, 2, 1, P), dtype=np.int32), [], 0
        for c in ch:
            y, state, st = _step_raw(eng, a[None, None, at:at + c], m.bits, m.exp, exps, state)
            assert (st[0, 0] & ~4) == 0 and st[0, 2] == 3
            ys.append(y[0, 0])
            at += c
        assert np.array_equal(np.concatenate(ys), yw[0]), ch
        assert np.array_equal(state[0, :, :, 0], cw[0]), ch
    # one B = 2 group in steps of L = 16 (and the last 6 frames)
    both = np.stack([a, b])
    state, ys = np.zeros((1, nl, 2, 2, P), dtype=np.int32), []
    for at in range(0, 70, 16):
        y, state, _ = _step_raw(eng, both[None, :, at:at + 16], m.bits, m.exp, exps, state)
        ys.append(y[0])
    assert np.array_equal(np.concatenate(ys, axis=1), yw)
    assert np.array_equal(state[0].transpose(2, 0, 1, 3), cw)


@gpu
@pytest.mark.parametrize("f32", [False, True], ids=["i32", "f32"])
@pytest.mark.parametrize("key", MODELS)
def test_ragged_step_with_a_mixed_descriptor_array(key, f32):
    """A FRESH entry on a slot full of rubbish, a rows = 0 entry, two entries at different phases of their signals, and a slot
    no entry names: rows and carries are those of the clip launch on the signals' prefixes."""
    import torch
    from sparsernns_amd import _lib
    m = _model(key)
    eng, nl, P = m.engine(), m.dims["n_layers"], m.dims["P"]
    exps = _common(key)[0]
    A, B_, C_ = _clip(m, 40, 61), _clip(m, 40, 62), _clip(m, 40, 63)
    Lmax = 7
    prefixes = [A[:5], B_[:10], B_[:17], C_[:33], C_[:36]]
    yp, cp, _ = _clips_raw(eng, _pad(prefixes, 36), [5, 10, 17, 33, 36], m.bits, m.exp, exps)
    # entries: slot 2 FRESH (A, 5 rows), slot 0 idle (0 rows), slot 3 (B at frame 10, 7 rows), slot 4 (C at frame 33, 3 rows)
    rng = np.random.default_rng(8)
    state = rng.integers(-2 ** 31, 2 ** 31 - 1, size=(5, nl, 2, 1, P), dtype=np.int64).astype(np.int32)
    state[3, :, :, 0], state[4, :, :, 0] = cp[1], cp[3]
    before = state.copy()
    rows = [A[:5], A[:0], B_[10:17], C_[33:36]]
    desc = np.zeros((4, 8), dtype=np.int32)
    desc[:, 0], desc[:, 1], desc[0, 2] = [2, 0, 3, 4], [5, 0, 7, 3], _lib.PUSH_FRESH
    assert _lib.lib.s5fxp_push_desc_check(desc.ctypes.data, 4, 5, Lmax, 0, 0) == 0
    x = _pad(_as_float_input(rows, m.exp) if f32 else rows, Lmax, np.float32 if f32 else np.int32)
    xd, dd, sd = _t(x), _t(desc), _t(state)
    y = torch.full((4, Lmax, eng.d_out), SENTINEL, dtype=torch.int32, device="cuda")
    st = torch.full((4, _lib.STATUS_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    e = _host_exps(exps)
    entry = _lib.lib.s5fxp_model_step_ragged_at_f32 if f32 else _lib.lib.s5fxp_model_step_ragged_at
    rc = entry(eng._h, xd.data_ptr(), m.bits, m.exp, 4, 1, Lmax, y.data_ptr(), dd.data_ptr(), sd.data_ptr(), 5, st.data_ptr(),
               e.ctypes.data, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    y, st, after = y.cpu().numpy(), st.cpu().numpy(), sd.cpu().numpy()
    conv = (lambda v: _to_float(v, eng.out_exp).view(np.int32)) if f32 else (lambda v: v)
    for ent, (want, nrows) in enumerate(((yp[0, :5], 5), (yp[0, :0], 0), (yp[2, 10:17], 7), (yp[4, 33:36], 3))):
        assert np.array_equal(y[ent, :nrows], conv(want)), ent
        assert np.all(y[ent, nrows:] == SENTINEL), ent
    assert np.array_equal(after[2, :, :, 0], cp[0])                     # FRESH: from zeros, whatever the slot held
    assert np.array_equal(after[0], before[0])                          # rows = 0, not FRESH: untouched
    assert np.array_equal(after[1], before[1])                          # unnamed: keeps its bytes
    assert np.array_equal(after[3, :, :, 0], cp[2]) and np.array_equal(after[4, :, :, 0], cp[4])
    words = np.where(PH.exp_max(m.om) >= 0, exps, 0)
    for ent, nrows in enumerate((5, 0, 7, 3)):
        assert (st[ent, 0] & ~4) == 0 and st[ent, 2] == 3
        assert np.array_equal(_exps_words(st[ent], nl), words if nrows else np.zeros_like(words))


# ------------------------------------------------------------------------------------------------------------------
# GPU 4: refusals before the device is touched
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_every_output_poisoned():
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine
    m = _model("s025")
    eng, nl = m.engine(), m.dims["n_layers"]
    good, mx = _common("s025")[0], PH.exp_max(m.om)
    above, below, neg = good.copy(), good.copy(), good.copy()
    above[1, 4] = mx[1, 4] + 1
    below[2, 0] = -1
    neg[0, 0], neg[0, 1] = 0, mx[0, 1]   # mul(invsq_var): right shift 0 + invsq_var_exp - 15 < 0
    assert not PH.shifts_ok(m.om, neg) and PH.shifts_ok(m.om, good)
    generic = Engine(m.product().export(), flags=_lib.MODEL_FORCE_GENERIC)
    cases = [(eng, above, _lib.S5FXP_EBADARG), (eng, below, _lib.S5FXP_EBADARG), (eng, neg, _lib.S5FXP_ENEGSHIFT),
             (generic, good, _lib.S5FXP_EUNSUPPORTED)]
    clip = _clips("s025")[2]
    for en, exps, rc in cases:
        eh = _host_exps(exps)
        assert _lib.lib.s5fxp_model_exps_check(en._h, eh.ctypes.data) == rc
        for x in (clip[None], _as_float_input([clip], m.exp)[0][None]):
            y, c, st = _clips_raw(en, x, [len(clip)], m.bits, m.exp, exps, want_rc=rc)
            assert np.all(y.view(np.int32) == SENTINEL) and np.all(c == SENTINEL) and np.all(st == SENTINEL)
            y, c, st = _step_raw(en, x[:, None], m.bits, m.exp, exps, None, want_rc=rc)
            assert np.all(y.view(np.int32) == SENTINEL) and np.all(c == SENTINEL) and np.all(st == SENTINEL)
            y, c, st = _ragged_refused(en, x, m, exps, rc)
            assert np.all(y == SENTINEL) and np.all(c == SENTINEL) and np.all(st == SENTINEL)
    with pytest.raises(ValueError):
        eng.check_exps(above)
    with pytest.raises(ValueError):
        eng.check_exps(neg)
    with pytest.raises(NotImplementedError):
        generic.check_exps(good)
    assert np.array_equal(generic.exp_max(), mx)
    assert _lib.lib.s5fxp_model_exp_max(eng._h, nl, 0) == -1 and _lib.lib.s5fxp_model_exp_max(eng._h, 0, 5) == -1


def _ragged_refused(en, x, m, exps, rc):
    import torch
    from sparsernns_amd import _lib
    L = x.shape[1]
    desc = np.zeros((1, 8), dtype=np.int32)
    desc[0, 1] = L
    xd, dd = _t(x), _t(desc)
    y = torch.full((1, L, en.d_out), SENTINEL, dtype=torch.int32, device="cuda")
    state = torch.full((1, en.n_layers, 2, 1, en.P), SENTINEL, dtype=torch.int32, device="cuda")
    st = torch.full((1, _lib.STATUS_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    entry = _lib.lib.s5fxp_model_step_ragged_at_f32 if x.dtype == np.float32 else _lib.lib.s5fxp_model_step_ragged_at
    eh = _host_exps(exps)
    got = entry(en._h, xd.data_ptr(), m.bits, m.exp, 1, 1, L, y.data_ptr(), dd.data_ptr(), state.data_ptr(), 1, st.data_ptr(),
                eh.ctypes.data, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert got == rc, got
    return y.cpu().numpy(), state.cpu().numpy(), st.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------
# GPU 5: caller memory
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", ["s025", "bnsb"])
def test_outputs_do_not_depend_on_what_caller_memory_held(key):
    m = _model(key)
    eng = m.engine()
    exps = _common(key)[1]
    clips = list(_clips(key))
    x = _pad(clips, max(LENS))
    runs = [_clips_raw(eng, x, LENS, m.bits, m.exp, exps, fill=f) for f in (0x7F, 0xFF)]
    ref = _forced(key, 1)
    for (y, c, st), f in zip(runs, (0x7F, 0xFF)):
        poison = np.frombuffer(bytes([f]) * 4, dtype=np.int32)[0]
        for e, L in enumerate(LENS):
            assert np.array_equal(y[e, :L], ref[e][0]) and np.all(y[e, L:] == poison)
            assert np.array_equal(c[e], ref[e][1])
    assert np.array_equal(runs[0][2], runs[1][2])   # status written completely: no word keeps its fill
    a = clips[-1][None, None, :32]
    steps = [_step_raw(eng, a, m.bits, m.exp, exps, None, fill=f) for f in (0x7F, 0xFF)]
    for got in steps:
        assert np.array_equal(got[0][0, 0], ref[-1][0][:32])
    for u, v in zip(steps[0], steps[1]):
        assert np.array_equal(u, v)


# ------------------------------------------------------------------------------------------------------------------
# GPU 6: Python
# ------------------------------------------------------------------------------------------------------------------
def _fxp(m, clip):
    import torch
    from sparsernns_amd.fxparray import FxpArray
    return FxpArray(torch.from_numpy(np.ascontiguousarray(clip)).cuda(), m.bits, m.exp, True)


@gpu
@pytest.mark.parametrize("key", ["s025", "bnsb"])
def test_calibrate_exps(key):
    from sparsernns_amd import _lib
    m = _model(key)
    eng, nl = m.engine(), m.dims["n_layers"]
    three = [_fxp(m, c) for c in (_clips(key)[5], _clips(key)[2], _clips(key)[0], _clips(key)[4])]   # one of them empty
    unpinned = [y.data.cpu().numpy() for y in eng.forward_clips(three)]
    st = eng.lane_status(0, 4).cpu().numpy()[:4 * _lib.STATUS_WORDS].reshape(4, _lib.STATUS_WORDS)
    want = _exps_words(st[[0, 1, 3]], nl).min(axis=0)
    cal = eng.calibrate_exps(three)
    assert np.array_equal(cal, want)
    assert np.array_equal(eng.calibrate_exps(three, headroom=1), np.where(PH.exp_max(m.om) >= 0, np.maximum(want - 1, 0), 0))
    assert np.array_equal(eng.calibrate_exps(three, headroom=99), np.zeros_like(want))
    # one clip: its own exponents, so the pinned forward is the unpinned one (GPU 1 through the Python route)
    one = eng.calibrate_exps(three[:1])
    assert np.array_equal(one, _natural(key)[5][2])
    got = eng.forward_clips(three[:1], exps=one)[0]
    assert np.array_equal(got.data.cpu().numpy(), unpinned[0]) and (got.bits, got.exp) == (eng.out_bits, eng.out_exp)
    # exps=None is today's call
    again = [y.data.cpu().numpy() for y in eng.forward_clips(three, exps=None)]
    assert all(np.array_equal(u, v) for u, v in zip(unpinned, again))
    y_raw, _, _ = _clips_raw(eng, _pad([c.data.cpu().numpy() for c in three], 70), [70, 31, 0, 33], m.bits, m.exp, None)
    assert all(np.array_equal(y_raw[e, :len(u)], u) for e, u in enumerate(unpinned))


@gpu
@pytest.mark.parametrize("key", ["s025", "s05"])
def test_session_pool_at_stated_exponents(key):
    import torch
    m = _model(key)
    eng = m.engine()
    exps = _common(key)[0]
    a, b = _clips(key)[-1], _clip(m, 70, 91)
    x = torch.from_numpy(np.stack([a, b])).cuda()
    from sparsernns_amd.fxparray import FxpArray
    fx = lambda t: FxpArray(t.contiguous(), m.bits, m.exp, True)
    whole = eng.pool(2, exps=exps)
    y70 = whole.push(fx(x)).data.clone()
    by_hand = eng.pool(2, exps=exps)
    parts = [by_hand.push(fx(x[:, s:e])).data.clone() for s, e in ((0, 32), (32, 64), (64, 70))]
    assert torch.equal(y70, torch.cat(parts, dim=1)) and torch.equal(whole.state, by_hand.state)
    yw, cw, _ = _clips_raw(eng, np.stack([a, b]), [70, 70], m.bits, m.exp, exps)
    assert np.array_equal(y70.cpu().numpy(), yw) and np.array_equal(whole.state.cpu().numpy()[:, :, :, 0], cw)
    assert list(whole.frames) == [70, 70]
    # the ragged push of the same 70 rows (split the same way), a float push, and an unchecked push
    ragged = eng.pool(3, exps=exps)
    yr = ragged.push_ragged([2, 0], fx(x), [70, 40], fresh=[2, 0]).data
    assert torch.equal(yr[0], y70[0]) and torch.equal(yr[1, :40], y70[1, :40])
    assert torch.equal(ragged.state[2], whole.state[0]) and list(ragged.frames) == [40, 0, 70]
    lazy = eng.pool(2, exps=exps)
    assert torch.equal(lazy.push(fx(x), check=False).data, y70)
    lazy.check()
    # exps=None: the pool as it was -- each chunk its own batch
    old, new = eng.pool(2), eng.pool(2, exps=None)
    assert torch.equal(old.push(fx(x[:, :20])).data, new.push(fx(x[:, :20])).data) and torch.equal(old.state, new.state)
    with pytest.raises(ValueError):
        bad = exps.copy()
        bad[0, 0] = -1
        eng.pool(1, exps=bad)


@gpu
@pytest.mark.parametrize("dim_scale", [0.25, 0.5])
def test_stream_denoiser_at_stated_exponents(dim_scale):
    """70 hops in groups of 1 and of 5 give the same audio, and that audio is denoise_clips([signal], exps=) bit for bit.  Which
    samples are comparable: all of them, the rule of tests/test_stream_denoise.py -- the pushes' outputs and finish(), joined,
    are the m * 128 samples of the signal, as many as the batch inverse returns for a signal of whole hops."""
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd.fxpmodel import build_regression_model
    md, qc, dims = synth.make_model(dim_scale, calib_L=128)
    model, ib, ie = build_regression_model(md, qc, dims["n_layers"]), qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    HOP, hops = 128, 70
    noisy = (0.02 * torch.randn(1, HOP * hops, generator=torch.Generator().manual_seed(5))).cuda()
    x = audio.stft_mag(noisy)
    eng = model.engine()
    exps = eng.calibrate_exps([_from_float(x[0], ib, ie)])

    def stream(group, ex):
        d, outs = audio.StreamDenoiser(model, 1, exps=ex), []
        for at in range(0, hops, group):
            outs.append(d.push(noisy[:, at * HOP:(at + group) * HOP]).clone())
        outs.append(d.finish().clone())
        return torch.cat(outs, dim=1)

    one, five = stream(1, exps), stream(5, exps)
    assert tuple(one.shape) == (1, HOP * hops) and torch.equal(one, five)
    cleaned, _, xc, mask = audio.denoise_clips(model, ib, ie, [noisy[0]], exps=exps)[0]
    assert torch.equal(xc, x[0]) and torch.equal(cleaned, one[0])
    # the session form, two slots at different phases
    sd = audio.SessionDenoiser(model, 2, exps=exps)
    outs, at = [], 0
    for c in [3, 32, 30, 5]:
        out, n_out = sd.push([1], noisy[:, at * HOP:(at + c) * HOP])
        outs.append(out[0, :int(n_out[0]) * HOP].clone())
        at += c
    out, n_out = sd.finish([1])
    outs.append(out[0, :int(n_out[0]) * HOP].clone())
    assert torch.equal(torch.cat(outs), one[0])
    # exps=None: today's objects; and calibrated exponents with no headroom reproduce the unpinned whole-clip forward
    assert torch.equal(stream(5, None), _stream_plain(audio, model, noisy, HOP, hops, 5))
    plain = audio.denoise_clips(model, ib, ie, [noisy[0]])[0]
    assert torch.equal(plain[0], cleaned) and torch.equal(plain[3], mask)
    assert torch.equal(audio.denoise_clips(model, ib, ie, [noisy[0]], exps=None)[0][0], plain[0])
    clean = torch.zeros_like(noisy[0])
    v0, v1 = audio.validate_clips(model, ib, ie, [noisy[0]], [clean]), audio.validate_clips(model, ib, ie, [noisy[0]], [clean], exps=exps)
    assert torch.equal(v0[0], v1[0]) and torch.equal(v0[1], v1[1])


def _from_float(x, bits, exp):
    """fxp_from_fp FLOOR of device float rows, as an FxpArray: what the f32 entries do to them."""
    import torch
    from sparsernns_amd.fxparray import FxpArray
    q = torch.floor(x * float(1 << exp)).clamp(-(1 << (bits - 1)), (1 << (bits - 1)) - 1).to(torch.int32)
    return FxpArray(q.contiguous(), bits, exp, True)


def _stream_plain(audio, model, noisy, HOP, hops, group):
    import torch
    d, outs = audio.StreamDenoiser(model, 1), []
    for at in range(0, hops, group):
        outs.append(d.push(noisy[:, at * HOP:(at + group) * HOP]).clone())
    outs.append(d.finish().clone())
    return torch.cat(outs, dim=1)
