"""The batch forward at stated exponents (include/s5fxp.h s5fxp_model_forward_at / _f32 / _i16): every sequence of
the batch gets bit for bit the rows s5fxp_model_clips_at gives that sequence alone at the same exponents, and with a carry the
rows and the carry of the pinned step kernel, chunk for chunk.  Every GPU comparison is np.array_equal.

References: the NumPy oracle with its maxima forced (tests/pinned_helpers.py) for the three models of tests/test_pinned_exps.py
-- synth.make_model(calib_L=256) at dim_scale 0.25 and 0.5 and the scale-plus-bias contract model, built here the same way --
and the library's own entries at the same exponents (Engine.clips(exps=), SessionPool(exps=), the unpinned forward) for the
rest, dim_scale 0.75 and 1.0 included.
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
ORACLE_MODELS = ("s025", "s05", "bnsb")
SCALES = {"s025": 0.25, "s05": 0.5, "s075": 0.75, "s10": 1.0}
B_MAIN, L_MAIN = 3, 130          # two 64-frame tiles and a 2-frame tail; five 32-frame tiles / 32-step time blocks and a tail
SEEDS = (140, 141, 142)
SENTINEL = -123456789
NEW_SYMBOLS = ("s5fxp_model_forward_at", "s5fxp_model_forward_at_f32", "s5fxp_model_forward_at_i16")


# ------------------------------------------------------------------------------------------------------------------
# models, sequences and their oracle results (computed once, shared, never written to)
# ------------------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self, om, qc, dims, product):
        self.om, self.qc, self.dims, self._product = om, qc, dims, product
        self.bits, self.exp = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]

    def engine(self):
        return self._product().engine()

    def export(self):
        return self._product().export()


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
    md, qc, dims = synth.make_model(dim_scale=SCALES[key], calib_L=256)

    @functools.lru_cache(maxsize=None)
    def product():
        from sparsernns_amd.fxpmodel import build_regression_model
        return build_regression_model(md, qc, dims["n_layers"])

    return _Model(O.RegressionModel(md, qc, dims["n_layers"]), qc, dims, product)


def _seq(m: _Model, L: int, seed: int):
    x = synth.make_input(1, max(L, 1), m.dims["d_in"], seed=seed)
    return O.from_fp(x, m.bits, m.exp, True, O.FLOOR).data[0, :L]


@functools.lru_cache(maxsize=None)
def _batch(key, B=B_MAIN, L=L_MAIN):
    m = _model(key)
    return np.stack([_seq(m, L, SEEDS[b % len(SEEDS)] + 10 * (b // len(SEEDS)) + L) for b in range(B)])


@functools.lru_cache(maxsize=None)
def _natural(key, B=B_MAIN, L=L_MAIN):
    """Per sequence (y, carry, exponents) of the unforced oracle from a zero carry."""
    m = _model(key)
    out = []
    for s in _batch(key, B, L):
        y, carry, nat = PH.oracle_run(m.om, s, m.bits, m.exp)
        out.append((y, carry, nat[0]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _common(key, B=B_MAIN, L=L_MAIN):
    """The element-wise minimum of the sequences' own exponents, and that set 2 tighter per op where legal."""
    m = _model(key)
    emin = np.min([n[2] for n in _natural(key, B, L)], axis=0).astype(np.int32)
    return emin, PH.shifted(m.om, emin, +2)


@functools.lru_cache(maxsize=None)
def _forced(key, which, B=B_MAIN, L=L_MAIN):
    """Per sequence (y, carry) of the oracle at the common exponents (which = 0) / the tighter ones (1), from a zero carry."""
    m = _model(key)
    return tuple(PH.oracle_run(m.om, s, m.bits, m.exp, exps=_common(key, B, L)[which])[:2] for s in _batch(key, B, L))


def _exps_words(st, nl):
    return st[..., 8:8 + 8 * nl].reshape(st.shape[:-1] + (nl, 8))[..., :5]


def _host_exps(exps):
    return None if exps is None else np.ascontiguousarray(np.asarray(exps, dtype=np.int32))


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
    assert "a pinned batch is a clip list" not in hdr


def test_null_arguments_are_refused_without_a_device():
    """What can be said without a model (creating one needs a device; the model's own refusals are
    test_refusals_come_in_the_stated_order_and_touch_nothing): the namesake's argument check comes first, so a null model is
    S5FXP_EBADARG with and without exps, with and without traces."""
    from sparsernns_amd import _lib

    lib, E = _lib.lib, _lib.S5FXP_EBADARG
    buf = (C.c_int32 * 4096)()
    p = C.addressof(buf)
    tr = (_lib.LayerTrace * 1)()
    for entry in (lib.s5fxp_model_forward_at, lib.s5fxp_model_forward_at_f32, lib.s5fxp_model_forward_at_i16):
        for exps in (p, None):
            for t in (None, tr):
                assert entry(None, p, 16, 14, 1, 1, p, p, 1 << 20, p, t, None, exps, None) == E


@pytest.mark.parametrize("key", ORACLE_MODELS)
def test_the_tighter_set_changes_the_oracle_s_output(key):
    """The premise of the test that catches a missed clamp, on the oracle alone: at the set two tighter the forced output
    differs from the natural one on at least one sequence, and forcing a sequence's own exponents changes nothing."""
    m = _model(key)
    emin, tight = _common(key)
    assert PH.shifts_ok(m.om, emin) and PH.shifts_ok(m.om, tight) and not np.array_equal(emin, tight)
    assert any(not np.array_equal(f[0], n[0]) for f, n in zip(_forced(key, 1), _natural(key)))
    s, (y, carry, nat) = _batch(key)[0], _natural(key)[0]
    yf, cf, _ = PH.oracle_run(m.om, s, m.bits, m.exp, exps=nat)
    assert np.array_equal(yf, y) and np.array_equal(cf, carry)


# ------------------------------------------------------------------------------------------------------------------
# GPU: one raw launcher on caller-owned memory
# ------------------------------------------------------------------------------------------------------------------
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fwd_raw(eng, x, bits, exp, exps, state_in=None, carry=False, flags=0, groups=1, ws_fill=None, allreduce=None,
             traces=None, want_rc=0, pinned=True, B=None, ws_bytes=None):
    """One call of s5fxp_model_forward[_at][_f32|_i16] (by x's dtype; pinned=False: the namesake).  x: (groups * B, L, d_in).
    carry: state_out is wanted (state_in None: from zeros).  Returns y, carry out (or None), status (groups, 128) as numpy."""
    import torch
    from sparsernns_amd import _lib
    GB, L = x.shape[0], x.shape[1]
    B = GB // groups if B is None else B
    tdt = {np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32, np.dtype(np.int16): torch.int16}[x.dtype]
    suffix = {torch.int32: "", torch.float32: "_f32", torch.int16: "_i16"}[tdt]
    xd = _t(x)
    y = torch.full((GB, L, eng.d_out), SENTINEL, dtype=torch.int32, device="cuda")
    if tdt == torch.int16:
        y = torch.full((GB, L, eng.d_out), -12345, dtype=torch.int16, device="cuda")
    st = torch.full((groups, _lib.STATUS_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    per = getattr(_lib.lib, "s5fxp_workspace_bytes" + suffix)(eng._h, max(B, 1), max(L, 1))
    ws = torch.zeros(groups * per, dtype=torch.uint8, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    opts = _lib.ForwardOpts()
    opts.flags, opts.groups = int(flags), int(groups)
    shape = (eng.n_layers, 2, B, eng.P) if groups == 1 else (groups, eng.n_layers, 2, B, eng.P)
    sin = sout = None
    if carry or state_in is not None:
        sin = _t(state_in) if state_in is not None else torch.zeros(shape, dtype=torch.int32, device="cuda")
        sout = torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")
        opts.state_in, opts.state_out = sin.data_ptr(), sout.data_ptr()
    if allreduce is not None:
        opts.allreduce = allreduce
    e = _host_exps(exps)
    name = "s5fxp_model_forward" + ("_at" if pinned else "") + suffix
    tail = (e.ctypes.data if e is not None else None,) if pinned else ()
    rc = getattr(_lib.lib, name)(eng._h, xd.data_ptr(), bits, exp, B, L, y.data_ptr(), ws.data_ptr(),
                                 ws.numel() if ws_bytes is None else ws_bytes, st.data_ptr(), traces, C.byref(opts), *tail,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == want_rc, (name, rc)
    yy = y.view(torch.float32) if tdt == torch.float32 else y
    return yy.cpu().numpy(), None if sout is None else sout.cpu().numpy(), st.cpu().numpy()


def _clips_ref(eng, m, x, exps, state=None):
    """Engine.clips(exps=) on every sequence of x (n, L, d_in) alone: y (n, L, d_out), carry out (n, n_layers, 2, P)."""
    import torch
    n, L = x.shape[:2]
    ys, cs = [], []
    for e in range(n):
        so = torch.empty((1, eng.n_layers, 2, eng.P), dtype=torch.int32, device="cuda")
        si = None if state is None else _t(state[e:e + 1])
        y = eng.clips(_t(x[e:e + 1]), torch.tensor([L], dtype=torch.int32, device="cuda"), state=si, state_out=so,
                      x_bits=m.bits, x_exp=m.exp, exps=exps)
        torch.cuda.synchronize()
        ys.append(y.cpu().numpy()[0])
        cs.append(so.cpu().numpy()[0])
    return np.stack(ys), np.stack(cs)


def _status_ok(st, eng, exps, mx, defer=False):
    from sparsernns_amd import _lib
    words = np.where(mx >= 0, exps, 0)
    for g in range(st.shape[0]):
        assert (st[g, 0] & ~_lib.ST_WIDE_STATE) == 0, st[g, 0]   # never NEGSHIFT / NEGEXP; no REDO, no WIDE_INPUT here
        assert st[g, 2] == _lib.PATH_FUSED
        assert np.array_equal(_exps_words(st[g], eng.n_layers), words)


# ------------------------------------------------------------------------------------------------------------------
# GPU 1: against the forced oracle
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", [0, 1], ids=["minimum", "two_tighter"])
@pytest.mark.parametrize("key", ORACLE_MODELS)
def test_batch_equals_the_forced_oracle(key, which):
    m = _model(key)
    eng = m.engine()
    exps, ref, mx = _common(key)[which], _forced(key, which), PH.exp_max(m.om)
    eng.check_exps(exps)
    if which:   # not vacuous: the oracle itself gives other values than on the sequences' own exponents
        assert any(not np.array_equal(r[0], n[0]) for r, n in zip(ref, _natural(key)))
    x = _batch(key)
    # without a carry (live-state compaction where the model has it) and with one (every state slot)
    y0, _, st0 = _fwd_raw(eng, x, m.bits, m.exp, exps)
    y1, c1, st1 = _fwd_raw(eng, x, m.bits, m.exp, exps, carry=True)
    for b in range(B_MAIN):
        assert np.array_equal(y0[b], ref[b][0]), b
        assert np.array_equal(y1[b], ref[b][0]), b
        assert np.array_equal(c1[:, :, b], ref[b][1]), b
    _status_ok(st0, eng, exps, mx)
    _status_ok(st1, eng, exps, mx)


@gpu
@pytest.mark.parametrize("BL", [(1, 1), (2, 64), (2, 65)], ids=lambda v: f"B{v[0]}_L{v[1]}")
def test_edge_lengths_equal_the_forced_oracle(BL):
    B, L = BL
    m = _model("s05")
    eng = m.engine()
    exps, ref = _common("s05", B, L)[0], _forced("s05", 0, B, L)
    y, c, st = _fwd_raw(eng, _batch("s05", B, L), m.bits, m.exp, exps, carry=True)
    y0, _, _ = _fwd_raw(eng, _batch("s05", B, L), m.bits, m.exp, exps)
    for b in range(B):
        assert np.array_equal(y[b], ref[b][0]) and np.array_equal(c[:, :, b], ref[b][1]) and np.array_equal(y0[b], ref[b][0]), b
    _status_ok(st, eng, exps, PH.exp_max(m.om))


# ------------------------------------------------------------------------------------------------------------------
# GPU 2: against the library's own entries at the same exponents
# ------------------------------------------------------------------------------------------------------------------
def _lib_exps(m, eng, x, delta=0):
    """Exponents for a batch without oracle time: the minimum of what the unpinned clip launch reports per sequence."""
    import torch
    n, L = x.shape[:2]
    eng.clips(_t(x), torch.full((n,), L, dtype=torch.int32, device="cuda"), x_bits=m.bits, x_exp=m.exp)
    torch.cuda.synchronize()
    from sparsernns_amd import _lib
    st = eng.lane_status(0, n).cpu().numpy()[:n * _lib.STATUS_WORDS].reshape(n, _lib.STATUS_WORDS)
    e = _exps_words(st, eng.n_layers).min(axis=0).astype(np.int32)
    return PH.shifted(m.om, e, delta) if delta else e


@gpu
@pytest.mark.parametrize("key", ["s075", "s10"])
def test_every_sequence_equals_the_clip_launch(key):
    """dim_scale 0.75 and 1.0 (H = 144 / 192) against Engine.clips(exps=), itself held to the oracle by tests/test_pinned_exps.py
    at the smaller shapes: rows and carry, at the common exponents and one tighter."""
    m = _model(key)
    eng = m.engine()
    x = _batch(key, 2, 70)
    for delta in (0, 1):
        exps = _lib_exps(m, eng, x, delta)
        yr, cr = _clips_ref(eng, m, x, exps)
        y0, _, _ = _fwd_raw(eng, x, m.bits, m.exp, exps)
        y1, c1, st = _fwd_raw(eng, x, m.bits, m.exp, exps, carry=True)
        assert np.array_equal(y0, yr) and np.array_equal(y1, yr), delta
        assert np.array_equal(c1.transpose(2, 0, 1, 3), cr), delta
        _status_ok(st, eng, exps, PH.exp_max(m.om))


@gpu
@pytest.mark.parametrize("key", ["s025", "s05"])
def test_chunks_with_the_carry_and_a_session_pool_give_the_whole_signal(key):
    import torch
    from sparsernns_amd.fxparray import FxpArray
    m = _model(key)
    eng = m.engine()
    exps, x = _common(key)[0], _batch(key)
    yw, cw, _ = _fwd_raw(eng, x, m.bits, m.exp, exps, carry=True)
    ya, ca, _ = _fwd_raw(eng, x[:, :70], m.bits, m.exp, exps, carry=True)
    yb, cb, _ = _fwd_raw(eng, x[:, 70:], m.bits, m.exp, exps, state_in=ca)
    assert np.array_equal(np.concatenate([ya, yb], axis=1), yw) and np.array_equal(cb, cw)
    # Engine.forward_chunk(exps=) is the same two calls
    fx = lambda a: FxpArray(_t(a), m.bits, m.exp, True)
    y70, s70 = eng.forward_chunk(fx(x[:, :70]), exps=exps)
    y60, s130 = eng.forward_chunk(fx(x[:, 70:]), s70, exps=exps)
    assert np.array_equal(torch.cat([y70.data, y60.data], dim=1).cpu().numpy(), yw) and np.array_equal(s130.cpu().numpy(), cw)
    # a pool of B_MAIN sessions fed [32, 32, 32, 32, 2]
    pool, parts, at = eng.pool(B_MAIN, exps=exps), [], 0
    for c in (32, 32, 32, 32, 2):
        parts.append(pool.push(fx(x[:, at:at + c])).data.clone())
        at += c
    assert np.array_equal(torch.cat(parts, dim=1).cpu().numpy(), yw)
    assert np.array_equal(pool.state.cpu().numpy()[:, :, :, 0].transpose(1, 2, 0, 3), cw)


@gpu
@pytest.mark.parametrize("key", ["s05", "s10"])
def test_flags_give_the_same_bits_where_no_redo_is_raised(key):
    from sparsernns_amd import _lib
    m = _model(key)
    eng = m.engine()
    x = _batch(key, 2, 70)
    exps = _common(key, 2, 70)[0] if key == "s05" else _lib_exps(m, eng, x)
    runs = {}
    for name, fl in (("default", 0), ("defer", _lib.FWD_DEFER_REDO), ("exact", _lib.FWD_EXACT),
                     ("defer_no_pair", _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR)):
        for carry in (False, True):
            runs[name, carry] = _fwd_raw(eng, x, m.bits, m.exp, exps, carry=carry, flags=fl)
    y, c = runs["exact", True][:2]
    for (name, carry), (yy, cc, st) in runs.items():
        assert not (st[0, 0] & _lib.ST_REDO), name
        assert np.array_equal(yy, y), (name, carry)
        if carry:
            assert np.array_equal(cc, c), name
        assert np.array_equal(_exps_words(st[0], eng.n_layers), np.where(PH.exp_max(m.om) >= 0, exps, 0))
    # the rung words are the namesake's
    for fl in (0, _lib.FWD_DEFER_REDO, _lib.FWD_EXACT):
        sn = _fwd_raw(eng, x, m.bits, m.exp, None, flags=fl, pinned=False)[2]
        sp = _fwd_raw(eng, x, m.bits, m.exp, exps, flags=fl)[2]
        w = lambda s: s[0, 8:8 + 8 * eng.n_layers].reshape(eng.n_layers, 8)[:, 5:]
        assert np.array_equal(w(sn), w(sp)), fl


@gpu
def test_a_planted_wide_carry_raises_redo_or_runs_exact():
    from sparsernns_amd import _lib
    m = _model("s05")
    eng = m.engine()
    exps, x = _common("s05")[0], _batch("s05")[:2, :70]
    state = np.zeros((eng.n_layers, 2, 2, eng.P), dtype=np.int32)
    state[0, 0, 1, :] = 40000      # beyond every fast rung's bound (<= 32767), in sequence 1 of layer 0
    state[1, 1, 0, 3] = -40000
    yr, cr = _clips_ref(eng, m, x, exps, state=state.transpose(2, 0, 1, 3))
    yd, cd, sd = _fwd_raw(eng, x, m.bits, m.exp, exps, state_in=state)
    assert np.array_equal(yd, yr) and np.array_equal(cd.transpose(2, 0, 1, 3), cr) and not (sd[0, 0] & _lib.ST_REDO)
    ye, ce, _ = _fwd_raw(eng, x, m.bits, m.exp, exps, state_in=state, flags=_lib.FWD_EXACT)
    assert np.array_equal(ye, yr) and np.array_equal(ce, cd)
    _, _, sr = _fwd_raw(eng, x, m.bits, m.exp, exps, state_in=state, flags=_lib.FWD_DEFER_REDO)
    assert sr[0, 0] & _lib.ST_REDO
    # what the namesake does on the same carry
    _, _, sn = _fwd_raw(eng, x, m.bits, m.exp, None, state_in=state, flags=_lib.FWD_DEFER_REDO, pinned=False)
    _, _, sn0 = _fwd_raw(eng, x, m.bits, m.exp, None, state_in=state, pinned=False)
    assert (sn[0, 0] & _lib.ST_REDO) and sn[0, 0] == sr[0, 0] and sn0[0, 0] == sd[0, 0]
    # Engine.forward_chunk(exps=) climbs the ladder to the same result
    from sparsernns_amd.fxparray import FxpArray
    yl, sl = eng.forward_chunk(FxpArray(_t(x), m.bits, m.exp, True), _t(state), exps=exps)
    assert np.array_equal(yl.data.cpu().numpy(), yr) and np.array_equal(sl.cpu().numpy(), cd)


@gpu
def test_two_groups_equal_two_single_calls():
    import torch
    from sparsernns_amd.fxparray import FxpArray
    m = _model("s05")
    eng = m.engine()
    exps = _common("s05")[1]
    x = np.concatenate([_batch("s05")[:2], _batch("s05", 2, L_MAIN + 1)[:, :L_MAIN]])   # groups of B = 2
    yg, cg, sg = _fwd_raw(eng, x, m.bits, m.exp, exps, carry=True, groups=2)
    for g in range(2):
        y1, c1, s1 = _fwd_raw(eng, x[2 * g:2 * g + 2], m.bits, m.exp, exps, carry=True)
        assert np.array_equal(yg[2 * g:2 * g + 2], y1) and np.array_equal(cg[g], c1) and np.array_equal(sg[g], s1[0]), g
    yb = eng.forward_batches(FxpArray(_t(x), m.bits, m.exp, True), 2, exps=exps)
    assert np.array_equal(yb.data.cpu().numpy(), yg)


@gpu
def test_float_and_int16_boundaries():
    """_f32 is from_fp -> the int entry -> to_float, _i16 the int entry on the same integers in 2 bytes: the conversions of
    tests/test_forward_boundaries.py."""
    import torch
    m = _model("s05")
    eng = m.engine()
    exps, x = _common("s05")[1], _batch("s05")
    y, c, st = _fwd_raw(eng, x, m.bits, m.exp, exps, carry=True)
    xf = np.ldexp(x.astype(np.float32), -m.exp).astype(np.float32)   # floats whose FLOOR at m.exp is exactly x
    yf, cf, sf = _fwd_raw(eng, xf, m.bits, m.exp, exps, carry=True)
    assert np.array_equal(yf.view(np.int32), np.ldexp(y.astype(np.float32), -eng.out_exp).astype(np.float32).view(np.int32))
    assert np.array_equal(cf, c) and np.array_equal(sf, st)
    assert eng.out_bits <= 16 and np.abs(x).max() < 32768
    yi, ci, si = _fwd_raw(eng, x.astype(np.int16), m.bits, m.exp, exps, carry=True)
    assert yi.dtype == np.int16 and np.array_equal(yi.astype(np.int32), y) and np.array_equal(ci, c) and np.array_equal(si, st)
    # the Python routes
    assert torch.equal(eng.forward_float(_t(xf), m.bits, m.exp, exps=exps), _t(yf))
    assert torch.equal(eng.forward_int16(_t(x.astype(np.int16)), m.bits, m.exp, exps=exps), _t(yi))


# ------------------------------------------------------------------------------------------------------------------
# GPU 3: what the pinned path no longer does
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_allreduce_hook_is_never_called():
    from sparsernns_amd import _lib
    m = _model("s05")
    eng = m.engine()
    exps, x = _common("s05")[0], _batch("s05")
    calls = []

    def hook(ctx, vals, n, stream):
        calls.append(n)
        return 0

    fn = _lib.ALLREDUCE_FN(hook)
    y, _, st = _fwd_raw(eng, x, m.bits, m.exp, exps, allreduce=fn)
    assert calls == [] and np.array_equal(y, _fwd_raw(eng, x, m.bits, m.exp, exps)[0])
    # the namesake with the same hook calls it: the hook is wired
    _fwd_raw(eng, x, m.bits, m.exp, None, allreduce=fn, pinned=False)
    assert len(calls) > 0


@gpu
@pytest.mark.parametrize("key", ["s05", "bnsb", "s025"])
def test_results_do_not_depend_on_what_the_workspace_held(key):
    m = _model(key)
    eng = m.engine()
    exps, x = _common(key)[1], _batch(key)
    runs = [_fwd_raw(eng, x, m.bits, m.exp, exps, carry=True, ws_fill=f) for f in (0x00, 0x7F, 0x80, 0xFF)]
    runs += [_fwd_raw(eng, x, m.bits, m.exp, exps, ws_fill=f, flags=1) for f in (0x00, 0xFF)]
    ref = _forced(key, 1)
    from sparsernns_amd import _lib
    for i, (y, c, st) in enumerate(runs):
        if st[0, 0] & _lib.ST_REDO:   # a deferred forward whose states left the fast rung's range: its rows are the caller's to repeat
            assert i >= 4
            continue
        for b in range(B_MAIN):
            assert np.array_equal(y[b], ref[b][0]), (i, b)
    for y, c, st in runs[1:4]:
        assert np.array_equal(y, runs[0][0]) and np.array_equal(c, runs[0][1]) and np.array_equal(st, runs[0][2])
    assert np.array_equal(runs[4][2], runs[5][2])


@gpu
def test_own_exponents_reproduce_the_unpinned_forward():
    for key in ORACLE_MODELS:
        m = _model(key)
        eng = m.engine()
        for b in range(2):
            x = _batch(key)[b:b + 1]
            for carry in (False, True):
                y0, c0, s0 = _fwd_raw(eng, x, m.bits, m.exp, None, carry=carry, pinned=False)
                own = _exps_words(s0[0], eng.n_layers)
                assert np.array_equal(own, np.where(PH.exp_max(m.om) >= 0, _natural(key)[b][2], 0))
                y1, c1, s1 = _fwd_raw(eng, x, m.bits, m.exp, own, carry=carry)
                assert np.array_equal(y1, y0) and np.array_equal(s1, s0), (key, b, carry)
                if carry:
                    assert np.array_equal(c1, c0)


# ------------------------------------------------------------------------------------------------------------------
# GPU 4: refusals, before the device is touched and in the stated order
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_come_in_the_stated_order_and_touch_nothing(monkeypatch):
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine
    m = _model("s025")
    eng = m.engine()
    good, mx = _common("s025")[0], PH.exp_max(m.om)
    above, neg = good.copy(), good.copy()
    above[1, 4] = mx[1, 4] + 1
    neg[0, 0], neg[0, 1] = 0, mx[0, 1]   # mul(invsq_var): right shift 0 + invsq_var_exp - 15 < 0
    assert not PH.shifts_ok(m.om, neg)
    generic = Engine(m.export(), flags=_lib.MODEL_FORCE_GENERIC)
    monkeypatch.setenv("S5FXP_NO_BN_EXT", "1")   # read once, at creation: a fused model on the four-reduction route
    four = Engine(m.export())
    monkeypatch.delenv("S5FXP_NO_BN_EXT")
    assert _lib.lib.s5fxp_model_is_fast(four._h) and not _lib.lib.s5fxp_model_is_fast(generic._h)
    tr = (_lib.LayerTrace * eng.n_layers)()
    x = _batch("s025")[:1, :33]
    E = _lib
    cases = [
        # (engine, exps, kwargs, code)
        (eng, None, {}, E.S5FXP_EBADARG),                       # 2. a null exps
        (eng, None, {"traces": tr}, E.S5FXP_EBADARG),           # ... ahead of the traces
        (eng, good, {"traces": tr}, E.S5FXP_EUNSUPPORTED),      # 3. traces
        (eng, above, {"traces": tr}, E.S5FXP_EUNSUPPORTED),     # ... ahead of the exponents' own check
        (eng, above, {}, E.S5FXP_EBADARG),                      # 4. s5fxp_model_exps_check
        (eng, neg, {}, E.S5FXP_ENEGSHIFT),
        (generic, good, {}, E.S5FXP_EUNSUPPORTED),
        (eng, above, {"ws_bytes": 16}, E.S5FXP_EWORKSPACE),     # 1. the namesake's checks come first
        (eng, None, {"ws_bytes": 16}, E.S5FXP_EWORKSPACE),
    ]
    for en, exps, kw, rc in cases:
        for xx in (x, np.ldexp(x.astype(np.float32), -m.exp).astype(np.float32), x.astype(np.int16)):
            y, c, st = _fwd_raw(en, xx, m.bits, m.exp, exps, carry=True, want_rc=rc, **kw)
            assert np.all(y.view(np.int32 if y.dtype != np.int16 else np.int16) == (SENTINEL if y.dtype != np.int16 else -12345))
            assert np.all(c == SENTINEL) and np.all(st == SENTINEL), (rc, kw)
    # a fused model on the four-reduction route is served, through the two-plane residual pass: the same bits
    xb = _batch("s025")
    for ex in _common("s025"):
        for carry in (False, True):
            a, b = _fwd_raw(four, xb, m.bits, m.exp, ex, carry=carry), _fwd_raw(eng, xb, m.bits, m.exp, ex, carry=carry)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and (not carry or np.array_equal(a[1], b[1]))
    # the same through Python
    import torch
    from sparsernns_amd.fxparray import FxpArray
    fx = FxpArray(_t(x), m.bits, m.exp, True)
    with pytest.raises(ValueError):
        eng.forward(fx, exps=above)
    with pytest.raises(NotImplementedError):
        eng.forward(fx, traces=True, exps=good)
    with pytest.raises(NotImplementedError):
        generic.forward(fx, exps=good)
    assert torch.equal(eng.forward(fx, exps=None).data, eng.forward(fx).data)


# ------------------------------------------------------------------------------------------------------------------
# GPU 5: the Python routes above the engine
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_runner_and_audio_routes_at_stated_exponents():
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd.engine import InflightRunner
    from sparsernns_amd.fxpmodel import build_regression_model
    m = _model("s05")
    eng = m.engine()
    exps, x = _common("s05")[0], _batch("s05")
    want = _fwd_raw(eng, x, m.bits, m.exp, exps)[0]
    runner = InflightRunner(eng, depth=2)
    xd = _t(x)
    ys = [torch.empty((B_MAIN, L_MAIN, eng.d_out), dtype=torch.int32, device="cuda") for _ in range(3)]
    for y in ys:
        runner.submit(xd, m.bits, m.exp, y, B_MAIN, L_MAIN, exps=exps)
    runner.drain()
    assert all(np.array_equal(y.cpu().numpy(), want) for y in ys)
    # audio: two clips of equal length as a batch at stated exponents == the clip route at the same exponents
    md, qc, dims = synth.make_model(0.5, calib_L=128)
    model, ib, ie = build_regression_model(md, qc, dims["n_layers"]), qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    noisy = (0.02 * torch.randn(2, 128 * 40, generator=torch.Generator().manual_seed(5))).cuda()
    clean = torch.zeros_like(noisy)
    ae = model.engine()
    q = lambda r: torch.floor(r * float(1 << ie)).clamp(-(1 << (ib - 1)), (1 << (ib - 1)) - 1).to(torch.int32).contiguous()
    from sparsernns_amd.fxparray import FxpArray
    cal = ae.calibrate_exps([FxpArray(q(r), ib, ie, True) for r in audio.stft_mag(noisy)])
    per_clip = audio.denoise_clips(model, ib, ie, [noisy[0], noisy[1]], exps=cal)
    for boundary in ("float32", "int16"):
        cleaned, _, xr, mask = audio.denoise_fused(model, ib, ie, noisy, boundary=boundary, exps=cal)
        for e in range(2):
            assert torch.equal(cleaned[e], per_clip[e][0]), (boundary, e)
            if boundary == "float32":
                assert torch.equal(mask[e], per_clip[e][3]) and torch.equal(xr[e], per_clip[e][2])
    # validate_fused(exps=) scores that mask: the batch scorer on the mask of denoise_fused(exps=)
    mask = audio.denoise_fused(model, ib, ie, noisy, exps=cal)[3]
    v_f, v_m = audio.validate_fused(model, ib, ie, noisy, clean, exps=cal), audio.score_fused(noisy, clean, mask, 0.001)[:2]
    assert torch.equal(v_f[0], v_m[0]) and torch.equal(v_f[1], v_m[1])
    # exps=None is today's call
    assert torch.equal(audio.denoise_fused(model, ib, ie, noisy, exps=None)[0], audio.denoise_fused(model, ib, ie, noisy)[0])
