"""The int16 model boundary (include/s5fxp.h s5fxp_model_forward_i16): int16 rows in, int16 rows out.  It must give bit for bit
what s5fxp_model_forward gives for the sign-extended input -- the output (every int32 value inside int16), every status word,
every trace plane and the carry -- for every option the int entry takes, on the fused path (the int16 rows read and written
inside k_enc_ps / k_dec_ps) and on the generic one.  The int16 tensors are views one element into their buffers (2-byte
alignment only) and the output sits between sentinels, so a packed or over-wide store cannot pass.
"""
import ctypes as C

import numpy as np
import pytest

from sparsernns_amd import synth

SENT = -21846   # 0xAAAA: what the bytes around y hold


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_int16_entry_symbols_are_exported():
    from sparsernns_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("s5fxp_model_forward_i16", "s5fxp_workspace_bytes_i16", "s5fxp_stft_mag_i16", "s5fxp_mask_istft_i16"):
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS, name
    assert _lib.lib.s5fxp_version() >= 109


def test_int16_entry_rejects_bad_arguments_before_any_device_access():
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib

    E = _lib.S5FXP_EBADARG
    ok = dict(m=1, x=1, xb=16, xe=8, B=2, L=3, y=1, ws=1, st=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.s5fxp_model_forward_i16(a["m"], a["x"], a["xb"], a["xe"], a["B"], a["L"], a["y"], a["ws"], 1 << 30, a["st"],
                                           None, None, None)

    for bad in (dict(m=None), dict(x=None), dict(y=None), dict(ws=None), dict(st=None), dict(B=0), dict(L=0), dict(B=-1),
                dict(xb=0), dict(xb=17), dict(xb=32), dict(xb=-1)):
        assert call(**bad) == E, bad
    assert lib.s5fxp_workspace_bytes_i16(None, 2, 3) == 0


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name):
    """The engine of a synthetic model (ds0.25 .. ds1.0), a generic engine of ds0.5, or a contract model."""
    if name not in _MODELS:
        from sparsernns_amd import _lib
        from sparsernns_amd.engine import Engine
        from sparsernns_amd.fxpmodel import build_regression_model
        if name.startswith("F"):
            import contract_models as CM
            c = CM.case(name)
            eng, ex = c.engine(), c.export()
        else:
            ds = 0.5 if name == "generic" else float(name[2:])
            md, qc, dims = synth.make_model(ds, calib_L=128)
            model = build_regression_model(md, qc, dims["n_layers"])
            ex = model.export()
            eng = Engine(ex, flags=_lib.MODEL_FORCE_GENERIC) if name == "generic" else model.engine()
        _MODELS[name] = (eng, ex)
    return _MODELS[name][0]


def _input(eng, B, L, seed=0):
    """Rows at the encoder's input configuration that use the whole int16 range: the synthetic input, with one value in twenty
    replaced by a uniform int16."""
    from oracle import fxp_oracle as O
    rng = np.random.default_rng(seed)
    x = O.from_fp(synth.make_input(B, L, eng.d_in, seed=seed), eng.inp_bits, eng.inp_exp, True, O.FLOOR).data.astype(np.int64)
    wild = rng.integers(-32768, 32768, x.shape)
    x = np.where(rng.random(x.shape) < 0.05, wild, x)
    assert x.min() >= -32768 and x.max() <= 32767
    return x.astype(np.int16)


def _run(eng, xs, xb, xe, B, L, i16, groups=1, flags=0, state_in=None, carry=False, traced=False):
    """One forward through the int16 entry (i16) or the int32 entry on the widened input; returns (y as int32, status words,
    traces, state_out).  The int16 tensors start one element into their buffers; 64 sentinels lie either side of y."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import TRACE_FIELDS

    shape = tuple(xs.shape[:-1])
    nx, ny = xs.size, int(np.prod(shape)) * eng.d_out
    if i16:
        xbuf = torch.full((nx + 2,), SENT, dtype=torch.int16, device="cuda")
        x = xbuf[1:1 + nx].view(xs.shape)
        x.copy_(torch.from_numpy(xs))
        ybuf = torch.full((1 + 64 + ny + 64,), SENT, dtype=torch.int16, device="cuda")
        y = ybuf[65:65 + ny].view(shape + (eng.d_out,))
        assert x.data_ptr() % 4 == 2 and y.data_ptr() % 4 == 2 and x.is_contiguous() and y.is_contiguous()
    else:
        x = torch.from_numpy(xs.astype(np.int32)).cuda()
        y = torch.full(shape + (eng.d_out,), -7, dtype=torch.int32, device="cuda")
    so = None
    if carry:
        so = torch.full((eng.n_layers, 2, B, eng.P) if groups == 1 else (groups, eng.n_layers, 2, B, eng.P), -3,
                        dtype=torch.int32, device="cuda")
    tr = None
    if traced:
        tr = [{k: torch.full(shape + (eng.P if k in ("Bu_re", "Bu_im", "xs_re", "xs_im") else eng.H,), -5, dtype=torch.int32,
                             device="cuda") for k in TRACE_FIELDS} for _ in range(eng.n_layers)]
    eng.lane_status(0, groups).fill_(-9)
    eng.enqueue(x, xb, xe, y, B, L, traces=tr, flags=flags, state_in=state_in, state_out=so, groups=groups)
    torch.cuda.synchronize()
    if i16:
        guard = torch.cat([ybuf[:65], ybuf[65 + ny:]]).cpu().numpy()
        assert guard.size == 129 and np.all(guard == SENT), f"{np.count_nonzero(guard != SENT)} sentinels around y were overwritten"
        assert np.array_equal(xbuf[1:1 + nx].cpu().numpy().reshape(xs.shape), xs), "the input was modified"
    st = eng.lane_status(0, groups).cpu().numpy()[:groups * _lib.STATUS_WORDS].copy()
    trn = None if tr is None else [{k: v.cpu().numpy() for k, v in d.items()} for d in tr]
    return (y.cpu().numpy().astype(np.int32), st, trn, None if so is None else so.cpu().numpy())


def _same(eng, xs, xb=None, xe=None, B=None, L=None, **kw):
    xb = eng.inp_bits if xb is None else xb
    xe = eng.inp_exp if xe is None else xe
    B = xs.shape[0] if B is None else B
    L = xs.shape[1] if L is None else L
    a = _run(eng, xs, xb, xe, B, L, False, **kw)
    b = _run(eng, xs, xb, xe, B, L, True, **kw)
    assert a[0].min() >= -32768 and a[0].max() <= 32767, "the int32 entry's output leaves int16"
    assert np.array_equal(a[0], b[0]), f"y differs in {np.count_nonzero(a[0] != b[0])} values"
    assert np.array_equal(a[1], b[1]), np.nonzero(a[1] != b[1])
    if a[2] is not None:
        for i, (ta, tb) in enumerate(zip(a[2], b[2])):
            for k in ta:
                assert np.array_equal(ta[k], tb[k]), (i, k)
    if a[3] is not None:
        assert np.array_equal(a[3], b[3])
    return b


def _flag_sets():
    from test_float_io import _flag_sets as f
    return f()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ds0.25", "ds0.5", "ds0.75", "ds1.0", "generic", "F3_dims257x1_ds0.5", "F3_dims288x257_ds0.5",
                                  "F3_dims257x272_ds0.5", "F2_rails_ds0.5"])
def test_int16_entry_is_the_int32_entry(name):
    import torch
    from sparsernns_amd import _lib

    eng = _model(name)
    assert eng.out_bits <= 16
    xs = _input(eng, 2, 65, seed=1)
    for flags in _flag_sets():
        st = _same(eng, xs, flags=flags)[1]
        assert st[2] == (_lib.PATH_GENERIC if name == "generic" else _lib.PATH_FUSED)
    # traces, and a carry in and out
    y0 = _same(eng, xs, carry=True, traced=True)
    state = torch.from_numpy(y0[3]).cuda()
    _same(eng, _input(eng, 2, 63, seed=2), state_in=state, carry=True)
    # grouped: G independent batches in one call (one set of launches on the fused path, a loop on the generic one)
    _same(eng, _input(eng, 3 * 2, 33, seed=3), B=2, groups=3)
    # 1 x 5 x 257 = 1285 elements per group at d_in = 257: the groups' bases are odd in dwords
    _same(eng, _input(eng, 3 * 1, 5, seed=4), B=1, groups=3, carry=True, flags=_lib.FWD_DEFER_REDO)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 129])
def test_int16_entry_lengths(B, L):
    eng = _model("ds0.5")
    _same(eng, _input(eng, B, L, seed=10 * L + B))


@pytest.mark.gpu
def test_int16_entry_long_sequence():
    eng = _model("ds0.5")
    _same(eng, _input(eng, 1, 3751, seed=3751))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ds0.5", "ds1.0", "F3_dims288x257_ds0.5", "generic"])
def test_int16_edge_inputs(name):
    """-32768, 32767, 0 and +-1 in column 0, in lane 63's columns (252..255) and in the tail column 256 (and, for d_in = 288, the
    last one), among random rows; with (x_bits, x_exp) at the encoder's input configuration, then above it (the change_cfg inside
    the encoder runs and saturates) and below it."""
    eng = _model(name)
    enc = eng._desc.encoder
    # the lowest exponent the encoder's result shift takes (a negative shift is an error in both entries)
    low = max(0, enc.out_exp - enc.w_exp, eng.inp_exp - 2)
    assert low < eng.inp_exp, "the model leaves no input exponent below the encoder's"
    edges = np.array([-32768, 32767, 0, 1, -1], dtype=np.int16)
    cols = [0, 252, 253, 254, 255, 256, eng.d_in - 1]
    for xb, xe in ((eng.inp_bits, eng.inp_exp), (16, eng.inp_exp + 3), (eng.inp_bits, low), (min(eng.inp_bits, 12), eng.inp_exp)):
        xs = _input(eng, 2, 70, seed=7 + xe)
        for i, v in enumerate(edges):
            for j, c in enumerate(cols):
                xs[0, 5 * j + i, c] = v          # one edge value per row ...
            xs[1, i, cols] = v                   # ... and rows that hold it in all of those columns
            xs[1, 69 - i, :] = v                 # ... and in every column (the tensor's last rows)
        _same(eng, xs, xb=xb, xe=xe)


@pytest.mark.gpu
def test_int16_entry_refuses_a_wide_output():
    """F3_out32: the decoder's output has 32 bits, the narrowing would lose them: NotImplementedError, y untouched."""
    import torch
    eng = _model("F3_out32_ds0.5")
    assert eng.out_bits > 16
    x = torch.zeros((2, 5, eng.d_in), dtype=torch.int16, device="cuda")
    y = torch.full((2, 5, eng.d_out), SENT, dtype=torch.int16, device="cuda")
    with pytest.raises(NotImplementedError):
        eng.enqueue(x, eng.inp_bits, eng.inp_exp, y, 2, 5)
    with pytest.raises(NotImplementedError):
        eng.forward_int16(x)
    torch.cuda.synchronize()
    assert bool((y == SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ds0.5", "F2_rails_ds0.5"])
def test_int16_entry_matches_the_c_oracle(name):
    """The C oracle's forward on the widened input: independent of the device's int32 entry."""
    import torch
    from oracle import cref

    eng = _model(name)
    xs = _input(eng, 2, 70, seed=9)
    ref, rb, re_, _ = cref.CModel(_MODELS[name][1]).forward(xs.astype(np.int32), eng.inp_bits, eng.inp_exp)
    got = eng.forward_int16(torch.from_numpy(xs))
    assert got.dtype == torch.int16 and (rb, re_) == (eng.out_bits, eng.out_exp)
    assert np.array_equal(ref, got.cpu().numpy().astype(np.int32))


def _profiled(fn):
    from test_variant_matrix import _profiled as p
    return p(fn)[0]


@pytest.mark.gpu
def test_fused_int16_forward_launches_no_conversion_pass():
    """The int16 forward's kernel list is the int forward's one for one (same grids) with k_enc_ps / k_dec_ps in place of
    k_enc_p / k_dec_p, and no k_widen_i16 / k_narrow_i16; all twelve int16 instantiations run (dim 0.25 .. 1.0, with and
    without the decoder's residual pass)."""
    import torch
    from sparsernns_amd import _lib
    from test_variant_matrix import _targs

    seen = set()
    for name in ("ds0.25", "ds0.5", "ds0.75", "ds1.0"):
        eng = _model(name)
        assert _lib.lib.s5fxp_workspace_bytes_i16(eng._h, 2, 65) == _lib.lib.s5fxp_workspace_bytes(eng._h, 2, 65)
        xs = torch.from_numpy(_input(eng, 2, 65)).cuda()
        xi = xs.to(torch.int32)
        for traced in (False, True):
            kw = {}
            if traced:
                from sparsernns_amd._lib import TRACE_FIELDS
                kw["traces"] = [{k: torch.empty((2, 65, eng.P if k in ("Bu_re", "Bu_im", "xs_re", "xs_im") else eng.H),
                                                dtype=torch.int32, device="cuda") for k in TRACE_FIELDS} for _ in range(eng.n_layers)]
            ys = torch.empty((2, 65, eng.d_out), dtype=torch.int16, device="cuda")
            yi = torch.empty((2, 65, eng.d_out), dtype=torch.int32, device="cuda")
            ks = _profiled(lambda: eng.enqueue(xs, eng.inp_bits, eng.inp_exp, ys, 2, 65, flags=_lib.FWD_DEFER_REDO, **kw))
            ki = _profiled(lambda: eng.enqueue(xi, eng.inp_bits, eng.inp_exp, yi, 2, 65, flags=_lib.FWD_DEFER_REDO, **kw))
            names = [_targs(n)[0] for n, _ in ks]
            assert "k_widen_i16" not in names and "k_narrow_i16" not in names
            assert "k_enc_p" not in names and "k_dec_p" not in names
            twin = {"k_enc_ps": "k_enc_p", "k_dec_ps": "k_dec_p"}
            mapped = [(twin.get(_targs(n)[0], _targs(n)[0]), _targs(n)[1], g) for n, g in ks]
            assert mapped == [(_targs(n)[0], _targs(n)[1], g) for n, g in ki]
            seen |= {(_targs(n)[0], tuple(_targs(n)[1])) for n, _ in ks if _targs(n)[0] in twin}
    want = {("k_enc_ps", (nt,)) for nt in "2356"} | {("k_dec_ps", (nt, r)) for nt in "2356" for r in ("false", "true")}
    assert seen == want, seen


@pytest.mark.gpu
def test_enqueue_rejects_mixed_dtypes_with_int16():
    import torch
    eng = _model("ds0.5")
    t = {d: (torch.zeros((1, 4, eng.d_in), dtype=d, device="cuda"), torch.empty((1, 4, eng.d_out), dtype=d, device="cuda"))
         for d in (torch.int16, torch.int32, torch.float32, torch.int64, torch.uint8)}
    for dx, dy in ((torch.int16, torch.int32), (torch.int32, torch.int16), (torch.int16, torch.float32),
                   (torch.float32, torch.int16), (torch.int64, torch.int64), (torch.uint8, torch.uint8)):
        with pytest.raises(ValueError):
            eng.enqueue(t[dx][0], eng.inp_bits, eng.inp_exp, t[dy][1], 1, 4)


@pytest.mark.gpu
def test_int16_callers():
    """InflightRunner with int16 tensors, Engine.forward_int16 / forward_batches_int16 / forward_chunk_int16 and
    FxpRegressionModel.forward_int16 give the integers of their int32 forms."""
    import torch
    from sparsernns_amd.engine import InflightRunner
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = synth.make_model(0.5, calib_L=128)
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    xs = torch.from_numpy(_input(eng, 4, 40, seed=11)).cuda()
    fx = lambda t: FxpArray(t.to(torch.int32).contiguous(), ib, ie, True)
    ref = model(fx(xs)).data
    narrow = lambda t: t.to(torch.int16)
    assert bool((ref == narrow(ref)).all())

    for got in (model.forward_int16(xs), eng.forward_int16(xs), eng.forward_int16(xs, ib, ie), eng.forward_int16(xs, check_status=False)):
        assert got.dtype == torch.int16 and torch.equal(got, narrow(ref))
    assert torch.equal(eng.forward_batches_int16(xs, 2), narrow(eng.forward_batches(fx(xs), 2).data))
    yc, state = eng.forward_chunk_int16(xs[:, :25])
    yc2, _ = eng.forward_chunk_int16(xs[:, 25:], state)
    ic, istate = eng.forward_chunk(fx(xs[:, :25]))
    ic2, _ = eng.forward_chunk(fx(xs[:, 25:]), istate)
    assert torch.equal(yc, narrow(ic.data)) and torch.equal(yc2, narrow(ic2.data)) and torch.equal(state, istate)
    with pytest.raises(ValueError):
        eng.forward_int16(xs.to(torch.int32))

    runner = InflightRunner(eng, 2)
    outs = [torch.empty((4, 40, eng.d_out), dtype=torch.int16, device="cuda") for _ in range(3)]
    for y in outs:
        runner.submit(xs, ib, ie, y, 4, 40)
    runner.drain()
    assert all(torch.equal(y, narrow(ref)) for y in outs)
