"""The float-in, float-out forward (include/s5fxp.h s5fxp_model_forward_f32), the reference's validation step
(sparseRNNs/fxprun.py:63-88) in one call.  It must give bit for bit what the three-step route gives:
s5fxp_from_fp(FLOOR) -> s5fxp_model_forward -> s5fxp_to_float -- output, every status word, every trace plane and the carry
-- for every option the int entry takes, on the fused path (the conversions inside k_enc_pf / k_dec_pf) and on the generic one.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import fxp_oracle as O
from sparsernns_amd import synth


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_float_entry_symbols_are_exported():
    from sparsernns_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("s5fxp_model_forward_f32", "s5fxp_workspace_bytes_f32"):
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS
    assert _lib.lib.s5fxp_version() >= 103


def test_float_entry_rejects_bad_arguments_before_any_device_access():
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib

    E = _lib.S5FXP_EBADARG
    ok = dict(m=1, x=1, xb=16, xe=8, B=2, L=3, y=1, ws=1, st=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.s5fxp_model_forward_f32(a["m"], a["x"], a["xb"], a["xe"], a["B"], a["L"], a["y"], a["ws"], 1 << 30, a["st"],
                                           None, None, None)

    for bad in (dict(m=None), dict(x=None), dict(y=None), dict(ws=None), dict(st=None), dict(B=0), dict(L=0), dict(B=-1),
                dict(xb=0), dict(xb=33), dict(xe=-1), dict(xe=32)):
        assert call(**bad) == E, bad
    assert lib.s5fxp_workspace_bytes_f32(None, 2, 3) == 0


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name):
    """The engine of a synthetic model, a generic engine of it, or a contract model."""
    if name not in _MODELS:
        from sparsernns_amd import _lib
        from sparsernns_amd.engine import Engine
        from sparsernns_amd.fxpmodel import build_regression_model
        if name.startswith("F3_"):
            import contract_models as CM
            c = CM.case(name)
            eng, ex = c.engine(), c.export()
        else:
            ds = 1.0 if name == "ds1.0" else 0.5
            md, qc, dims = synth.make_model(ds, calib_L=128)
            model = build_regression_model(md, qc, dims["n_layers"])
            ex = model.export()
            eng = Engine(ex, flags=_lib.MODEL_FORCE_GENERIC) if name == "generic" else model.engine()
        _MODELS[name] = (eng, ex)
    return _MODELS[name][0]


def _float_input(eng, B, L, seed=0):
    """Float rows that quantise to the whole int16 range of the encoder's input, most of them between 2^-exp steps."""
    rng = np.random.default_rng(seed)
    span = 2.0 ** (eng.inp_bits - 1 - eng.inp_exp)
    x = synth.make_input(B, L, eng.d_in, seed=seed).astype(np.float64)
    x += rng.uniform(-0.5, 0.5, x.shape) * span * (rng.random(x.shape) < 0.05)
    return x.astype(np.float32)


def _run(eng, xf, xb, xe, B, L, f32, groups=1, flags=0, state_in=None, carry=False, traced=False):
    """One forward through the float entry (f32) or the three-step route; returns (y as float32 bits, status words, traces,
    state_out)."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import TRACE_FIELDS
    from sparsernns_amd.fxparray import FxpArray, RoundingMode, fxp_from_fp

    xd = torch.from_numpy(xf).cuda()
    shape = tuple(xd.shape[:-1])
    if f32:
        x, y = xd, torch.full(shape + (eng.d_out,), float("nan"), dtype=torch.float32, device="cuda")
    else:
        x = fxp_from_fp(xd, bits=xb, exp=xe, signed=True, round_mode=RoundingMode.FLOOR).data
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
    if not f32:
        y = FxpArray(y, eng.out_bits, eng.out_exp, True).to_float()
    st = eng.lane_status(0, groups).cpu().numpy()[:groups * _lib.STATUS_WORDS].copy()
    trn = None if tr is None else [{k: v.cpu().numpy() for k, v in d.items()} for d in tr]
    return (y.view(torch.int32).cpu().numpy(), st, trn, None if so is None else so.cpu().numpy())


def _same(eng, xf, xb=None, xe=None, B=None, L=None, **kw):
    xb = eng.inp_bits if xb is None else xb
    xe = eng.inp_exp if xe is None else xe
    B = xf.shape[0] if B is None else B
    L = xf.shape[1] if L is None else L
    a = _run(eng, xf, xb, xe, B, L, False, **kw)
    b = _run(eng, xf, xb, xe, B, L, True, **kw)
    assert np.array_equal(a[0], b[0]), f"y differs in {np.count_nonzero(a[0] != b[0])} values"
    assert np.array_equal(a[1], b[1]), np.nonzero(a[1] != b[1])
    if a[2] is not None:
        for i, (ta, tb) in enumerate(zip(a[2], b[2])):
            for k in ta:
                assert np.array_equal(ta[k], tb[k]), (i, k)
    if a[3] is not None:
        assert np.array_equal(a[3], b[3])
    return a


def _flag_sets():
    from sparsernns_amd import _lib
    return (0, _lib.FWD_DEFER_REDO, _lib.FWD_EXACT, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ds0.5", "ds1.0", "generic", "F3_dims257x1_ds0.5", "F3_dims288x257_ds0.5",
                                  "F3_dims257x272_ds0.5", "F3_out32_ds0.5"])
def test_float_entry_is_the_three_step_route(name):
    import torch
    from sparsernns_amd import _lib

    eng = _model(name)
    xf = _float_input(eng, 2, 65, seed=1)
    for flags in _flag_sets():
        st = _same(eng, xf, flags=flags)[1]
        assert st[2] == (_lib.PATH_GENERIC if name == "generic" else _lib.PATH_FUSED)
    # traces, and a carry in and out
    y0 = _same(eng, xf, carry=True, traced=True)
    state = torch.from_numpy(y0[3]).cuda()
    _same(eng, _float_input(eng, 2, 63, seed=2), state_in=state, carry=True)
    # grouped: G independent batches in one call (one set of launches on the fused path, a loop on the generic one)
    _same(eng, _float_input(eng, 3 * 2, 33, seed=3), B=2, groups=3)
    _same(eng, _float_input(eng, 3 * 1, 5, seed=4), B=1, groups=3, carry=True, flags=_lib.FWD_DEFER_REDO)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 63, 65, 3751])
def test_float_entry_lengths(L):
    eng = _model("ds0.5")
    _same(eng, _float_input(eng, 1, L, seed=L))


def _edge_values(bits, exp):
    step = np.float32(2.0 ** -exp)
    on = np.arange(-6, 7, dtype=np.float32) * step
    below = np.nextafter(on, np.float32(-np.inf))
    rail = np.float32(2.0 ** (bits - 1 - exp))
    return np.concatenate([on, below, np.array([rail, -rail, rail - step, -rail - step, rail * 4, -rail * 4, 1e30, -1e30, 3e38,
                                                -3e38, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.inf, -np.inf, np.nan], dtype=np.float32)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ds0.5", "F3_dims288x257_ds0.5", "generic"])
def test_float_edge_inputs(name):
    """Values on and just below the 2^-x_exp steps, rails and far beyond, -0.0, denormals, +-inf and NaN; with the quantisation
    target at, above and below the encoder's input configuration (above: the change_cfg inside the encoder runs)."""
    eng = _model(name)
    rng = np.random.default_rng(7)
    for db, de in ((0, 0), (4, 3), (-4, -2), (32 - eng.inp_bits, 31 - eng.inp_exp)):
        xb, xe = eng.inp_bits + db, eng.inp_exp + de
        vals = _edge_values(xb, xe)
        xf = rng.choice(vals, size=(2, 70, eng.d_in)).astype(np.float32)
        xf[0, :3, :len(vals)] = vals[:eng.d_in]   # every value at least once, in the K-256 tail too
        xf[1, -1, -len(vals):] = vals[-eng.d_in:]
        _same(eng, xf, xb=xb, xe=xe)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ds0.5", "F3_out32_ds0.5"])
def test_float_entry_matches_the_c_oracle(name):
    """O.from_fp -> the C oracle's forward -> data / 2^out_exp in float32: independent of the device's k_from_fp / k_to_float."""
    import torch
    from oracle import cref

    eng = _model(name)
    xf = _float_input(eng, 2, 70, seed=9)
    fx = O.from_fp(xf, eng.inp_bits, eng.inp_exp, True, O.FLOOR)
    ref, rb, re_, _ = cref.CModel(_MODELS[name][1]).forward(fx.data, fx.bits, fx.exp)
    want = (ref.astype(np.float64) / 2.0 ** re_).astype(np.float32)
    got = eng.forward_float(torch.from_numpy(xf)).cpu().numpy()
    assert re_ == eng.out_exp
    assert np.array_equal(want.view(np.int32), got.view(np.int32))


def _profiled(fn):
    from test_variant_matrix import _profiled as p
    return p(fn)[0]


@pytest.mark.gpu
def test_fused_float_forward_launches_no_conversion_pass():
    """The float forward's kernel list is the int forward's one for one (same grids) with k_enc_pf / k_dec_pf in place of
    k_enc_p / k_dec_p, and no k_from_fp / k_to_float; all six float instantiations run (dim 0.5 / 1.0, with and without the
    decoder's residual pass)."""
    import torch
    from sparsernns_amd import _lib
    from test_variant_matrix import _targs

    seen = set()
    for name in ("ds0.5", "ds1.0"):
        eng = _model(name)
        assert _lib.lib.s5fxp_workspace_bytes_f32(eng._h, 2, 65) == _lib.lib.s5fxp_workspace_bytes(eng._h, 2, 65)
        xf = torch.from_numpy(_float_input(eng, 2, 65)).cuda()
        xi = torch.zeros(xf.shape, dtype=torch.int32, device="cuda")
        for traced in (False, True):
            kw = {}
            if traced:
                from sparsernns_amd._lib import TRACE_FIELDS
                kw["traces"] = [{k: torch.empty((2, 65, eng.P if k in ("Bu_re", "Bu_im", "xs_re", "xs_im") else eng.H),
                                                dtype=torch.int32, device="cuda") for k in TRACE_FIELDS} for _ in range(eng.n_layers)]
            yf = torch.empty((2, 65, eng.d_out), dtype=torch.float32, device="cuda")
            yi = torch.empty((2, 65, eng.d_out), dtype=torch.int32, device="cuda")
            kf = _profiled(lambda: eng.enqueue(xf, eng.inp_bits, eng.inp_exp, yf, 2, 65, flags=_lib.FWD_DEFER_REDO, **kw))
            ki = _profiled(lambda: eng.enqueue(xi, eng.inp_bits, eng.inp_exp, yi, 2, 65, flags=_lib.FWD_DEFER_REDO, **kw))
            names = [_targs(n)[0] for n, _ in kf]
            assert "k_from_fp" not in names and "k_to_float" not in names
            assert "k_enc_p" not in names and "k_dec_p" not in names
            mapped = [(_targs(n)[0].replace("_pf", "_p"), _targs(n)[1], g) for n, g in kf]
            assert mapped == [(_targs(n)[0], _targs(n)[1], g) for n, g in ki]
            seen |= {(b, tuple(a)) for b, a, _ in [(_targs(n)[0], _targs(n)[1], g) for n, g in kf] if b in ("k_enc_pf", "k_dec_pf")}
    assert seen == {("k_enc_pf", ("3",)), ("k_enc_pf", ("6",)), ("k_dec_pf", ("3", "false")), ("k_dec_pf", ("3", "true")),
                    ("k_dec_pf", ("6", "false")), ("k_dec_pf", ("6", "true"))}, seen


@pytest.mark.gpu
def test_enqueue_rejects_mixed_dtypes():
    import torch
    eng = _model("ds0.5")
    xf = torch.zeros((1, 4, eng.d_in), dtype=torch.float32, device="cuda")
    xi = torch.zeros((1, 4, eng.d_in), dtype=torch.int32, device="cuda")
    yf = torch.empty((1, 4, eng.d_out), dtype=torch.float32, device="cuda")
    yi = torch.empty((1, 4, eng.d_out), dtype=torch.int32, device="cuda")
    for x, y in ((xf, yi), (xi, yf), (xf.double(), yf.double())):
        with pytest.raises(ValueError):
            eng.enqueue(x, eng.inp_bits, eng.inp_exp, y, 1, 4)


@pytest.mark.gpu
def test_float_callers(tmp_path):
    """InflightRunner with float tensors, Engine.forward_batches_float / forward_chunk_float, FxpRegressionModel.forward_float,
    audio.denoise and fxprun --outputs give what the int route gives."""
    import torch
    from sparsernns_amd import audio, fxprun
    from sparsernns_amd.engine import InflightRunner
    from sparsernns_amd.fxparray import RoundingMode, fxp_from_fp
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = synth.make_model(0.5, calib_L=128)
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    xf = torch.from_numpy(_float_input(eng, 4, 40, seed=11)).cuda()
    ref = model(fxp_from_fp(xf, bits=ib, exp=ie, signed=True, round_mode=RoundingMode.FLOOR)).to_float()

    assert torch.equal(model.forward_float(xf), ref)
    assert torch.equal(eng.forward_batches_float(xf, 2), torch.cat([model.forward_float(xf[:2]), model.forward_float(xf[2:])]))
    yc, state = eng.forward_chunk_float(xf[:, :25])
    yc2, _ = eng.forward_chunk_float(xf[:, 25:], state)
    ic, istate = eng.forward_chunk(fxp_from_fp(xf[:, :25].contiguous(), bits=ib, exp=ie))
    ic2, _ = eng.forward_chunk(fxp_from_fp(xf[:, 25:].contiguous(), bits=ib, exp=ie), istate)
    assert torch.equal(yc, ic.to_float()) and torch.equal(yc2, ic2.to_float()) and torch.equal(state, istate)

    runner = InflightRunner(eng, 2)
    outs = [torch.empty((4, 40, eng.d_out), dtype=torch.float32, device="cuda") for _ in range(3)]
    for y in outs:
        runner.submit(xf, ib, ie, y, 4, 40)
    runner.drain()
    assert all(torch.equal(y, ref) for y in outs)

    g = torch.Generator().manual_seed(5)
    noisy = (0.02 * torch.randn(2, 128 * 63, generator=g)).cuda()
    _, cleaned_mag, mag = audio.denoise(model, ib, ie, noisy)
    x = (mag - audio.STFT_MAG_MEAN).transpose(-1, -2).contiguous()
    mask = model(fxp_from_fp(x, bits=ib, exp=ie, signed=True, round_mode=RoundingMode.FLOOR)).to_float().transpose(-1, -2)
    assert torch.equal(cleaned_mag, mag * (1.0 + mask))

    out = str(tmp_path / "y.npy")
    common = ["--synthetic", "--seq_len", "64", "--bsz", "2", "--seed", "5", "--steps", "2"]
    assert fxprun.main(common + ["--outputs", out]) == 0
    m2, q2, d2 = synth.make_model(0.5, calib_L=64, state_headroom_bits=1)
    e2 = build_regression_model(m2, q2, d2["n_layers"]).engine()
    xs = synth.make_input(2, 64, d2["d_in"], seed=5)
    yi = e2.forward(fxp_from_fp(xs, bits=q2["encoder"]["inp_bits"], exp=q2["encoder"]["inp_exp"])).to_float().cpu().numpy()
    assert np.array_equal(np.load(out).view(np.int32), yi.view(np.int32))
