"""The tile I/O of the encoder and the decoder (proj_dec_body.inc, proj_enc_body.inc) at its edges, bit for bit against the C
oracle (oracle/cref.py).

The decoder writes a 64-frame tile of y into LDS and moves it out as 16-byte vectors.  What can go wrong there: a tensor's
partial last tile (its valid bytes are whole vectors plus a remainder of single elements, and nothing behind them may be
touched), a group's output base that is aligned to one element only, the ragged ninth column tile, the int16 tile of half the
size, and the shapes whose LDS holds one workgroup per CU.  The encoder's tail column (element 256 of a row at d_in = 257) must
still take part in the wide-input check, down to the last valid row.

Every output sits between poisoned elements, which must come back untouched.
"""
import numpy as np
import pytest

from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth

pytestmark = pytest.mark.gpu

PAD = 96            # poisoned elements either side of y
IOS = ("i32", "f32", "i16")
POISON = {"i32": -1431655766, "f32": -1431655766, "i16": -21846}   # 0xAA..AA (as float bits: -3.0316e-13)

_MODELS, _REFS = {}, {}


def _model(name):
    """(engine, C oracle) of a synthetic model ds<dim_scale> or of a contract model (tests/contract_models.py)."""
    if name not in _MODELS:
        from sparsernns_amd.fxpmodel import build_regression_model
        if name.startswith("F3_"):
            import contract_models as CM
            c = CM.case(name)
            _MODELS[name] = (c.engine(), c.c_oracle())
        else:
            md, qc, dims = synth.make_model(float(name[2:]), calib_L=128)
            model = build_regression_model(md, qc, dims["n_layers"])
            _MODELS[name] = (model.engine(), cref.CModel(model.export()))
    return _MODELS[name]


def _case(name, B, L, seed):
    """(int32 input, the oracle's output) of one batch; computed once per (model, shape, seed) and never modified."""
    key = (name, B, L, seed)
    if key not in _REFS:
        eng, cm = _model(name)
        x = O.from_fp(synth.make_input(B, L, eng.d_in, seed=seed), eng.inp_bits, eng.inp_exp, True, O.FLOOR).data
        x = np.ascontiguousarray(x, dtype=np.int32)
        ref, rb, re_, _ = cm.forward(x, eng.inp_bits, eng.inp_exp)
        assert (rb, re_) == (eng.out_bits, eng.out_exp)
        ref = np.ascontiguousarray(ref, dtype=np.int32)
        x.setflags(write=False)
        ref.setflags(write=False)
        _REFS[key] = (x, ref)
    return _REFS[key]


def _forward(eng, x, B, L, io, groups=1, traced=False, ladder=True):
    """One fused forward of int32 rows x ((groups * B, L, d_in)) through the boundary `io`; y lies PAD poisoned elements into
    its buffer (an odd number of elements for int16: 2-byte alignment only).  An untraced forward starts on the optimistic
    recurrence kernels and steps down the ladder while ST_REDO comes back, as Engine.forward does (ladder=False: one
    self-contained launch, whatever its status says); a traced one is self-contained.  Returns (y, status words)."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import TRACE_FIELDS

    dt = {"i32": torch.int32, "f32": torch.float32, "i16": torch.int16}[io]
    shape = (groups * B, L)
    ny = groups * B * L * eng.d_out
    lead = PAD + 1 if io == "i16" else PAD
    if io == "f32":
        xd = torch.from_numpy(x.astype(np.float64) * 2.0 ** -eng.inp_exp).to(torch.float32).cuda()   # exact: 16 bits and a power of two
        ybuf = torch.full((lead + ny + PAD,), POISON[io], dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        assert io == "i32" or (x.min() >= -32768 and x.max() <= 32767)
        xd = torch.from_numpy(x.astype(np.int16 if io == "i16" else np.int32)).cuda()
        ybuf = torch.full((lead + ny + PAD,), POISON[io], dtype=dt, device="cuda")
    y = ybuf[lead:lead + ny].view(shape + (eng.d_out,))
    tr = None
    if traced:
        tr = [{k: torch.empty(shape + (eng.P if k in ("Bu_re", "Bu_im", "xs_re", "xs_im") else eng.H,), dtype=torch.int32,
                              device="cuda") for k in TRACE_FIELDS} for _ in range(eng.n_layers)]
    eng.lane_status(0, groups).fill_(-9)
    if traced or not ladder:
        eng.enqueue(xd, eng.inp_bits, eng.inp_exp, y, B, L, traces=tr, groups=groups, flags=0)
    else:
        eng.level = 0
        eng.run_ladder(lambda fl: eng.enqueue(xd, eng.inp_bits, eng.inp_exp, y, B, L, groups=groups, flags=fl), eng.check_status)
    torch.cuda.synchronize()
    raw = ybuf.view(torch.int32) if io == "f32" else ybuf
    guard = torch.cat([raw[:lead], raw[lead + ny:]]).cpu().numpy()
    assert np.all(guard == POISON[io]), f"{np.count_nonzero(guard != POISON[io])} poisoned elements around y were overwritten"
    st = eng.lane_status(0, groups).cpu().numpy()[:groups * _lib.STATUS_WORDS].copy()
    for g in range(groups):
        w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
        assert w[2] == _lib.PATH_FUSED and not (w[0] & _lib.ST_REDO), w[:8]
    return y.cpu().numpy(), st


def _expect(eng, ref, io):
    """The oracle's int32 output as the boundary `io` delivers it."""
    if io == "f32":
        assert eng.out_bits <= 24   # every value is a float32
        return (ref.astype(np.float64) * 2.0 ** -eng.out_exp).astype(np.float32)
    if io == "i16":
        assert eng.out_bits <= 16
        return ref.astype(np.int16)
    return ref


def _check(got, want, what):
    if got.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    assert np.array_equal(got, want), f"{what}: {np.count_nonzero(got != want)} of {want.size} values differ"


@pytest.mark.parametrize("frames", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("io", IOS)
def test_partial_tiles(io, frames):
    """No full tile, exactly one, and a partial last tile whose valid bytes are no multiple of 16 (1, 63 and 65 frames of 257
    elements; 130 = 2 x 65 crosses a sequence boundary inside a tile)."""
    B, L = (2, 65) if frames == 130 else (1, frames)
    eng, _ = _model("ds0.5")
    x, ref = _case("ds0.5", B, L, seed=frames)
    got, _ = _forward(eng, x, B, L, io)
    _check(got, _expect(eng, ref, io), f"{io}, {frames} frames")


@pytest.mark.parametrize("BL", [(1, 3), (3, 67)])
@pytest.mark.parametrize("io", IOS)
def test_unaligned_group_bases(io, BL):
    """groups = 3 with B L 257 % 4 != 0: the second and third group's y start 4, 8 or 12 bytes (int16: odd multiples of 2) off a
    16-byte boundary.  Every group must equal its own single forward, and the oracle."""
    B, L = BL
    eng, _ = _model("ds0.5")
    assert (B * L * eng.d_out) % 4 != 0
    parts = [_case("ds0.5", B, L, seed=300 + g) for g in range(3)]
    got, _ = _forward(eng, np.concatenate([p[0] for p in parts]), B, L, io, groups=3)
    for g, (x, ref) in enumerate(parts):
        _check(got[g * B:(g + 1) * B], _expect(eng, ref, io), f"{io}, group {g} against the oracle")
        single, _ = _forward(eng, x, B, L, io)
        _check(got[g * B:(g + 1) * B], single, f"{io}, group {g} against its single forward")


@pytest.mark.parametrize("traced", [False, True], ids=["resid", "plain"])
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("ds", ["ds0.25", "ds0.5", "ds0.75", "ds1.0"])
def test_every_shape_and_both_decoder_forms(ds, io, traced):
    """The four channel counts (H = 48 and 144 are the ragged ones; at 144 and 192 a 4-byte tile leaves room for one workgroup
    per CU), the decoder with the last layer's residual pass (an untraced forward) and without it (a traced one)."""
    eng, _ = _model(ds)
    x, ref = _case(ds, 2, 65, seed=11)
    got, _ = _forward(eng, x, 2, 65, io, traced=traced)
    _check(got, _expect(eng, ref, io), f"{ds} {io} traced={traced}")


@pytest.mark.parametrize("io", ["i32", "f32"])
@pytest.mark.parametrize("name", ["F3_dims288x257_ds0.5", "F3_dims257x272_ds0.5", "F3_dims257x1_ds0.5"])
def test_other_widths(name, io):
    """d_in = 288: the encoder's tail is 32 columns wide and takes the loop; d_out = 272 and 1: the widest tile the library
    accepts and one of 256 bytes (16 vectors: most waves copy nothing)."""
    eng, _ = _model(name)
    for B, L in ((1, 1), (2, 65)):
        x, ref = _case(name, B, L, seed=7 + L)
        got, _ = _forward(eng, x, B, L, io)
        _check(got, _expect(eng, ref, io), f"{name} {io} {B}x{L}")


@pytest.mark.parametrize("BL", [(1, 65), (2, 64), (1, 1)])
def test_wide_input_in_the_tail_column(BL):
    """An int32 input whose only out-of-range element is element 256 of the last valid row raises ST_WIDE_INPUT; the same input
    with that element in range does not."""
    from sparsernns_amd import _lib
    B, L = BL
    eng, _ = _model("ds0.5")
    assert eng.d_in == 257
    x, ref = _case("ds0.5", B, L, seed=500 + L)
    got, st = _forward(eng, x, B, L, "i32", ladder=False)
    assert not (st[0] & _lib.ST_WIDE_INPUT), st[:8]
    _check(got, ref, "in range")
    for v in (1 << 15, -(1 << 15) - 1, 1 << 24):
        xw = x.copy()
        xw[B - 1, L - 1, 256] = v
        _, st = _forward(eng, xw, B, L, "i32", ladder=False)
        assert st[0] & _lib.ST_WIDE_INPUT, (v, st[:8])
