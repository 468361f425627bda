"""The fused MFMA forward at dim_scale 0.25 (H = 48, P = 32) and 0.75 (H = 144, P = 96): the two N-DNS shapes whose last
32-channel tile is half empty (csrc/proj_p.hpp shape_channels).  Every comparison is np.array_equal against the C oracle of the
product's own export, through the C ABI: the path, the four flag sets at ragged lengths, an overflowing input, every trace
field, the carry, grouped launches, the float entry, the contract families (tests/contract_models.py) at both shapes, the
inputs that would show a pad lane in a maximum, and one full-size batch per shape.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_DS = (0.25, 0.75)
TRACE_MAP = dict(pre_s5="pre_s5", u="u", Bu_re="bu_re", Bu_im="bu_im", xs_re="xs_re", xs_im="xs_im", ys="ys",
                 out2="out2", out2_sigmoid="sigmoid", post_GLU="post_glu", residadd="residadd")


# ------------------------------------------------------------------------------------------------------------------------
# the shape rule, restated for the tests' expectations (csrc/s5fxp_fast.hpp fast_shape)
# ------------------------------------------------------------------------------------------------------------------------
FUSED_SHAPES = {(48, 32), (96, 64), (144, 96), (192, 128)}


def fused_shape(H: int, P: int) -> bool:
    """The fused path's (H, P): the N-DNS recipe at dim_scale 0.25, 0.5, 0.75, 1.0."""
    return (H, P) in FUSED_SHAPES


def state_slots(P: int, n_live: int) -> int:
    """State slots of a layer on an untraced, carry-free forward: compaction needs P % 64 == 0 (s5fxp_fast.hpp pack_fast),
    so layers of 32 and 96 states always run on all of them."""
    import contract_models as CM
    return CM.compact_slots(n_live, P) if P % 64 == 0 else P


def test_shape_rule_agrees_with_the_recipe_dims():
    """Not GPU: the rule above against synth.ndns_dims (main.py:480-485 of the reference: blocks = int(16 s), H = 12 blocks,
    P = 8 blocks)."""
    want = {0.25: (48, 32), 0.5: (96, 64), 0.75: (144, 96), 1.0: (192, 128)}
    for ds, hp in want.items():
        d = synth.ndns_dims(ds)
        assert (d["H"], d["P"]) == hp and fused_shape(*hp), ds
    d = synth.ndns_dims(0.375)
    assert (d["H"], d["P"]) == (72, 48) and not fused_shape(72, 48)
    assert not fused_shape(48, 64) and not fused_shape(144, 128) and not fused_shape(8, 4)
    assert state_slots(32, 12) == 32 and state_slots(96, 24) == 96 and state_slots(64, 20) == 32 and state_slots(128, 40) == 64


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
_RECIPES = {}


class Recipe:
    def __init__(self, ds, md, qc, dims, headroom):
        from sparsernns_amd.fxpmodel import build_regression_model
        self.ds, self.md, self.qc, self.dims, self.headroom = ds, md, qc, dims, headroom
        self.model = build_regression_model(md, qc, dims["n_layers"])
        self.cm = cref.CModel(self.model.export())
        self.nl = dims["n_layers"]
        self._eng = None

    @property
    def eng(self):
        if self._eng is None:
            self._eng = self.model.engine()
        return self._eng

    def input(self, B, L, seed=0, scale=1.0):
        x = synth.make_input(B, L, self.dims["d_in"], seed=seed, scale=scale)
        return O.from_fp(x, self.qc["encoder"]["inp_bits"], self.qc["encoder"]["inp_exp"], True, O.FLOOR)


def _top_state(rtr) -> int:
    return max(max(int(np.abs(t["xs_re"]).max()), int(np.abs(t["xs_im"]).max())) for t in rtr)


def recipe(ds) -> Recipe:
    """synth.make_model(dim_scale=ds, calib_L=256, state_headroom_bits=h) with the smallest h >= 1 at which the oracle's
    states of the probe input (scale 1) fit the int16 recurrence streams -- checked on the CPU, here."""
    if ds not in _RECIPES:
        for h in (1, 2, 3, 4):
            md, qc, dims = synth.make_model(dim_scale=ds, calib_L=256, state_headroom_bits=h)
            r = Recipe(ds, md, qc, dims, h)
            fx = r.input(3, 333, seed=11)
            if _top_state(r.cm.forward(fx.data, fx.bits, fx.exp, trace=True)[3]) <= 32766:
                break
        else:
            raise AssertionError(f"dim_scale {ds}: the states do not fit 16 bits with 4 bits of headroom")
        _RECIPES[ds] = r
    return _RECIPES[ds]


def _words(eng, nl, k, lane=0, group=0):
    from sparsernns_amd import _lib
    st = eng.lane_status(lane, group + 1).cpu().numpy()[group * _lib.STATUS_WORDS:]
    return [int(v) for v in st[8 + k:8 + 8 * nl:8]]


def _flag_sets():
    from sparsernns_amd import _lib
    return (0, _lib.FWD_DEFER_REDO, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, _lib.FWD_EXACT)


def _check_flags(eng, cm, nl, P, x, bits, exp, live, what):
    """The four flag sets on one input: path, rungs, slots, and the output wherever the forward completed (a deferred forward
    that reports ST_REDO has no output by contract; it must not happen while the oracle's states are inside the bound the
    model itself reports)."""
    import torch
    from sparsernns_amd import _lib
    B, L = x.shape[:2]
    ref, rb, re_, rtr = cm.forward(x, bits, exp, trace=True)
    tops = [max(int(np.abs(t["xs_re"]).max()), int(np.abs(t["xs_im"]).max())) for t in rtr]
    xd = torch.from_numpy(x).cuda()
    plain_rungs = [_lib.lib.s5fxp_model_recurrence_kernel(eng._h, i) for i in range(nl)]
    bounds = [_lib.lib.s5fxp_model_recurrence_xmax(eng._h, i) for i in range(nl)]
    for flags in _flag_sets():
        y = torch.full((B, L, cm.d_out), -7, dtype=torch.int32, device="cuda")
        eng.enqueue(xd, bits, exp, y, B, L, flags=flags)
        st = eng.check_status()
        redo = bool(int(st[0]) & _lib.ST_REDO)
        assert st[2] == _lib.PATH_FUSED, (what, flags, st[:8])
        rungs = _words(eng, nl, 5)
        assert _words(eng, nl, 6) == [state_slots(P, n) for n in live], (what, flags)
        assert _words(eng, nl, 7) == [state_slots(P, n) for n in live], (what, flags)   # no compaction: whole streams
        if flags == _lib.FWD_EXACT:
            assert rungs == [5] * nl and not redo, (what, rungs)
        if flags == _lib.FWD_DEFER_REDO:
            assert rungs == plain_rungs, (what, rungs, plain_rungs)
            if all(t <= b for t, b in zip(tops, bounds)):
                assert not redo, (what, tops, bounds)
        if flags == 0:
            assert not redo, what      # self-contained: the gated exact kernels are part of the forward
        if not redo:
            got = y.cpu().numpy()
            assert np.array_equal(got, ref), (what, flags, np.count_nonzero(got != ref))
    return ref, rb, re_, rtr


def _live(eng, nl):
    from sparsernns_amd import _lib
    return [_lib.lib.s5fxp_model_live_states(eng._h, i) for i in range(nl)]


# ---- 1. path
@gpu
@pytest.mark.parametrize("ds", NEW_DS)
def test_new_shapes_run_the_fused_path(ds):
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    r = recipe(ds)
    assert fused_shape(r.dims["H"], r.dims["P"])
    assert _lib.lib.s5fxp_model_is_fast(r.eng._h) == 1
    fx = r.input(2, 130, seed=1)
    y = r.eng.forward(FxpArray(fx.data, fx.bits, fx.exp))
    assert int(r.eng.lane_status(0).cpu().numpy()[2]) == _lib.PATH_FUSED
    ref, rb, re_, _ = r.cm.forward(fx.data, fx.bits, fx.exp)
    assert (y.bits, y.exp) == (rb, re_) and np.array_equal(y.numpy(), ref)
    # the int16 rung the plan reports is the one the forward ran, on every state slot
    rungs = [_lib.lib.s5fxp_model_recurrence_kernel(r.eng._h, i) for i in range(r.nl)]
    assert all(k in (2, 3, 4) for k in rungs), rungs
    assert _words(r.eng, r.nl, 5) == rungs and _words(r.eng, r.nl, 6) == [r.dims["P"]] * r.nl


@gpu
def test_a_shape_outside_the_contract_stays_a_fallback():
    """dim_scale 0.375 (H = 72, P = 48: rows are not whole 16-byte vectors): generic kernels, the oracle's result."""
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model
    md, qc, dims = synth.make_model(dim_scale=0.375, calib_L=256, state_headroom_bits=1)
    assert (dims["H"], dims["P"]) == (72, 48)
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 0
    x = synth.make_input(2, 65, dims["d_in"], seed=2)
    fx = O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    y = eng.forward(FxpArray(fx.data, fx.bits, fx.exp))
    assert int(eng.lane_status(0).cpu().numpy()[2]) == _lib.PATH_GENERIC
    ref, rb, re_, _ = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp)
    assert (y.bits, y.exp) == (rb, re_) and np.array_equal(y.numpy(), ref)


# ---- 2. parity under the four flag sets, ragged lengths
@gpu
@pytest.mark.parametrize("ds", NEW_DS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", [1, 3, 65, 333])
def test_flag_sets_at_ragged_lengths(ds, B, L):
    r = recipe(ds)
    fx = r.input(B, L, seed=100 + L + B)
    _check_flags(r.eng, r.cm, r.nl, r.dims["P"], fx.data, fx.bits, fx.exp, _live(r.eng, r.nl), (ds, B, L))


@gpu
@pytest.mark.parametrize("ds", NEW_DS)
def test_state_overflow_takes_the_exact_kernels(ds):
    """Calibrated at scale 1, run at scale 6 (or the first larger scale at which the oracle's states leave 16 bits): the range
    check fires, ST_REDO comes back under DEFER_REDO, and the exact kernels -- gated inside the forward, or alone under
    S5FXP_FWD_EXACT -- give the oracle's result."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    r = recipe(ds)
    B, L = 2, 512
    for scale in (6.0, 12.0, 24.0, 48.0, 96.0):
        fx = r.input(B, L, seed=9, scale=scale)
        ref, _, _, rtr = r.cm.forward(fx.data, fx.bits, fx.exp, trace=True)
        if _top_state(rtr) > 32767:
            break
    assert _top_state(rtr) > 32767, "the case must overflow 16 bits to mean anything"
    eng = r.eng
    fxa = FxpArray(fx.data, fx.bits, fx.exp)
    y = eng.forward(fxa, check_status=False)
    assert np.array_equal(y.numpy(), ref)
    assert int(eng.status[0].item()) & _lib.ST_WIDE_STATE and not int(eng.status[0].item()) & _lib.ST_REDO
    y2 = torch.empty_like(y.data)
    eng.enqueue(fxa.data, fx.bits, fx.exp, y2, B, L, flags=_lib.FWD_DEFER_REDO)
    assert int(eng.status[0].item()) & _lib.ST_REDO
    eng.enqueue(fxa.data, fx.bits, fx.exp, y2, B, L, flags=_lib.FWD_EXACT)
    assert not int(eng.status[0].item()) & _lib.ST_REDO
    assert np.array_equal(y2.cpu().numpy(), ref)
    assert np.array_equal(eng.forward(fxa).numpy(), ref)
    # the traced forms of the exact kernels (self-contained traced forward: traced gate kernel + gated traced re-run)
    y3, tr = eng.forward(fxa, traces=True, check_status=False)
    assert np.array_equal(y3.numpy(), ref)
    for i in range(r.nl):
        for k, ck in TRACE_MAP.items():
            got = tr[i][k].cpu().numpy()
            assert np.array_equal(got, rtr[i][ck]), f"ds {ds} layer {i} {k}: {np.count_nonzero(got != rtr[i][ck])} mismatches"


# ---- 3. traces
@gpu
@pytest.mark.parametrize("ds", NEW_DS)
@pytest.mark.parametrize("B,L", [(2, 200), (3, 65), (1, 1)])
def test_every_trace_field_matches_the_oracle(ds, B, L):
    from sparsernns_amd.fxparray import FxpArray
    r = recipe(ds)
    fx = r.input(B, L, seed=5)
    ref, rb, re_, rtr = r.cm.forward(fx.data, fx.bits, fx.exp, trace=True)
    y, tr = r.eng.forward(FxpArray(fx.data, fx.bits, fx.exp), traces=True)
    exps = r.eng.layer_exponents()
    assert (y.bits, y.exp) == (rb, re_) and np.array_equal(y.numpy(), ref)
    for i in range(r.nl):
        assert exps[i]["residadd"] == rtr[i]["residadd_exp"], (i, exps[i])
        assert exps[i]["norm_output_raw"] == rtr[i]["pre_s5_exp"], (i, exps[i])
        for k, ck in TRACE_MAP.items():
            got = tr[i][k].cpu().numpy()
            assert got.shape == rtr[i][ck].shape
            assert np.array_equal(got, rtr[i][ck]), f"ds {ds} layer {i} {k}: {np.count_nonzero(got != rtr[i][ck])} mismatches"


# ---- 4. carry
@gpu
@pytest.mark.parametrize("ds", NEW_DS)
def test_three_chunks_carry_the_state_like_the_oracle(ds):
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    r = recipe(ds)
    B = 2
    sess = r.eng.stream(B)
    ref_state = np.zeros((r.nl, 2, B, r.dims["P"]), dtype=np.int32)
    for i, L in enumerate((64, 37, 130)):
        fx = r.input(B, L, seed=300 + i)
        ref, rb, re_, _ = r.cm.forward(fx.data, fx.bits, fx.exp, state=ref_state)   # updates ref_state in place
        y = sess.push(FxpArray(fx.data, fx.bits, fx.exp))
        assert (y.bits, y.exp) == (rb, re_)
        assert np.array_equal(y.numpy(), ref), f"chunk {i} (L={L})"
        assert np.array_equal(sess.state.cpu().numpy(), ref_state), f"carry after chunk {i}"
        assert int(r.eng.lane_status(0).cpu().numpy()[2]) == _lib.PATH_FUSED
    assert np.abs(ref_state).max() > 0


# ---- 5. groups
@gpu
@pytest.mark.parametrize("ds", NEW_DS)
def test_three_groups_in_one_call_equal_three_oracle_runs(ds):
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    r = recipe(ds)
    G, B, L = 3, 4, 203
    scales = (1.0, 0.25, 2.0)
    parts = [r.input(B, L, seed=70 + g, scale=scales[g]) for g in range(G)]
    bits, exp = parts[0].bits, parts[0].exp
    x = np.concatenate([p.data for p in parts])
    refs, res_exps = [], []
    ref_state = np.zeros((G, r.nl, 2, B, r.dims["P"]), dtype=np.int32)
    for g in range(G):
        ref, rb, re_, rtr = r.cm.forward(parts[g].data, bits, exp, trace=True, state=ref_state[g])
        refs.append(ref)
        res_exps.append([t["residadd_exp"] for t in rtr])
    assert len({tuple(e) for e in res_exps}) > 1       # the groups really choose different exponents
    y = r.eng.forward_batches(FxpArray(x, bits, exp), B)
    assert (y.bits, y.exp) == (rb, re_)
    assert np.array_equal(y.numpy(), np.concatenate(refs))
    st = r.eng.lane_status(0, G).cpu().numpy()
    for g in range(G):
        w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
        assert w[2] == _lib.PATH_FUSED
        assert [int(w[8 + 8 * i + 4]) for i in range(r.nl)] == res_exps[g], g
    # ... and the carry, group by group
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty((G * B, L, r.dims["d_out"]), dtype=torch.int32, device="cuda")
    s_in = torch.zeros((G, r.nl, 2, B, r.dims["P"]), dtype=torch.int32, device="cuda")
    s_out = torch.empty_like(s_in)
    eng = r.eng
    eng.run_ladder(lambda fl: eng.enqueue(xd, bits, exp, yd, B, L, flags=fl, groups=G, state_in=s_in, state_out=s_out), eng.check_status)
    assert np.array_equal(s_out.cpu().numpy(), ref_state)
    assert np.array_equal(yd.cpu().numpy(), np.concatenate(refs))


# ---- 6. float entry
@gpu
@pytest.mark.parametrize("ds", NEW_DS)
def test_float_entry_equals_the_three_step_route(ds):
    """s5fxp_model_forward_f32 against from_fp -> forward -> to_float: output bits, status words, carry; with and without the
    residual pass riding on the decoder (traced forwards keep it apart)."""
    from test_float_io import _float_input, _run
    from sparsernns_amd import _lib
    r = recipe(ds)
    eng = r.eng
    for B, L, kw in ((2, 130, {}), (3, 65, dict(carry=True)), (1, 3, dict(flags=_lib.FWD_DEFER_REDO)), (2, 64, dict(traced=True)),
                     (2, 70, dict(groups=2))):
        G = kw.get("groups", 1)
        xf = _float_input(eng, G * B, L, seed=L)
        a = _run(eng, xf, eng.inp_bits, eng.inp_exp, B, L, True, **kw)
        b = _run(eng, xf, eng.inp_bits, eng.inp_exp, B, L, False, **kw)
        assert np.array_equal(a[0], b[0]), (ds, B, L, kw, np.count_nonzero(a[0] != b[0]))
        assert np.array_equal(a[1], b[1]), (ds, B, L, kw)
        assert a[1][2] == _lib.PATH_FUSED
        if kw.get("traced"):
            for ta, tb in zip(a[2], b[2]):
                for k in ta:
                    assert np.array_equal(ta[k], tb[k]), (ds, k)
        if kw.get("carry"):
            assert np.array_equal(a[3], b[3])
        # and the three-step route is the oracle's
        fx = O.from_fp(xf, eng.inp_bits, eng.inp_exp, True, O.FLOOR)
        for g in range(G):
            ref = r.cm.forward(fx.data[g * B:(g + 1) * B], fx.bits, fx.exp)[0]
            want = O.to_float(ref, eng.out_exp) if hasattr(O, "to_float") else (ref.astype(np.float64) / 2.0 ** eng.out_exp).astype(np.float32)
            assert np.array_equal(b[0][g * B:(g + 1) * B], np.asarray(want, dtype=np.float32).view(np.int32)), (ds, B, L, kw, g)


# ---- 7. contract families, 8. pad lanes
def _families(ds):
    import contract_models as CM
    return {
        "F1_full": lambda: CM.f1_full_range(ds), "F2_rails": lambda: CM.f2_rails(ds), "F3_D16": lambda: CM.f3_wide_D(ds),
        "F3_Bu24": lambda: CM.f3_wide_bu(ds), "F3_out32": lambda: CM.f3_wide_out(ds),
        "F5_y+4": lambda: CM.f5_pk16(ds, 4), "F5_y+3_l-y14": lambda: CM.f5_pk16(ds, 3, 14), "F5_y+3_l-y15": lambda: CM.f5_pk16(ds, 3, 15),
    }


_CASES = {}


def _case(ds, fam):
    if (ds, fam) not in _CASES:
        _CASES[(ds, fam)] = _families(ds)[fam]()
    return _CASES[(ds, fam)]


def _run_contract(c, kind, B, L, seed=0, traced=True):
    """One (model, input): the four flag sets, the ladder, a traced run with every field and the per-layer exponents."""
    import contract_models as CM
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    nl, P = c.dims["n_layers"], c.dims["P"]
    x, bits, exp = CM.input_for(c, kind, B, L, seed=seed)
    eng = c.engine()
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1, c.name
    live = [len(v) for v in CM.export_live(c.export(), nl)]
    assert _live(eng, nl) == live
    ref, rb, re_, rtr = _check_flags(eng, c.c_oracle(), nl, P, x, bits, exp, live, (c.name, kind))
    y = eng.forward(FxpArray(x, bits, exp))
    assert (y.bits, y.exp) == (rb, re_) and np.array_equal(y.numpy(), ref), (c.name, kind)
    exps = eng.layer_exponents()
    for i in range(nl):   # the untraced forward's exponents: where a pad lane in a maximum would show
        assert exps[i]["residadd"] == rtr[i]["residadd_exp"], (c.name, kind, i, exps[i])
        assert exps[i]["norm_output_raw"] == rtr[i]["pre_s5_exp"], (c.name, kind, i, exps[i])
    if traced:
        y2, tr = eng.forward(FxpArray(x, bits, exp), traces=True)
        assert np.array_equal(y2.numpy(), ref)
        exps = eng.layer_exponents()
        for i in range(nl):
            assert exps[i]["residadd"] == rtr[i]["residadd_exp"], (c.name, kind, i)
            assert exps[i]["norm_output_raw"] == rtr[i]["pre_s5_exp"], (c.name, kind, i)
            for k, ck in TRACE_MAP.items():
                got = tr[i][k].cpu().numpy()
                assert np.array_equal(got, rtr[i][ck]), f"{c.name} {kind} layer {i} {k}: {np.count_nonzero(got != rtr[i][ck])} mismatches"
    return eng


CONTRACT_RUNS = [
    ("F1_full", ("ndns", "pos_full", "flip", "impulse_first"), 2, 65),
    ("F1_full", ("neg_full",), 3, 333),
    ("F2_rails", ("ndns", "flip", "neg_full"), 2, 333),
    ("F2_rails", ("pos_full", "impulse_first"), 2, 65),
    ("F3_D16", ("ndns", "flip", "pos_full"), 2, 64),
    ("F3_Bu24", ("ndns", "flip"), 2, 130),
    ("F3_out32", ("ndns", "pos_full"), 2, 65),
    ("F5_y+4", ("ndns", "flip"), 3, 333),
    ("F5_y+3_l-y14", ("ndns", "flip"), 3, 333),
    ("F5_y+3_l-y15", ("ndns", "flip"), 3, 333),
]


@gpu
@pytest.mark.parametrize("ds", NEW_DS)
@pytest.mark.parametrize("fam,inputs,B,L", [pytest.param(*r, id=f"{r[0]}-L{r[3]}") for r in CONTRACT_RUNS])
def test_contract_families_match_the_oracle(ds, fam, inputs, B, L):
    from sparsernns_amd import _lib
    c = _case(ds, fam)
    assert fused_shape(c.dims["H"], c.dims["P"])
    for kind in inputs:
        eng = _run_contract(c, kind, B, L, seed=L, traced=not fam.startswith("F5_") or kind == "ndns")
    if fam == "F3_Bu24":   # 24-bit Bu cannot travel as int16: no int16 rung
        assert all(_lib.lib.s5fxp_model_recurrence_kernel(eng._h, i) in (1, 5) for i in range(c.dims["n_layers"]))


@gpu
@pytest.mark.parametrize("ds", NEW_DS)
@pytest.mark.parametrize("fam", ["F1_full", "F2_rails", "F5_y+4"])
@pytest.mark.parametrize("kind", ["impulse_last", "mixed", "zeros"])
def test_pad_lanes_stay_out_of_the_maxima(ds, fam, kind):
    """An impulse in the last frame, one full-scale sequence among zero ones, and all zeros: the maxima behind every
    compute_best exponent are then set by few elements (or none), so a pad lane of the half empty tile that entered one -- a
    stale LDS word, a neighbouring row's channel -- would move an exponent.  _run_contract compares the BatchNorm and residual
    exponents of every layer with the oracle's on the untraced and the traced forward, and every trace field."""
    c = _case(ds, fam)
    for B, L in ((3, 65), (2, 1), (2, 130)):
        _run_contract(c, kind, B, L, seed=B + L)
    r = recipe(ds)   # and on the recipe's own model
    import contract_models as CM
    x = CM.make_input(kind, 3, 97, r.dims["d_in"], r.qc["encoder"]["inp_bits"], seed=4)
    bits, exp = r.qc["encoder"]["inp_bits"], r.qc["encoder"]["inp_exp"]
    ref, rb, re_, rtr = _check_flags(r.eng, r.cm, r.nl, r.dims["P"], x, bits, exp, _live(r.eng, r.nl), (ds, kind))
    from sparsernns_amd.fxparray import FxpArray
    y = r.eng.forward(FxpArray(x, bits, exp))
    assert np.array_equal(y.numpy(), ref)
    exps = r.eng.layer_exponents()
    for i in range(r.nl):
        assert exps[i]["residadd"] == rtr[i]["residadd_exp"] and exps[i]["norm_output_raw"] == rtr[i]["pre_s5_exp"], (ds, kind, i, exps[i])


# ---- the pair kernel's other feed (the int32 K stream: S5FXP_PAIR_GLOBAL is read once per process)
@gpu
@pytest.mark.parametrize("ds", NEW_DS)
def test_pair_kernel_fed_from_global_memory(ds):
    h = recipe(ds).headroom
    code = ("import numpy as np\n"
            "from oracle import cref, fxp_oracle as O\n"
            "from sparsernns_amd import _lib, synth\n"
            "from sparsernns_amd.fxparray import FxpArray\n"
            "from sparsernns_amd.fxpmodel import build_regression_model\n"
            f"md, qc, dims = synth.make_model({ds}, calib_L=256, state_headroom_bits={h})\n"
            "model = build_regression_model(md, qc, dims['n_layers'])\n"
            "eng = model.engine()\n"
            "assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1\n"
            "want = [_lib.lib.s5fxp_model_recurrence_kernel(eng._h, i) for i in range(3)]\n"
            "assert 4 not in want, want\n"
            "x = synth.make_input(3, 333, dims['d_in'], seed=4)\n"
            "fx = O.from_fp(x, qc['encoder']['inp_bits'], qc['encoder']['inp_exp'], True, O.FLOOR)\n"
            "y = eng.forward(FxpArray(fx.data, fx.bits, fx.exp))\n"
            "assert np.array_equal(y.numpy(), cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp)[0])\n"
            "print('rungs', want, 'ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, S5FXP_PAIR_GLOBAL="1"))
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- 9. full size
@gpu
@pytest.mark.parametrize("ds", NEW_DS)
def test_full_size_batch_matches_the_oracle(ds):
    """B = 32, L = 4096 through the in-flight runner (DEFER_REDO with the engine's ladder) and through Engine.forward, against
    the OpenMP C oracle."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import InflightRunner
    from sparsernns_amd.fxparray import FxpArray
    r = recipe(ds)
    B, L = 32, 4096
    eng = r.eng
    runner = InflightRunner(eng, depth=1)
    fx = r.input(B, L, seed=1000)
    x = torch.from_numpy(fx.data).cuda()
    y = torch.empty((B, L, r.dims["d_out"]), dtype=torch.int32, device="cuda")
    runner.submit(x, fx.bits, fx.exp, y, B, L)
    runner.drain()
    ref, rb, re_, _ = r.cm.forward(fx.data, fx.bits, fx.exp)
    got = y.cpu().numpy()
    assert np.array_equal(got, ref), f"{np.count_nonzero(got != ref)} of {ref.size} outputs differ"
    assert int(eng.lane_status(0).cpu().numpy()[2]) == _lib.PATH_FUSED
    y1 = eng.forward(FxpArray(x, fx.bits, fx.exp))
    assert (y1.bits, y1.exp) == (rb, re_) and np.array_equal(y1.numpy(), ref)


# ---- the int16 rungs without the direct sigmoid table
@gpu
@pytest.mark.parametrize("ds", NEW_DS)
def test_segment_table_sigmoid_on_the_int16_rungs(ds):
    """out2's output exponent lowered to 8: the sigmoid input keeps 16 - (8 - 6) = 14 bits, more than the direct table's 12, so
    the gate kernel on the int16 rungs takes the (segment, remainder) table -- k_cgate_p<.., S16, !DIRECT> with and without
    PAIR -- which the recipe's own exponents never select."""
    import copy
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxpmodel import build_regression_model
    from test_variant_matrix import _launched, _profiled
    base = recipe(ds)
    qc = copy.deepcopy(base.qc)
    assert qc["blocks"]["out2"]["out_exp"] > 8
    qc["blocks"]["out2"]["out_exp"] = 8
    model = build_regression_model(base.md, qc, base.nl)
    cm = cref.CModel(model.export())
    eng = model.engine()
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    B, L = 3, 130
    x = synth.make_input(B, L, base.dims["d_in"], seed=21)
    fx = O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    _check_flags(eng, cm, base.nl, base.dims["P"], fx.data, fx.bits, fx.exp, _live(eng, base.nl), (ds, "out_exp 8"))
    xd = torch.from_numpy(fx.data).cuda()
    y = torch.empty((B, L, base.dims["d_out"]), dtype=torch.int32, device="cuda")
    for flags, pair in ((_lib.FWD_DEFER_REDO, "true"), (_lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, "false")):
        kernels = _profiled(lambda: eng.enqueue(xd, fx.bits, fx.exp, y, B, L, flags=flags))[0]
        gates = [a for a, _ in _launched(kernels, "k_cgate_p") if a[2] == "false" and a[6] == "false"]
        if pair == "true" and _words(eng, base.nl, 5) != [4] * base.nl and _words(eng, base.nl, 5) != [3] * base.nl:
            continue   # (the model does not reach the pair rung: nothing to name)
        assert gates and all(a[3] == "true" and a[4] == "false" and a[7] == pair and a[8] == "false" for a in gates), gates
