"""The fused MFMA path on models from the whole of what s5fxp_fast.hpp fast_eligible admits (tests/contract_models.py), not only
the recipe's corner: full-range and railed int8 weights, a 16-bit D, 24-bit Bu, a 32-bit decoder output, every live-state count
at the compaction rules' boundaries, and gate exponents that stress the PK16 epilogue -- fed all-zero, full-scale, sign-flipping
and impulse inputs.  Output, (bits, exp), per-layer exponents and every trace must be the C oracle's bit for bit, under the four
forward flag sets, and the status words / kernel names must show each case ran where it was meant to.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import contract_models as CM

TRACE_MAP = dict(pre_s5="pre_s5", u="u", Bu_re="bu_re", Bu_im="bu_im", xs_re="xs_re", xs_im="xs_im", ys="ys",
                 out2="out2", out2_sigmoid="sigmoid", post_GLU="post_glu", residadd="residadd")
CFG1 = dict(dim_scale=0.5, calib_L=1024, state_headroom_bits=1)   # bench.py's configs[1] model


def _flag_sets():
    from sparsernns_amd import _lib
    return (_lib.FWD_DEFER_REDO, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, 0, _lib.FWD_EXACT)


def _words(eng, nl, k, lane=0):
    return [int(v) for v in eng.lane_status(lane).cpu().numpy()[8 + k:8 + 8 * nl:8]]


def _profiled(fn):
    from test_variant_matrix import _profiled as p
    return p(fn)


def _gates(kernels):
    """Template arguments of the untraced, non-WIDE k_cgate_p launches (a[8] = PK16)."""
    from test_variant_matrix import _launched
    return [a for a, _ in _launched(kernels, "k_cgate_p") if a[2] == "false" and a[6] == "false"]


def _run_case(c, kind, B, L, seed=0, traced=True):
    """Every check of one (model, input): the four flag sets with their status words, the ladder's forward, and a traced run.
    Returns the per-flag-set (redo, rungs) and the profiled kernels of the DEFER_REDO forward."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray

    nl, P = c.dims["n_layers"], c.dims["P"]
    x, bits, exp = CM.input_for(c, kind, B, L, seed=seed)
    cm = c.c_oracle()
    ref, rb, re_, rtr = cm.forward(x, bits, exp, trace=True)
    eng = c.engine()
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1, c.name
    live = [len(v) for v in CM.export_live(c.export(), nl)]
    assert [_lib.lib.s5fxp_model_live_states(eng._h, i) for i in range(nl)] == live
    xd = torch.from_numpy(x).cuda()
    seen, kernels = {}, None
    for flags in _flag_sets():
        y = torch.empty((B, L, c.dims["d_out"]), dtype=torch.int32, device="cuda")
        run = lambda: eng.enqueue(xd, bits, exp, y, B, L, flags=flags)
        if flags == _lib.FWD_DEFER_REDO:
            kernels = _profiled(run)[0]
        else:
            run()
        st = eng.lane_status(0).cpu().numpy()
        redo = bool(int(eng.check_status()[0]) & _lib.ST_REDO)
        assert st[2] == _lib.PATH_FUSED, (c.name, st[:8])
        rungs = _words(eng, nl, 5)
        slots = _words(eng, nl, 6)
        assert slots == [CM.compact_slots(n, P) for n in live], (c.name, flags, slots, live)
        stream = _words(eng, nl, 7)
        assert stream == [CM.stream_slots(n, P, r in (2, 4)) for n, r in zip(live, rungs)], (c.name, flags, stream, rungs)
        if flags == _lib.FWD_EXACT:
            assert rungs == [5] * nl and not redo
        if not redo:
            assert np.array_equal(y.cpu().numpy(), ref), (c.name, kind, flags, np.count_nonzero(y.cpu().numpy() != ref))
        seen[flags] = (redo, rungs)
    y = eng.forward(FxpArray(x, bits, exp))
    assert (y.bits, y.exp) == (rb, re_)
    assert np.array_equal(y.numpy(), ref), (c.name, kind)
    if traced:
        y2, tr = eng.forward(FxpArray(x, bits, exp), traces=True)
        assert np.array_equal(y2.numpy(), ref)
        exps = eng.layer_exponents()
        for i in range(nl):
            assert exps[i]["residadd"] == rtr[i]["residadd_exp"], (c.name, i)
            for k, ck in TRACE_MAP.items():
                got = tr[i][k].cpu().numpy()
                assert np.array_equal(got, rtr[i][ck]), f"{c.name} {kind} layer {i} {k}: {np.count_nonzero(got != rtr[i][ck])} mismatches"
    return seen, kernels


# (case, inputs, B, L): a fitting subset of the inputs per family
RUNS = [
    ("F1_full_ds0.5", ("zeros", "pos_full", "flip", "impulse_first", "impulse_last"), 2, 65),
    ("F1_full_ds0.5", ("neg_full", "mixed"), 4, 333),
    ("F1_full_ds1.0", ("pos_full", "flip", "impulse_last"), 2, 63),
    ("F1_full_ds1.0", ("mixed",), 3, 64),
    ("F2_rails_ds0.5", ("ndns", "flip", "neg_full", "impulse_last"), 2, 333),
    ("F2_rails_ds1.0", ("ndns", "pos_full", "impulse_first"), 2, 65),
    ("F3_D16_ds0.5", ("ndns", "flip", "pos_full"), 2, 64),
    ("F3_D16_ds1.0", ("ndns", "neg_full"), 2, 65),
    ("F3_Bu24_ds0.5", ("ndns", "flip"), 2, 333),
    ("F3_Bu24_ds1.0", ("ndns",), 2, 63),
    ("F3_out32_ds0.5", ("ndns", "pos_full"), 2, 65),
    ("F3_out32_ds1.0", ("flip",), 2, 64),
    ("F3_dims257x1_ds0.5", ("ndns", "flip"), 2, 65),
    ("F3_dims288x257_ds0.5", ("ndns", "pos_full"), 2, 64),
    ("F3_dims257x272_ds0.5", ("ndns", "impulse_last"), 2, 1),
] + [(n, ("ndns", "pos_full"), 2, 65) for n in CM.BUILDERS if n.startswith("F4_")] + [
    (n, ("ndns", "flip", "mixed"), 3, 333) for n in CM.BUILDERS if n.startswith("F5_")]


@pytest.mark.parametrize("name,inputs,B,L", [pytest.param(*r, id=f"{r[0]}-L{r[3]}") for r in RUNS])
def test_contract_model_matches_oracle(name, inputs, B, L):
    c = CM.case(name)
    nl = c.dims["n_layers"]
    for kind in inputs:
        seen, kernels = _run_case(c, kind, B, L, seed=L, traced=not name.startswith("F5_") or kind == "ndns")
        from sparsernns_amd import _lib
        defer_redo, defer_rungs = seen[_lib.FWD_DEFER_REDO]
        if name.startswith("F3_Bu"):
            # Bu of 24 bits cannot travel as int16: the B projection writes the int32 stream (SM 0) and no int16 rung runs
            from test_variant_matrix import _launched
            sm = [a[3] for a, _ in _launched(kernels, "k_bproj_p")]
            assert sm and all(s == "0" for s in sm), sm
            assert all(r in (1, 5) for r in defer_rungs), defer_rungs
        if name.startswith("F5_"):
            # the PK16 epilogue runs on the untraced top-rung forward (pk16 needs s16, the direct table, !traces) ...
            gates = _gates(kernels)
            want = "false" if "l-y15" in name else "true"
            assert gates and all(a[8] == want for a in gates), (name, gates)
            # ... and that forward is the one whose output was compared: it completed without a step down
            assert not defer_redo and defer_rungs == [4] * nl, (name, kind, defer_rungs)


def test_long_full_range_sequence():
    """One N-DNS-length clip (3751 frames) on the full-range model."""
    c = CM.case("F1_full_ds0.5")
    _run_case(c, "ndns", 1, 3751, traced=False)


def test_grouped_launch_with_zero_and_full_scale_groups():
    """G = 3 in one set of launches: an all-zero group, a full-scale group and an ordinary group, each its own oracle run."""
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray

    c = CM.case("F1_full_ds0.5")
    B, L = 2, 203
    parts = [CM.input_for(c, k, B, L, seed=7)[0] for k in ("zeros", "pos_full", "ndns")]
    cm = c.c_oracle()
    refs, exps = [], []
    for p in parts:
        r, rb, re_, rtr = cm.forward(p, c.in_bits, c.in_exp, trace=True)
        refs.append(r)
        exps.append([t["residadd_exp"] for t in rtr])
    eng = c.engine()
    y = eng.forward_batches(FxpArray(np.concatenate(parts), c.in_bits, c.in_exp), B)
    assert (y.bits, y.exp) == (rb, re_)
    got = y.numpy()
    for g in range(3):
        assert np.array_equal(got[g * B:(g + 1) * B], refs[g]), g
    st = eng.lane_status(0, 3).cpu().numpy()
    for g in range(3):
        w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
        assert w[2] == _lib.PATH_FUSED
        assert [int(w[8 + 8 * i + 4]) for i in range(c.dims["n_layers"])] == exps[g], g


def _boundary(base: str, tag: str, edit):
    c = CM.copy_case(CM.case(base), f"{base}:{tag}")
    edit(c)
    return c


def _set_entry(c, field, value_float):
    for i in range(c.dims["n_layers"]):
        c.md["encoder"][f"layers_{i}"]["mixer"][field][2] = value_float


@pytest.mark.parametrize("which", ["B_bar", "D", "d_in"])
def test_contract_boundary_pairs(which):
    """Just inside fast_eligible the fused path runs, just outside the generic one; both equal the oracle."""
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray

    if which == "B_bar":
        # the 8-bit B_bar with an entry at -128 against the 9-bit one with that entry at -129
        def edit(v):
            def f(c):
                w = c.qc["blocks"]["ssm"]["weights"]
                w["B_re"]["bits"] = 8 if v >= -128 else 9
                e = w["B_re"]["exp"]
                for i in range(c.dims["n_layers"]):
                    mx = c.md["encoder"][f"layers_{i}"]["mixer"]
                    coef = CM._bbar_coef(mx)
                    b = (v / 2.0 ** e) / complex(coef[3])   # B_bar[3, 0] = v / 2^e (re), 0 (im)
                    mx["B"][3, 0] = (b.real, b.imag)
            return f
        pair = [_boundary("F1_full_ds0.5", "B-128", edit(-128.0)), _boundary("F1_full_ds0.5", "B-129", edit(-129.0))]
        ex = [c.export()["params"]["encoder"]["layers_0"]["mixer"]["B_real"] for c in pair]
        assert int(np.min(ex[0])) == -128 and int(ex[0][3, 0]) == -128 and int(ex[1][3, 0]) == -129
    elif which == "D":
        def edit(bits):
            def f(c):
                w = c.qc["blocks"]["ssm"]["weights"]["D"]
                w["bits"] = bits
                for i in range(c.dims["n_layers"]):
                    c.md["encoder"][f"layers_{i}"]["mixer"]["D"][5] = CM.RAIL
            return f
        pair = [_boundary("F3_D16_ds0.5", "D16", edit(16)), _boundary("F3_D16_ds0.5", "D17", edit(17))]
        ex = [c.export()["params"]["encoder"]["layers_0"]["mixer"]["D"] for c in pair]
        assert int(np.max(ex[0])) == 32767 and int(np.max(ex[1])) == 65535
    else:
        pair = [CM.f3_dims(288, 257), CM.f3_dims(289, 257)]
        # fast_eligible admits d_out up to 288, but model creation refuses more than 272 output channels (the generic
        # kernels' column budget, s5fxp_api.hip validate): an error, never a silent fallback
        with pytest.raises(NotImplementedError):
            CM.f3_dims(257, 273).engine()
    want_fast = [1, 0]
    for c, fast in zip(pair, want_fast):
        x, bits, exp = CM.input_for(c, "ndns", 2, 65, seed=1)
        ref, rb, re_, _ = c.c_oracle().forward(x, bits, exp)
        eng = c.engine()
        assert _lib.lib.s5fxp_model_is_fast(eng._h) == fast, (which, c.name)
        y = eng.forward(FxpArray(x, bits, exp))
        assert int(eng.lane_status(0).cpu().numpy()[2]) == (_lib.PATH_FUSED if fast else _lib.PATH_GENERIC)
        assert (y.bits, y.exp) == (rb, re_) and np.array_equal(y.numpy(), ref), c.name


def test_bench_model_keeps_its_path():
    """bench.py's configs[1] model (dim 0.5 w8a16, state headroom 1): the fused path, the LDS-fed pair rung on every layer,
    32 compacted state slots with live-pair streams, and the 32-frame PK16 gate epilogue with the direct sigmoid table -- the
    path recorded on the parent commit."""
    import torch
    from oracle import cref
    from sparsernns_amd import _lib, synth
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = synth.make_model(**CFG1)
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    nl = dims["n_layers"]
    B, L = 4, 333
    x = synth.make_input(B, L, dims["d_in"], seed=2)
    from oracle import fxp_oracle as O
    fx = O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    ref = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp)[0]
    y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
    xd = torch.from_numpy(fx.data).cuda()
    kernels = _profiled(lambda: eng.enqueue(xd, fx.bits, fx.exp, y, B, L, flags=_lib.FWD_DEFER_REDO))[0]
    st = eng.lane_status(0).cpu().numpy()
    assert not (int(eng.check_status()[0]) & _lib.ST_REDO)
    assert np.array_equal(y.cpu().numpy(), ref)
    assert st[2] == _lib.PATH_FUSED
    live = [_lib.lib.s5fxp_model_live_states(eng._h, i) for i in range(nl)]
    assert _words(eng, nl, 5) == [4] * nl
    assert _words(eng, nl, 6) == [32] * nl
    assert _words(eng, nl, 7) == [CM.stream_slots(n, dims["P"], True) for n in live]
    gates = _gates(kernels)
    assert gates and all(a[3] == "true" and a[4] == "true" and a[5] == "32" and a[8] == "true" and a[9] == "false"
                         for a in gates), gates
