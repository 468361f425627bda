"""The contract models of tests/contract_models.py on the CPU: each builder must produce what it claims (rails, live sets,
PK16 hazards, wide states), and the NumPy and C oracles must agree on all of them bit for bit -- at the rails the two
restatements are stretched furthest, and this is the one check of them there that runs without a GPU."""
import numpy as np
import pytest

import contract_models as CM
from oracle import fxp_oracle as O

EIGHT_BIT = (("mixer", "B_real"), ("mixer", "B_imag"), ("mixer", "C_real"), ("mixer", "C_imag"), ("out2", "weight"))


def _matrices(export, n_layers):
    p = export["params"]
    yield "encoder", np.asarray(p["encoder"]["encoder"]["weight"])
    yield "decoder", np.asarray(p["decoder"]["weight"])
    for i in range(n_layers):
        for grp, k in EIGHT_BIT:
            yield f"layers_{i}.{k}", np.asarray(p["encoder"][f"layers_{i}"][grp][k])


@pytest.mark.parametrize("name", ["F2_rails_ds0.5", "F2_rails_ds1.0"])
def test_rails_sit_in_every_edge_and_tile(name):
    c = CM.case(name)
    ex = c.export()
    for what, w in _matrices(ex, c.dims["n_layers"]):
        R, C = w.shape
        parts = [w[0], w[-1], w[:, 0], w[:, -1]]
        parts += [w[:, j:j + 32] for j in range(0, C, 32)] + [w[j:j + 32] for j in range(0, R, 32)]
        for k, part in enumerate(parts):
            assert part.min() == -128 and part.max() == 127, f"the case must put both rails in {what} part {k} to mean anything"
    for i in range(c.dims["n_layers"]):
        D = np.asarray(ex["params"]["encoder"][f"layers_{i}"]["mixer"]["D"])
        assert D.min() == -128 and D.max() == 127


@pytest.mark.parametrize("ds", [0.5, 1.0])
def test_full_range_model_spans_int8_with_every_state_live(ds):
    c = CM.case(f"F1_full_ds{ds}")
    ex = c.export()
    nl, P = c.dims["n_layers"], c.dims["P"]
    assert [len(v) for v in CM.export_live(ex, nl)] == [P] * nl
    ms = [ex["params"]["encoder"][f"layers_{i}"]["mixer"] for i in range(nl)]   # one exponent per tensor over the layers
    assert max(max(int(np.abs(m["B_real"]).max()), int(np.abs(m["B_imag"]).max())) for m in ms) >= 120
    assert min(int(np.min(m["C_real"])) for m in ms) == -128 and min(int(np.min(m["D"])) for m in ms) == -128
    for m in ms:   # beyond anything the recipe holds (|w| <= 93), in every layer
        assert max(int(np.abs(m["B_real"]).max()), int(np.abs(m["B_imag"]).max())) > 93
    assert int(ex["params"]["encoder"]["encoder"]["weight"].min()) == -128


def test_wide_corners_hold_what_they_claim():
    c = CM.case("F3_D16_ds0.5")
    D = np.asarray(c.export()["params"]["encoder"]["layers_0"]["mixer"]["D"])
    assert D.min() == -32768 and D.max() == 32767
    q = CM.case("F3_Bu24_ds0.5").export()["qconfig"]["encoder"]["layers_0"]["mixer"]
    assert q["Bu_re_bits"] == q["Bu_im_bits"] == 24
    sh = q["Bu_re_exp"] - q["x_re_exp"]
    assert 24 - sh > 16, "Bu must not provably fit int16 at the state exponent (select_rung s16) to mean anything"
    e = CM.case("F3_out32_ds0.5").export()["qconfig"]
    assert e["decoder"]["out_bits"] == 32 and e["encoder"]["encoder"]["bias_bits"] > 16
    assert e["encoder"]["layers_0"]["out2"]["bias_bits"] > 16
    for name, (di, do) in (("F3_dims257x1_ds0.5", (257, 1)), ("F3_dims288x257_ds0.5", (288, 257)),
                           ("F3_dims257x272_ds0.5", (257, 272))):
        assert CM.case(name).export()["params"]["encoder"]["encoder"]["weight"].shape[0] == di
        assert CM.case(name).export()["params"]["decoder"]["weight"].shape[1] == do


@pytest.mark.parametrize("name", [n for n in CM.BUILDERS if n.startswith("F4_")])
def test_live_sets_are_the_design(name):
    c = CM.case(name)
    n, P, nl = c.meta["n_live"], c.dims["P"], c.dims["n_layers"]
    live = CM.export_live(c.export(), nl)
    for i in range(nl):
        want = CM.live_rows(P, n, CM.PLACES[i % 3])
        assert len(want) == n and len(set(want.tolist())) == n
        assert np.array_equal(live[i], want), (i, live[i], want)
    if 0 < n < P:
        assert live[1][-1] == P - 1   # the trailing block holds the layer's last state
    # the compaction rule on these counts: every boundary of Pc = max(32, ceil32(n)) <= P / 2 and the live pairs
    assert CM.compact_slots(n, P) == (P if n > P // 2 else 32 if n <= 32 else 64)
    assert CM.stream_slots(n, P, True) in (max(2, n + n % 2), CM.compact_slots(n, P))
    # the live rows are not trivially small: a full-range calibration left them
    if n >= 31:
        b = np.asarray(c.export()["params"]["encoder"]["layers_0"]["mixer"]["B_real"])[live[0]]
        assert np.abs(b).max() >= 64


def _layer_traces(c, kind, B=2, L=64, seed=3):
    x, bits, exp = CM.input_for(c, kind, B, L, seed=seed)
    it = {}
    c.numpy_oracle()(O.Fx(x, bits, exp), it)
    return O.flatten_intermediates(it)


@pytest.mark.parametrize("name", [n for n in CM.BUILDERS if n.startswith("F5_")])
def test_pk16_hazards_occur(name):
    """2 cx leaves int16 while 2 cx + D u does not: a clamp on the intermediate 2 cx would change y."""
    c = CM.case(name)
    q = c.export()["qconfig"]["encoder"]["layers_0"]
    assert q["sigmoid"]["x_exp"] == 6   # the reference's cap on the sigmoid input exponent
    if c.meta["l_minus_y"] is not None:
        assert q["multgate"]["l_exp"] - q["mixer"]["y_exp"] == c.meta["l_minus_y"]
    for kind in ("ndns", "flip", "mixed"):
        fl = _layer_traces(c, kind, B=3, L=333, seed=333)
        hits = 0
        for i in range(c.dims["n_layers"]):
            cx2 = fl[f"layers_{i}.mixer.Cxs2"].data.astype(np.int64)
            du = fl[f"layers_{i}.mixer.Du"].data.astype(np.int64)
            hits += int(((np.abs(cx2) > 32767) & (np.abs(cx2 + du) <= 32767)).sum())
        assert hits > 0, f"{name} on {kind} must produce |2cx| > 32767 with |2cx + Du| <= 32767 to mean anything"


@pytest.mark.parametrize("name", ["F1_full_ds0.5", "F1_full_ds1.0", "F2_rails_ds0.5"])
def test_states_pass_16_bits(name):
    fl = _layer_traces(CM.case(name), "pos_full")
    top = max(int(np.abs(fl[f"layers_{i}.mixer.{k}"].data).max()) for i in range(3) for k in ("xs_re", "xs_im"))
    assert top > 32767, "the full-range model must take states past 16 bits to mean anything"


ORACLE_NAMES = dict(pre_s5="pre_s5", u="mixer.u", bu_re="mixer.Bu_re", bu_im="mixer.Bu_im", xs_re="mixer.xs_re",
                    xs_im="mixer.xs_im", ys="mixer.ys", out2="out2", sigmoid="out2_sigmoid", post_glu="post_GLU",
                    residadd="residadd")


@pytest.mark.parametrize("name", list(CM.BUILDERS))
def test_numpy_and_c_oracles_agree(name):
    c = CM.case(name)
    m = c.numpy_oracle()
    cm = c.c_oracle()
    for kind in CM.INPUTS:
        x, bits, exp = CM.input_for(c, kind, 2, 23, seed=4)
        it = {}
        y = m(O.Fx(x, bits, exp), it)
        yc, yb, ye, tr = cm.forward(x, bits, exp, trace=True)
        assert (yb, ye) == (y.bits, y.exp), (name, kind)
        assert np.array_equal(yc, y.data), (name, kind)
        fl = O.flatten_intermediates(it)
        for i in range(c.dims["n_layers"]):
            assert tr[i]["pre_s5_exp"] == fl[f"layers_{i}.pre_s5"].exp and tr[i]["residadd_exp"] == fl[f"layers_{i}.residadd"].exp
            for ck, ok in ORACLE_NAMES.items():
                assert np.array_equal(tr[i][ck], fl[f"layers_{i}.{ok}"].data), (name, kind, i, ck)


def test_inputs_are_what_they_claim():
    hi, lo = 32767, -32768
    x = CM.make_input("flip", 2, 5, 7, 16)
    assert set(np.unique(x)) == {hi, lo} and np.all(x[:, 1:, 0] == -x[:, :-1, 0] - 1)
    x = CM.make_input("impulse_last", 2, 5, 7, 16)
    assert not x[:, :-1].any() and np.all(np.abs(x[:, -1]) >= hi)
    x = CM.make_input("mixed", 3, 5, 7, 16)
    assert np.all(x[0] == hi) and not x[1:].any()
    assert not CM.make_input("zeros", 1, 3, 4, 16).any()
