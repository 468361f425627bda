"""The float model with the integer recurrence's per-step rounding and with quantised weights.

The reference of every step-mode test is ``floatmodel.fq_scan``, the float64 statement of the step
    xr' = (F(ar xr, er) - F(ai xi, er)) + F(br, er),   xi' = (F(ar xi, ei) + F(ai xr, ei)) + F(bi, ei),
F(v, e) = floor(v 2^e) 2^-e of the exact v.  On the CPU it is pinned to ``oracle.fxp_oracle.scan`` integer for integer; on the
GPU ``s5fxp_fq_scan_c64`` and the model entries in step mode must give it bit for bit (zeros of either sign count as equal).
Every input stays inside the domain (|x| 2^e < 2^24, no subnormal v 2^e), which the tests assert.  The stages around the
recurrence hold the sandwich of tests/test_float_fq.py, whose helpers and cached engines this file shares.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import float_model_ref as R
import test_float_fq as T
from sparsernns_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
TRIPLES = [(15, 15, 14), (15, 12, 15), (7, 7, 7), (7, 12, 9)]  # exponents of (A, Bu, x); A has 16 bits at 15, 8 bits at 7


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def grid_problem(B, L, P, ea, eb, ex, seed):
    """Integer poles of radius 0.5 .. 0.95 and integer Bu of fewer than 2^10 LSBs AT THE STATE'S exponent: with
    sum |A|^k <= 20 per component pair the states stay far below 2^24 and |A_int x_int| below 2^31."""
    rng = np.random.default_rng(seed)
    bits = 16 if ea == 15 else 8
    lam = rng.uniform(0.5, 0.95, P) * np.exp(1j * rng.uniform(-np.pi, np.pi, P))
    hi = 2 ** (bits - 1) - 1
    a_re = np.clip(np.rint(lam.real * 2.0 ** ea), -hi - 1, hi).astype(np.int32)
    a_im = np.clip(np.rint(lam.imag * 2.0 ** ea), -hi - 1, hi).astype(np.int32)
    lim = (1 << 10) >> max(0, ex - eb)  # the oracle shifts Bu left by ex - eb
    bu_re = rng.integers(-lim + 1, lim, (B, L, P)).astype(np.int32)
    bu_im = rng.integers(-lim + 1, lim, (B, L, P)).astype(np.int32)
    return a_re, a_im, bu_re, bu_im, bits


def as_c64(re, im, exp):
    out = np.empty(re.shape, dtype=np.complex64)
    out.real, out.imag = np.ldexp(re.astype(F32), -exp), np.ldexp(im.astype(F32), -exp)
    return out


def oracle_scan(a_re, a_im, bu_re, bu_im, bits, ea, eb, ex, x0=None):
    from oracle import fxp_oracle as O

    xr, xi = O.scan(O.Fx(bu_re, 16, eb), O.Fx(bu_im, 16, eb), O.Fx(a_re, bits, ea), O.Fx(a_im, bits, ea), ex, ex, x0=x0)
    # the two bounds inside which the float statement and the integer one are the same function: the reference alone must
    # stay inside them, or the comparison means nothing
    amax = int(max(np.abs(a_re).max(), np.abs(a_im).max()))
    xmax = int(max(np.abs(xr).max(), np.abs(xi).max(), 0 if x0 is None else np.abs(x0[0]).max(), 0 if x0 is None else np.abs(x0[1]).max()))
    assert xmax < 2 ** 24 and amax * xmax < 2 ** 31, (amax, xmax)
    return xr, xi


@pytest.mark.parametrize("ea,eb,ex", TRIPLES)
def test_fq_scan_is_the_integer_oracle_integer_for_integer(ea, eb, ex):
    from sparsernns_amd.floatmodel import fq_scan

    B, L, P = 3, 300, 32
    a_re, a_im, bu_re, bu_im, bits = grid_problem(B, L, P, ea, eb, ex, seed=ea * 100 + eb)
    xr, xi = oracle_scan(a_re, a_im, bu_re, bu_im, bits, ea, eb, ex)
    lam, bu = as_c64(a_re, a_im, ea), as_c64(bu_re, bu_im, eb)
    xs, x_last, inside = fq_scan(lam, bu, ex, ex, domain="report")
    assert inside and xs.dtype == np.complex64 and x_last.dtype == np.complex64
    assert np.array_equal(xs.real.astype(np.float64) * 2.0 ** ex, xr) and np.array_equal(xs.imag.astype(np.float64) * 2.0 ** ex, xi)
    assert np.array_equal(x_last, xs[:, -1])
    # x0 and the carry out: two halves chained are the whole, on both sides
    cut = 130
    h1, c1 = fq_scan(lam, bu[:, :cut], ex, ex)
    h2, c2 = fq_scan(lam, bu[:, cut:], ex, ex, x0=c1)
    assert np.array_equal(np.concatenate([h1, h2], axis=1), xs) and np.array_equal(c2, x_last)
    x0 = (xr[:, cut - 1], xi[:, cut - 1])
    yr, yi = oracle_scan(a_re, a_im, bu_re[:, cut:], bu_im[:, cut:], bits, ea, eb, ex, x0=x0)
    assert np.array_equal(h2.real.astype(np.float64) * 2.0 ** ex, yr) and np.array_equal(h2.imag.astype(np.float64) * 2.0 ** ex, yi)
    # lens: a sequence stops where its length says, the rows behind are zero, the carry is the last real state
    lens = [0, 17, 999]
    xl, cl = fq_scan(lam, bu, ex, ex, lens=lens)
    assert not xl[0].any() and not cl[0].any() and np.array_equal(xl[1, :17], xs[1, :17]) and not xl[1, 17:].any()
    assert np.array_equal(cl[1], xs[1, 16]) and np.array_equal(xl[2], xs[2]) and np.array_equal(cl[2], xs[2, -1])


def test_fq_scan_reports_a_run_that_leaves_the_domain():
    from sparsernns_amd.floatmodel import fq_scan

    lam = np.array([0.5], dtype=np.complex64)
    big = np.full((1, 2, 1), 2.0 ** 15, dtype=np.complex64)
    assert fq_scan(lam, big, 8, 8, domain="report")[2] and not fq_scan(lam, big, 9, 9, domain="report")[2]
    with pytest.raises(ValueError, match="domain"):
        fq_scan(lam, big, 9, 9, domain="raise")
    tiny = np.full((1, 1, 1), 2.0 ** -140, dtype=np.complex64)  # times 2^8 still subnormal
    assert not fq_scan(lam, tiny, 8, 8, domain="report")[2]
    nan = np.array([[[1.0], [np.nan], [1.0]]], dtype=np.complex64)
    xs, last, inside = fq_scan(lam, nan, 8, 8, domain="report")
    assert inside and xs[0, 0, 0] == 1 and np.isnan(xs[0, 1:, 0].real).all() and np.isnan(last.real).all()


def floor_rule_f32(a, b, e):
    """The kernel's exact floor of a product, written out in float32: p the rounded product, r its exact residual."""
    a, b = a.astype(F32), b.astype(F32)
    p = (a * b).astype(F32)
    r = (a.astype(np.float64) * b.astype(np.float64) - p.astype(np.float64)).astype(F32)  # what fmaf(a, b, -p) returns: exact
    assert np.array_equal(r.astype(np.float64), a.astype(np.float64) * b.astype(np.float64) - p.astype(np.float64))
    s = (p * F32(2.0 ** e)).astype(F32)
    fl = np.floor(s)
    fl = np.where((fl == s) & (r < 0), fl - F32(1), fl).astype(F32)
    return (fl * F32(2.0 ** -e)).astype(F32)


def test_the_float32_exact_floor_rule_is_the_floor_of_the_exact_product():
    from sparsernns_amd.floatmodel import fq_scan

    rng = np.random.default_rng(11)
    n = 1_000_000
    for e, grid in ((14, True), (7, True), (10, False), (15, False)):
        x = (rng.integers(-2 ** 20, 2 ** 20, n) * 2.0 ** -e).astype(F32)  # states on their grid, up to 2^20 LSBs
        if grid:
            ea = 15 if e == 14 else 7
            a = (rng.integers(-2 ** ea, 2 ** ea, n) * 2.0 ** -ea).astype(F32)
        else:
            a = rng.uniform(-1, 1, n).astype(F32)
        want = np.floor(a.astype(np.float64) * x.astype(np.float64) * 2.0 ** e) * 2.0 ** -e
        assert np.array_equal(floor_rule_f32(a, x, e).astype(np.float64), want), (e, grid)
        # and it is one step of fq_scan: a real pole, a real state, no input
        m = 4096
        one, _ = fq_scan(a[:m].astype(np.complex64), np.zeros((1, 1, m), dtype=np.complex64), e, e, x0=x[:m].astype(np.complex64))
        assert np.array_equal(one[0, 0].real, floor_rule_f32(a[:m], x[:m], e)) and not one.imag.any()
    # hand-made: p * 2^e an integer with the exact product below it, above it, and equal to it
    e = 0
    a = np.array([1 + 2.0 ** -23, 1 + 2.0 ** -23, 3.0, -(1 + 2.0 ** -23)], dtype=F32)
    b = np.array([2.0 ** 23 - 1, 2.0 ** 23 + 1, 5.0, 2.0 ** 23 + 1], dtype=F32)
    exact = a.astype(np.float64) * b.astype(np.float64)
    p = (a * b).astype(F32).astype(np.float64)
    assert (p == np.floor(p)).all() and list(np.sign(exact - p)) == [-1, 1, 0, -1]
    assert np.array_equal(floor_rule_f32(a, b, e).astype(np.float64), np.floor(exact))
    assert floor_rule_f32(a[:1], b[:1], e)[0] == p[0] - 1 and floor_rule_f32(a[1:2], b[1:2], e)[0] == p[1]


@pytest.mark.parametrize("recipe", T.RECIPES)
def test_quantised_modeldict_holds_the_integer_models_weights(recipe):
    from sparsernns_amd import floatmodel as F
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = T.model(0.25, recipe)
    n = dims["n_layers"]
    before = F.pack_blob(md, n).copy()
    qmd = F.quantised_modeldict(md, qc, n)
    ex = build_regression_model(md, qc, n).export()
    deq = lambda data, exp: (data.astype(F32) / F32(2.0 ** exp)).astype(F32)

    def dense_equal(d, p, q):
        return (T.same_bits(d["kernel"], deq(p["weight"], q["weight_exp"])) and T.same_bits(d["bias"], deq(p["bias"], q["bias_exp"])))

    assert dense_equal(qmd["encoder"]["encoder"], ex["params"]["encoder"]["encoder"], ex["qconfig"]["encoder"]["encoder"])
    assert dense_equal(qmd["decoder"], ex["params"]["decoder"], ex["qconfig"]["decoder"])
    for i in range(n):
        p, q = ex["params"]["encoder"][f"layers_{i}"], ex["qconfig"]["encoder"][f"layers_{i}"]
        layer = qmd["encoder"][f"layers_{i}"]
        assert dense_equal(layer["out2"], p["out2"], q["out2"])
        lam, Bb, Cc = synth.zoh(layer["mixer"])
        for got, k in ((lam, "A"), (Bb, "B"), (Cc, "C")):
            assert got.dtype == np.complex64
            assert T.same_bits(np.ascontiguousarray(got.real), deq(p["mixer"][f"{k}_real"], q["mixer"][f"{k}_real_exp"])), (i, k)
            assert T.same_bits(np.ascontiguousarray(got.imag), deq(p["mixer"][f"{k}_imag"], q["mixer"][f"{k}_imag_exp"])), (i, k)
        assert T.same_bits(layer["mixer"]["D"], deq(p["mixer"]["D"], q["mixer"]["D_exp"]))
        assert all(T.same_bits(layer["norm"][k], md["encoder"][f"layers_{i}"]["norm"][k]) for k in layer["norm"])
    # the input is not modified, and a modeldict without the hook behaves as before, to the bit
    assert T.same_bits(F.pack_blob(md, n), before) and synth.ZOH_KEY not in md["encoder"]["layers_0"]["mixer"]
    assert not T.same_bits(F.pack_blob(qmd, n), before)
    # a subset leaves the other groups bit-identical
    sub = F.quantised_modeldict(md, qc, n, ["ssm.A", "out2"])
    for i in range(n):
        l0, l1, l2 = (m["encoder"][f"layers_{i}"] for m in (md, sub, qmd))
        z0, z1, z2 = (synth.zoh(l["mixer"]) for l in (l0, l1, l2))
        assert T.same_bits(z1[0], z2[0]) and T.same_bits(z1[1], z0[1]) and T.same_bits(z1[2], z0[2])
        assert T.same_bits(l1["mixer"]["D"], l0["mixer"]["D"]) and T.same_bits(l1["out2"]["kernel"], l2["out2"]["kernel"])
    assert T.same_bits(sub["decoder"]["kernel"], md["decoder"]["kernel"]) and T.same_bits(sub["encoder"]["encoder"]["bias"], md["encoder"]["encoder"]["bias"])
    with pytest.raises(ValueError, match="ssm.E"):
        F.quantised_modeldict(md, qc, n, ["ssm.E"])
    # accepted by float_forward and calibrate; the quantised weights move the output
    x = T.make_x(dims, (1, 9, 5), recipe)
    assert not np.array_equal(synth.float_forward(qmd, x, n), synth.float_forward(md, x, n))


def test_fq_spec_in_step_mode_and_float_forward_on_the_tiny_model():
    from sparsernns_amd import floatmodel as F

    dims = synth.tiny_dims()
    md, qc, _ = synth.make_model(dims=dims)
    n = dims["n_layers"]
    keys = F.stat_keys(n)
    assert F.FQ_STEP == 2 and F.FQ_MODES == ("floor", "nearest")
    scan, step = F.fq_spec(qc, n), F.fq_spec(qc, n, recurrence="step")
    assert np.array_equal(F.fq_spec(qc, n, recurrence="scan"), scan)
    for k, a, b in zip(keys, scan, step):
        state = k.split(".")[-1] in F.STATE_SITES
        assert (int(b["bits"]), int(b["exp"]), int(b["saturate"])) == (int(a["bits"]), int(a["exp"]), int(a["saturate"])), k
        assert int(b["mode"]) == (2 if state else 0) and int(a["mode"]) == 0, k
    one = F.fq_spec(qc, n, ["l1.x_re", "l1.x_im", "l0.y"], mode="nearest", recurrence="step")
    assert [k for k, s in zip(keys, one) if int(s["bits"])] == ["l0.y", "l1.x_re", "l1.x_im"] and F.step_layers(one, n) == [1]
    assert int(one[keys.index("l0.y")]["mode"]) == 1
    with pytest.raises(ValueError, match="recurrence"):
        F.fq_spec(qc, n, recurrence="both")
    with pytest.raises(ValueError, match="l0.x_re"):
        F.fq_spec(qc, n, ["l0.x_re"], recurrence="step")  # one state site of a layer only
    bad = step.copy()
    bad["mode"][keys.index("l0.u")] = 2
    with pytest.raises(ValueError, match="l0.u"):
        F._check_fq(bad, keys)
    bad = step.copy()
    bad["mode"][keys.index("l1.x_im")] = 0
    with pytest.raises(ValueError, match="l1.x_re"):
        F._check_fq(bad, keys)
    with pytest.raises(ValueError, match="l1.x_re"):
        synth.float_forward(md, np.zeros((1, 2, dims["d_in"]), dtype=F32), n, fq=bad)
    # the host forward in step mode: the states lie on their grid, and they are not those of scan mode
    x = synth.make_input(2, 40, dims["d_in"], seed=4)
    a_scan, a_step, st = {}, {}, {}
    y_scan = synth.float_forward(md, x, n, fq=scan, activations=a_scan)
    y_step = synth.float_forward(md, x, n, fq=step, activations=a_step, stats=st)
    assert y_step.dtype == F32 and not np.array_equal(y_step, y_scan)
    for i in range(n):
        xs = a_step["encoder"][f"layers_{i}"]["pre_C"]
        for part, key in ((xs.real, "x_re"), (xs.imag, "x_im")):
            bits, exp = F.quantiser_of(f"l{i}.{key}", qc)
            k = part.astype(np.float64) * 2.0 ** exp
            assert np.array_equal(k, np.round(k)), (i, key)
        assert st[f"l{i}.x_re"] > 0
    assert not np.array_equal(a_step["encoder"]["layers_0"]["pre_C"], a_scan["encoder"]["layers_0"]["pre_C"])
    # FloatEngine without the kernels hands the spec to the host forward
    eng = F.FloatEngine(md, n)
    assert not eng.on_device and np.array_equal(eng.forward(x, fq=step), y_step)
    # sensitivity on the host: the new rows, their order, and the plain rows unchanged
    got = F.sensitivity(md, [x], qc, n, engine=eng, recurrence="step", weights=qc)
    assert list(got) == keys + ["recurrence"] + list(F.WEIGHT_GROUPS) + ["all"]
    base = F.sensitivity(md, [x], qc, n, engine=eng)
    assert list(base) == keys + ["all"] and all(got[k] == base[k] for k in keys)
    y = synth.float_forward(md, x, n).astype(np.float64)
    rec = synth.float_forward(md, x, n, fq=F.fq_spec(qc, n, [f"l{i}.{k}" for i in range(n) for k in F.STATE_SITES], recurrence="step"))
    assert got["recurrence"] == pytest.approx(10 * math.log10((y * y).sum() / ((rec - y) ** 2).sum()), rel=1e-9)
    full = synth.float_forward(F.quantised_modeldict(md, qc, n), x, n, fq=step)
    assert got["all"] == pytest.approx(10 * math.log10((y * y).sum() / ((full - y) ** 2).sum()), rel=1e-9)
    wa = synth.float_forward(F.quantised_modeldict(md, qc, n, ["ssm.A"]), x, n)
    assert got["ssm.A"] == pytest.approx(10 * math.log10((y * y).sum() / ((wa - y) ** 2).sum()), rel=1e-9)
    with pytest.raises(ValueError, match="recurrence"):
        F.sensitivity(md, [x], qc, n, groups={"recurrence": ["l0.u"]}, engine=eng, recurrence="step")


def test_library_exports_the_step_scan_and_keeps_its_version():
    from sparsernns_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "s5fxp.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    name = "s5fxp_fq_scan_c64"
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and hasattr(_lib.lib, name) and name + "(" in hdr
    assert re.search(r"S5FXP_FQ_STEP\s*=\s*2", hdr) and _lib.lib.s5fxp_version() == 115


def test_the_step_scan_refuses_bad_arguments_before_the_device_is_touched():
    from sparsernns_amd._lib import lib

    fake = C.c_void_p(0x1000)  # never dereferenced: every call below must return before a launch
    ok = dict(lam=fake, bu=fake, xs=fake, B=1, L=1, P=32, er=8, ei=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.s5fxp_fq_scan_c64(a["lam"], a["bu"], a["xs"], None, None, None, a["B"], a["L"], a["P"], a["er"], a["ei"], None)

    for kw in (dict(lam=None), dict(bu=None), dict(xs=None), dict(B=0), dict(L=0), dict(P=0), dict(B=-3), dict(er=-25), dict(er=41),
               dict(ei=-25), dict(ei=41),
               dict(B=2 ** 31 - 1, P=2 ** 12),  # more than 2^31 - 1 workgroups
               dict(L=2 ** 21, P=128),          # row offsets past 32 bits: (64 / P + 2) * L * P * 8 bytes
               dict(L=2 ** 31 - 1, P=1)):
        assert call(**kw) == -1, kw
    null = None
    assert lib.s5fxp_float_model_forward_fq(null, fake, 1, 1, fake, None, fake, None, fake, 1 << 20, None) == -1


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the op
# ----------------------------------------------------------------------------------------------------------------------
SENTINEL = np.complex64(-7.25 + 3.5j)
OP_SHAPES = [(1, 1, 32), (3, 33, 32), (2, 70, 64), (2, 70, 96), (5, 600, 128)]  # the last: 37 prefetch blocks and 8 steps of one


def same_values(a, b):
    """Bit for bit but for the sign of a zero."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def free_problem(B, L, P, seed, exp):
    """Arbitrary float32 poles and inputs, scaled into the domain: |x| <= |Bu| / (1 - 0.97) stays below 2^24 LSBs."""
    rng = np.random.default_rng(seed)
    lam = (rng.uniform(0.3, 0.97, P) * np.exp(1j * rng.uniform(-np.pi, np.pi, P))).astype(np.complex64)
    bu = (3.0 * (rng.standard_normal((B, L, P)) + 1j * rng.standard_normal((B, L, P)))).astype(np.complex64)
    assert np.abs(bu).max() / 0.03 * 2.0 ** exp < 2.0 ** 24
    return lam, bu


def device_fq_scan(lam, bu, er, ei, x0=None, want_last=True, lens=None):
    """s5fxp_fq_scan_c64 on host arrays -> (xs, x_last or None); xs starts as SENTINEL everywhere."""
    import torch
    from sparsernns_amd._lib import check, lib

    dev = torch.device("cuda", 0)
    B, L, P = bu.shape
    t = lambda a: torch.view_as_real(torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex64))).to(dev).contiguous()
    lam_d, bu_d = t(lam), t(bu)
    xs_d = t(np.full(bu.shape, SENTINEL))
    x0_d = None if x0 is None else t(x0)
    last_d = t(np.full((B, P), SENTINEL)) if want_last else None
    lens_d = None if lens is None else torch.tensor(list(lens), dtype=torch.int32, device=dev)
    ptr = lambda v: None if v is None else v.data_ptr()
    check(lib.s5fxp_fq_scan_c64(ptr(lam_d), ptr(bu_d), ptr(xs_d), ptr(x0_d), ptr(last_d), ptr(lens_d), B, L, P, er, ei,
                                torch.cuda.current_stream().cuda_stream), "s5fxp_fq_scan_c64")
    torch.cuda.synchronize()
    c = lambda v: None if v is None else np.ascontiguousarray(v.cpu().numpy()).view(np.complex64)[..., 0]
    return c(xs_d), c(last_d)


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,P", OP_SHAPES, ids=[f"{b}-{l}-{p}" for b, l, p in OP_SHAPES])
def test_the_op_is_fq_scan_bit_for_bit(B, L, P):
    from sparsernns_amd.floatmodel import fq_scan

    for ea, eb, ex in TRIPLES[:1] + TRIPLES[3:]:  # inputs on their grids: also the integer oracle itself
        a_re, a_im, bu_re, bu_im, bits = grid_problem(B, L, P, ea, eb, ex, seed=B + L + P)
        lam, bu = as_c64(a_re, a_im, ea), as_c64(bu_re, bu_im, eb)
        ref, ref_last = fq_scan(lam, bu, ex, ex, domain="raise")
        xs, last = device_fq_scan(lam, bu, ex, ex)
        assert same_values(xs, ref) and same_values(last, ref_last)
        xr, xi = oracle_scan(a_re, a_im, bu_re, bu_im, bits, ea, eb, ex)
        assert np.array_equal(xs.real.astype(np.float64) * 2.0 ** ex, xr) and np.array_equal(xs.imag.astype(np.float64) * 2.0 ** ex, xi)
    er, ei = 10, 12  # arbitrary float32 lambda and Bu, different exponents for the two components
    lam, bu = free_problem(B, L, P, seed=7 * B + L + P, exp=max(er, ei))
    ref, ref_last = fq_scan(lam, bu, er, ei, domain="raise")
    xs, last = device_fq_scan(lam, bu, er, ei, want_last=False)
    assert same_values(xs, ref) and last is None
    x0 = ref_last * np.complex64(0.5)  # not zero, and not on the grids: a state enters a step through floored products only
    ref0, ref0_last = fq_scan(lam, bu, er, ei, x0=x0, domain="raise")
    xs, last = device_fq_scan(lam, bu, er, ei, x0=x0)
    assert same_values(xs, ref0) and same_values(last, ref0_last) and (L == 1 or not same_values(ref0, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("P", [32, 96])  # a wave holds lanes of two sequences of different lengths
def test_the_op_with_lens_touches_nothing_past_a_length(P):
    from sparsernns_amd.floatmodel import fq_scan

    lens, L = (0, 1, 15, 16, 17, 600, 70), 600
    er = ei = 11
    lam, bu = free_problem(len(lens), L, P, seed=P, exp=er)
    x0 = fq_scan(lam, bu[:, :5], er, ei)[1]
    ref, ref_last = fq_scan(lam, bu, er, ei, x0=x0, lens=lens, domain="raise")
    xs, last = device_fq_scan(lam, bu, er, ei, x0=x0, lens=lens)
    for e, n in enumerate(lens):
        assert same_values(xs[e, :n], ref[e, :n]), e
        assert (xs[e, n:] == SENTINEL).all(), e  # rows from the length on keep the sentinel
    assert same_values(last, ref_last) and same_values(last[0], x0[0])
    # lengths outside 0 .. L are clamped
    xs2, _ = device_fq_scan(lam, bu[:2], er, ei, lens=(-4, 10 ** 6))
    assert (xs2[0] == SENTINEL).all() and same_values(xs2[1], fq_scan(lam, bu[1:2], er, ei)[0][0])


@pytest.mark.gpu
def test_a_nan_in_bu_stays_in_its_state():
    from sparsernns_amd.floatmodel import fq_scan

    lam, bu = free_problem(1, 40, 32, seed=3, exp=9)
    bu[0, 20, 5] = np.nan
    ref, _ = fq_scan(lam, bu, 9, 9)
    xs, _ = device_fq_scan(lam, bu, 9, 9)
    nan = np.isnan(xs.real) | np.isnan(xs.imag)
    assert np.array_equal(nan, np.isnan(ref.real) | np.isnan(ref.imag)) and nan[0, 20:, 5].all() and nan.sum() == 20
    assert np.array_equal(xs[~nan], ref[~nan])


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the model
# ----------------------------------------------------------------------------------------------------------------------
MODEL_CASES = [(2, 70, 12), (1, 1, 13)]
MODEL_GRID = [(d, c, r) for r in T.RECIPES for d in (0.25, 1.0) for c in MODEL_CASES]
MODEL_IDS = [f"{r}-dim{d}-B{c[0]}L{c[1]}" for d, c, r in MODEL_GRID]


def state_exps(qc, i):
    from sparsernns_amd import floatmodel as F

    return F.quantiser_of(f"l{i}.x_re", qc)[1], F.quantiser_of(f"l{i}.x_im", qc)[1]


def check_xs_is_fq_scan(t, md, qc, i):
    """Layer i's xs plane is fq_scan of the device's own Bu plane and the packed lambda, inside the domain."""
    from sparsernns_amd.floatmodel import fq_scan

    lam = synth.zoh(md["encoder"][f"layers_{i}"]["mixer"])[0]
    ref, _ = fq_scan(lam, t[f"l{i}.Bu"], *state_exps(qc, i), domain="raise")
    assert same_values(t[f"l{i}.xs"], ref), (i, int(np.count_nonzero(t[f"l{i}.xs"] != ref)))


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case,recipe", MODEL_GRID, ids=MODEL_IDS)
def test_one_layer_in_step_mode(dim, case, recipe):
    from sparsernns_amd import floatmodel as F

    md, qc, dims = T.model(dim, recipe)
    n = dims["n_layers"]
    t0 = T.plain(dim, case, recipe)
    order, keys = T.plane_order(n), F.stat_keys(n)
    i = 1
    spec = F.fq_spec(qc, n, [f"l{i}.x_re", f"l{i}.x_im"], recurrence="step")
    t = T.host_planes(T.engine(dim, recipe).forward_traced(t0["x"], fq=spec))
    upstream = order.index(f"l{i}.xs")
    for k in order[:upstream]:  # every plane upstream is the plain forward's
        assert T.same_bits(t[k], t0[k]), k
    j = keys.index(f"l{i}.x_re")
    assert T.same_bits(t["stats"][:j], t0["stats"][:j])
    check_xs_is_fq_scan(t, md, qc, i)
    assert not np.array_equal(t[f"l{i}.xs"], t0[f"l{i}.xs"])
    # the observers keep their place and meaning: the absmax of the stepped states
    assert t["stats"][j] == np.abs(t[f"l{i}.xs"].real).max() and t["stats"][j + 1] == np.abs(t[f"l{i}.xs"].imag).max()
    # the gate kernel got the two sites as off: y is the plain stage on these states
    layer = md["encoder"][f"layers_{i}"]
    v, S = R.stage_y(t[f"l{i}.xs"], t[f"l{i}.u"], synth.zoh(layer["mixer"])[2], layer["mixer"]["D"])
    R.within(t[f"l{i}.y"], v, dims["P"], S, f"l{i}.y")


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case,recipe", MODEL_GRID, ids=MODEL_IDS)
def test_all_sites_on_in_step_mode(dim, case, recipe):
    check_all_sites_on_in_step_mode(dim, case, recipe)


def check_all_sites_on_in_step_mode(dim, case, recipe, t=None):
    """``t``: host copies of the planes of a traced forward of ``T.make_x(dims, case, recipe)`` under the all-sites step spec that
    the caller ran on buffers of its own (tests/test_caller_memory.py); None: ``forward_traced`` runs it here."""
    from sparsernns_amd import floatmodel as F

    md, qc, dims = T.model(dim, recipe)
    n, H, P = dims["n_layers"], dims["H"], dims["P"]
    x = T.make_x(dims, case, recipe)
    spec = F.fq_spec(qc, n, recurrence="step")
    if t is None:
        t = T.host_planes(T.engine(dim, recipe).forward_traced(x, fq=spec))
    Q = lambda key: T.fq_of(key, spec, n)
    shares = {}
    relu = lambda v: np.maximum(v, 0)
    enc = md["encoder"]
    v, S = R.stage_dense(Q("encoder.inp")(x), enc["encoder"]["kernel"], enc["encoder"]["bias"])
    T.sandwich(t["h_enc"], v, R.bound(257, S), Q("encoder.out"), "encoder.out", shares, post=relu)
    h = t["h_enc"]
    for i in range(n):
        layer = enc[f"layers_{i}"]
        lam_bar, B_bar, Cc = synth.zoh(layer["mixer"])
        u, y, g_in, g, h_out = (t[f"l{i}.{k}"] for k in ("u", "y", "g_in", "g", "h_out"))
        Bu, xs = t[f"l{i}.Bu"], t[f"l{i}.xs"]
        v, S = R.stage_u(h, layer["norm"])
        T.sandwich(u, v, R.bound(0, S), Q(f"l{i}.u"), "u", shares)
        (vr, Sr), (vi, Si) = R.stage_bu(u, B_bar)
        T.sandwich(Bu.real, vr, R.bound(H, Sr), Q(f"l{i}.Bu_re"), "Bu_re", shares)
        T.sandwich(Bu.imag, vi, R.bound(H, Si), Q(f"l{i}.Bu_im"), "Bu_im", shares)
        check_xs_is_fq_scan(t, md, qc, i)  # the recurrence rounds; the state sites do nothing more
        for part, key in ((xs.real, "x_re"), (xs.imag, "x_im")):
            T.on_grid(part, *F.quantiser_of(f"l{i}.{key}", qc), False, f"l{i}.{key}")
        v, S = R.stage_y(xs, u, Cc, layer["mixer"]["D"])
        T.sandwich(y, v, R.bound(P, S), Q(f"l{i}.y"), "y", shares)
        x1 = relu(y)
        v, S = R.stage_dense(Q(f"l{i}.out2.inp")(x1), layer["out2"]["kernel"], layer["out2"]["bias"])
        T.sandwich(g_in, v, R.bound(H, S), Q(f"l{i}.out2.out"), "out2.out", shares)
        T.sandwich(g, R.sigmoid64(g_in), T.sigmoid_bound(g_in), Q(f"l{i}.gate.r"), "gate.r", shares)
        v, S = R.stage_hout(Q(f"l{i}.gate.l")(x1), g, h)
        assert (np.abs(h_out.astype(np.float64) - v) <= R.bound(0, S)).all(), f"l{i}.h_out"
        h = h_out
    v, S = R.stage_dense(Q("decoder.inp")(h), md["decoder"]["kernel"], md["decoder"]["bias"])
    T.sandwich(t["out"], v, R.bound(H, S), Q("decoder.out"), "decoder.out", shares)
    if recipe != "w8a16":
        assert all(s <= 1.0 - T.PINNED_SHARE for s in shares.values()), shares
    st = dict(zip(F.stat_keys(n), t["stats"]))
    for i in range(n):
        assert st[f"l{i}.x_re"] == np.abs(t[f"l{i}.xs"].real).max() and st[f"l{i}.x_im"] == np.abs(t[f"l{i}.xs"].imag).max()
    # the hot forward is the traced one
    import torch
    eng = T.engine(dim, recipe)
    s2 = eng.new_stats()
    y2 = eng.forward_device(torch.from_numpy(x).to(eng.device), s2, fq=spec)
    assert T.same_bits(y2.cpu().numpy(), t["out"]) and T.same_bits(s2.cpu().numpy(), t["stats"])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [0.25, 1.0])
def test_clips_in_step_mode_get_what_their_own_forward_gets(dim):
    import torch
    from sparsernns_amd import floatmodel as F

    recipe = "w8a8"
    eng = T.engine(dim, recipe)
    _, qc, dims = T.model(dim, recipe)
    spec = F.fq_spec(qc, dims["n_layers"], recurrence="step")
    lens = [0, 1, 31, 32, 33, 70]
    x = torch.from_numpy(T.make_x(dims, (len(lens), 70, 21), recipe)).to(eng.device)
    ld = torch.tensor(lens, dtype=torch.int32, device=eng.device)
    y = torch.full_like(x, -7.25)
    st = eng.new_stats()
    assert eng.forward_clips_device(x, ld, st, out=y, fq=spec) is y
    want = eng.new_stats()
    for e, m in enumerate(lens):
        assert bool((y[e, m:] == -7.25).all()), e
        if m:
            ye = eng.forward_device(x[e:e + 1, :m], want, fq=spec)
            assert T.same_bits(y[e, :m].cpu().numpy(), ye[0].cpu().numpy()), e
    assert T.same_bits(st.cpu().numpy(), want.cpu().numpy())
    assert not torch.equal(eng.forward_clips_device(x, ld, fq=T.full_spec(dim, recipe))[5], y[5])  # not the scan-mode clips


@pytest.mark.gpu
def test_entries_refuse_misplaced_step_sites_before_anything_is_launched():
    import torch
    from sparsernns_amd import floatmodel as F
    from sparsernns_amd._lib import lib

    dim, recipe = 0.25, "w8a8"
    eng = T.engine(dim, recipe)
    _, qc, dims = T.model(dim, recipe)
    keys = eng.keys
    x = torch.from_numpy(T.plain(dim, T.CASES[0], recipe)["x"]).to(eng.device)
    B, L = x.shape[:2]
    need = lib.s5fxp_float_workspace_bytes(eng._h, B, L, 0)
    ws, y = torch.empty(need // 4, device=eng.device), torch.full_like(x, 7.0)
    lens = torch.full((B,), L, dtype=torch.int32, device=eng.device)
    st = eng.new_stats()

    def both(spec, nbytes=need):
        a = lib.s5fxp_float_model_forward_fq(eng._h, x.data_ptr(), B, L, y.data_ptr(), st.data_ptr(), spec.ctypes.data, None,
                                             ws.data_ptr(), nbytes, None)
        b = lib.s5fxp_float_model_clips_fq(eng._h, x.data_ptr(), B, L, lens.data_ptr(), y.data_ptr(), st.data_ptr(),
                                           spec.ctypes.data, ws.data_ptr(), nbytes, None)
        assert a == b
        return a

    good = F.fq_spec(qc, dims["n_layers"], recurrence="step")
    for key, field, value in (("l0.u", "mode", 2), ("encoder.inp", "mode", 2), ("l2.gate.r", "mode", 2), ("decoder.out", "mode", 2),
                              ("l1.x_re", "mode", 0), ("l1.x_im", "mode", 1), ("l0.x_im", "bits", 0), ("l2.x_re", "saturate", 1),
                              ("l2.x_im", "bits", 25), ("l0.x_re", "exp", 41), ("l0.x_re", "mode", 3)):
        bad = good.copy()
        bad[field][keys.index(key)] = value
        assert both(bad) == -1, (key, field, value)
        with pytest.raises(ValueError):
            eng.forward_device(x, fq=bad)
    assert both(good, need - 1) == -5  # the step sites pass, the workspace does not
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and not bool(st.any())


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [0.25, 1.0])
def test_a_spec_without_step_sites_is_scan_mode_to_the_bit(dim):
    from sparsernns_amd import floatmodel as F

    recipe, case = "w8a8", T.CASES[0]
    _, qc, dims = T.model(dim, recipe)
    n = dims["n_layers"]
    keys = F.stat_keys(n)
    eng = T.engine(dim, recipe)
    x = T.plain(dim, case, recipe)["x"]
    others = [k for k in keys if k.split(".")[-1] not in F.STATE_SITES]
    a = F.fq_spec(qc, n, others, recurrence="step")  # no state site on: nothing to step
    assert np.array_equal(a, F.fq_spec(qc, n, others)) and not F.step_layers(a, n)
    scan = T.host_planes(eng.forward_traced(x, fq=F.fq_spec(qc, n, recurrence="scan")))
    same = T.host_planes(eng.forward_traced(x, fq=T.full_spec(dim, recipe)))
    assert all(T.same_bits(scan[k], same[k]) for k in scan)
    step = T.host_planes(eng.forward_traced(x, fq=F.fq_spec(qc, n, recurrence="step")))
    assert T.same_bits(step["l0.Bu"], scan["l0.Bu"]) and not np.array_equal(step["l0.xs"], scan["l0.xs"])
    assert not np.array_equal(step["out"], scan["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", ["w8a8", "w4a8"])
def test_quantised_weights_on_the_device_are_the_host_forward_on_that_modeldict(recipe):
    from sparsernns_amd import floatmodel as F

    dim, case = 0.25, T.CASES[0]
    md, qc, dims = T.model(dim, recipe)
    n = dims["n_layers"]
    qmd = F.quantised_modeldict(md, qc, n)
    eng = F.FloatEngine(qmd, n)
    assert eng.on_device
    x = T.make_x(dims, case, recipe)
    t = T.host_planes(eng.forward_traced(x))
    R.check_stages(qmd, n, x, t)  # the plain model's bounds, stage by stage, on the quantised parameters
    R.check_observers(qmd, n, x, t)
    assert not np.array_equal(t["out"], T.plain(dim, case, recipe)["out"])
    # and together with the stepping recurrence: the packed quantised poles drive fq_scan
    ts = T.host_planes(eng.forward_traced(x, fq=F.fq_spec(qc, n, recurrence="step")))
    for i in range(n):
        check_xs_is_fq_scan(ts, qmd, qc, i)


@pytest.mark.gpu
def test_sensitivity_with_the_recurrence_and_the_weights_is_the_hand_written_loop():
    import torch
    from sparsernns_amd import floatmodel as F

    dim, recipe = 0.25, "w8a8"
    md, qc, dims = T.model(dim, recipe)
    n = dims["n_layers"]
    eng = T.engine(dim, recipe)
    xa = T.make_x(dims, (2, 70, 31), recipe)
    xb = torch.from_numpy(T.make_x(dims, (3, 40, 32), recipe)).to(eng.device)
    lens = [40, 0, 17]
    got = F.sensitivity(md, [xa, (xb, lens)], qc, n, engine=eng, recurrence="step", weights=qc)
    assert list(got) == F.stat_keys(n) + ["recurrence"] + list(F.WEIGHT_GROUPS) + ["all"]  # nothing left the domain

    def frames(e, fq):
        ya = e.forward_device(torch.from_numpy(xa).to(e.device), fq=fq).double().flatten()
        yb = [e.forward_device(xb[k:k + 1, :m], fq=fq).double().flatten() for k, m in enumerate(lens) if m]
        return ya, torch.cat(yb)

    pa, pb = frames(eng, None)
    num = float((pa * pa).sum() + (pb * pb).sum())
    states = [f"l{i}.{k}" for i in range(n) for k in F.STATE_SITES]
    rows = {"l0.x_re": (eng, F.fq_spec(qc, n, ["l0.x_re"])),
            "recurrence": (eng, F.fq_spec(qc, n, states, recurrence="step")),
            "ssm.A": (F.FloatEngine(F.quantised_modeldict(md, qc, n, ["ssm.A"]), n), None),
            "out2": (F.FloatEngine(F.quantised_modeldict(md, qc, n, ["out2"]), n), None),
            "all": (F.FloatEngine(F.quantised_modeldict(md, qc, n), n), F.fq_spec(qc, n, recurrence="step"))}
    for g, (e, fq) in rows.items():
        qa, qb = frames(e, fq)
        den = float(((qa - pa) ** 2).sum() + ((qb - pb) ** 2).sum())
        print(f"{g}: {got[g]:.2f} dB")
        assert got[g] == pytest.approx(10 * math.log10(num / den), rel=1e-9), g
    assert all(math.isfinite(v) for v in got.values())
    base = F.sensitivity(md, [xa], qc, n, groups={"l1": [f"l1.{k}" for k in T.LAYER_KEYS]}, engine=eng, recurrence="step")
    assert list(base) == ["l1", "recurrence", "all"]


@pytest.mark.gpu
def test_audio_wrappers_pass_a_step_spec_and_a_quantised_engine_on():
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd import floatmodel as F

    dim, recipe = 0.25, "w8a8"
    md, qc, dims = T.model(dim, recipe)
    n = dims["n_layers"]
    eng = F.FloatEngine(F.quantised_modeldict(md, qc, n), n)
    spec = F.fq_spec(qc, n, recurrence="step")
    rng = np.random.default_rng(4)
    Ts = [512 + 128 * 9, 512 + 128 * 3]
    noisy = [torch.from_numpy((0.05 * rng.standard_normal(v)).astype(F32)).to(eng.device) for v in Ts]
    clean = [torch.from_numpy((0.05 * rng.standard_normal(v)).astype(F32)).to(eng.device) for v in Ts]
    x = audio.stft_mag(noisy[0][None])
    mask = eng.forward(x, fq=spec)
    assert not torch.equal(mask, eng.forward(x, fq=T.full_spec(dim, recipe)))
    cleaned, cm = audio.mask_istft(noisy[0][None], mask, cleaned_mag=True)
    for a, b in zip(audio.denoise_float(eng, noisy[0][None], fq=spec), (cleaned, cm, x, mask)):
        assert torch.equal(a, b)
    loss, snr = audio.validate_float(eng, noisy[0][None], clean[0][None], lam=0.001, fq=spec)
    wl, ws, _ = audio.score_fused(noisy[0][None], clean[0][None], mask, 0.001)
    assert torch.equal(loss, wl) and torch.equal(snr, ws)
    outs = audio.denoise_float_clips(eng, noisy, fq=spec)
    cl, cs = audio.validate_float_clips(eng, noisy, clean, lam=0.001, fq=spec)
    for e in range(len(noisy)):
        for a, b in zip(outs[e], audio.denoise_float(eng, noisy[e][None], fq=spec)):
            assert torch.equal(a, b[0]), e
        l1, s1 = audio.validate_float(eng, noisy[e][None], clean[e][None], lam=0.001, fq=spec)
        assert torch.equal(cl[e:e + 1], l1) and torch.equal(cs[e:e + 1], s1), e
