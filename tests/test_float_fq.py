"""The fake-quantised float forward and the per-tensor sensitivity built on it.

The reference of every test is ``floatmodel.fake_quant``, the NumPy statement of the quantiser
q(v) = clamp(R(v 2^exp), -2^(bits-1), 2^(bits-1) - 1) 2^-exp.  On the device a site that is switched on alone must leave
everything upstream bit-identical and turn its own stored plane into ``fake_quant`` of the plain forward's plane, value for
value; with all sites on every stage is rebuilt in float64 from the device's own (quantised) input planes and the device value
must lie between q(ref - bound) and q(ref + bound), bound = the float32 chain bound of tests/float_model_ref.py -- q is
monotone, so that is exactly what the chain bound permits.  At the 8-bit recipes the two ends coincide for at least 98 % of
the elements of every site, so there the device value is pinned exactly.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import float_model_ref as R
from sparsernns_amd import synth

RECIPES = ("w8a8", "w4a8", "w8a16")
CASES = [(2, 70, 12), (1, 1, 13), (3, 33, 12)]
DIMS_FOR = {(2, 70, 12): (0.25, 0.5, 0.75, 1.0), (1, 1, 13): (0.25,), (3, 33, 12): (0.25,)}
STRIDE = (0.25, (5, 3300, 14))  # 516 tiles of 32 frames on a launch of at most 512 workgroups: a workgroup walks two tiles
GRID = [(d, c) for c in CASES for d in DIMS_FOR[c]] + [STRIDE]
IDS = [f"dim{d}-B{c[0]}L{c[1]}" for d, c in GRID]
STRIDES_UP = [(d, STRIDE[1]) for d in (0.5, 0.75, 1.0)]  # the same walk in the other three instantiations of every kernel
STRIDE_UP_IDS = [f"dim{d}-B{c[0]}L{c[1]}" for d, c in STRIDES_UP]
LAYER_KEYS = ("u", "Bu_re", "Bu_im", "x_re", "x_im", "y", "out2.inp", "out2.out", "gate.l", "gate.r")
PINNED_SHARE = 0.98  # of every site's elements, at the 8-bit recipes


@functools.lru_cache(maxsize=None)
def model(dim, recipe):
    if recipe == "w8a16":
        return synth.make_model(dim)
    return synth.make_model(dim, quantization=recipe, bn_stats="random", input_scale=300.0)  # test_gpu_parity.py's 8-bit recipes


def make_x(dims, case, recipe):
    return synth.make_input(case[0], case[1], dims["d_in"], seed=case[2], scale=1.0 if recipe == "w8a16" else 300.0)


def fq_of(key, spec, n_layers):
    """fake_quant with the fields of ``key``'s entry of ``spec``."""
    from sparsernns_amd import floatmodel as F

    s = spec[F.stat_keys(n_layers).index(key)]
    assert int(s["bits"]), key
    return lambda v: F.fake_quant(v, int(s["bits"]), int(s["exp"]), F.FQ_MODES[int(s["mode"])], bool(s["saturate"]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_fq_entries_and_keeps_its_version():
    from sparsernns_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.LIB_PATH))), "include", "s5fxp.h")).read()
    for name in ("s5fxp_float_model_forward_fq", "s5fxp_float_model_clips_fq"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and hasattr(_lib.lib, name) and name + "(" in hdr, name
    assert _lib.lib.s5fxp_version() == 115
    assert C.sizeof(_lib.FloatFqSite) == 4


def test_c_entries_refuse_null_arguments_before_the_device_is_touched():
    from sparsernns_amd._lib import lib

    fake = 0x1000  # never dereferenced: the argument checks fail first
    spec = np.zeros(34, dtype=np.int32).ctypes.data
    for fq in (None, spec):
        assert lib.s5fxp_float_model_forward_fq(None, fake, 1, 1, fake, None, fq, None, fake, 1 << 20, None) == -1
        assert lib.s5fxp_float_model_clips_fq(None, fake, 1, 1, fake, fake, None, fq, fake, 1 << 20, None) == -1


def test_fake_quant_known_answers():
    from sparsernns_amd.floatmodel import fake_quant

    f = np.float32
    q = fake_quant(f(-0.3), 8, 2)
    assert q.dtype == np.float32 and q == f(-0.5)  # floor, not truncation
    assert fake_quant(f(0.3), 8, 2) == f(0.25)
    # both saturation ends at 8 bits, exp 7
    assert np.array_equal(fake_quant(np.array([3.0, 1.0, 127 / 128, -1.0, -1.01, -3.0], dtype=f), 8, 7),
                          np.array([127 / 128, 127 / 128, 127 / 128, -1.0, -1.0, -1.0], dtype=f))
    assert fake_quant(f(3.0), 8, 7, saturate=False) == f(3.0) and fake_quant(f(-3.004), 8, 7, saturate=False) == f(-385 / 128)
    # ties of NEAREST go to even: 0.5 LSB -> 0, 1.5 LSB -> 2 LSB, 2.5 LSB -> 2 LSB, and the same below zero
    lsb = 2.0 ** -7
    ties = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.75], dtype=f) * f(lsb)
    assert np.array_equal(fake_quant(ties, 8, 7, mode="nearest"), np.array([0, 2, 2, 0, -2, -2, 1], dtype=f) * f(lsb))
    assert np.array_equal(fake_quant(ties, 8, 7), np.array([0, 1, 2, -1, -2, -3, 0], dtype=f) * f(lsb))
    # NaN stays NaN, with and without the clamp, in both modes
    for mode in ("floor", "nearest"):
        for sat in (True, False):
            out = fake_quant(np.array([np.nan, 0.25], dtype=f), 8, 7, mode=mode, saturate=sat)
            assert np.isnan(out[0]) and out[1] == f(0.25)
    # the two zeros count as equal
    assert fake_quant(f(-0.0), 8, 7) == 0 and fake_quant(f(-1e-9), 8, 7, mode="nearest") == 0
    # negative exponents and the widest fields
    assert fake_quant(f(1000.0), 8, -3) == f(1000.0) and fake_quant(f(1001.0), 8, -3) == f(1000.0) and fake_quant(f(5000.0), 8, -3) == f(1016.0)
    assert fake_quant(f(0.7), 24, 23) == f(math.floor(0.7 * 2 ** 23) / 2 ** 23)
    with pytest.raises(ValueError):
        fake_quant(f(1.0), 8, 7, mode="trunc")
    # idempotence, and q(v) 2^exp is an integer inside the bounds
    rng = np.random.default_rng(3)
    v = (rng.standard_normal(4096) * 2.0).astype(f)
    for bits, exp, mode, sat in ((8, 7, "floor", True), (8, 5, "nearest", True), (16, 12, "floor", False), (4, 1, "nearest", True),
                                 (2, 0, "floor", True), (24, 20, "floor", True), (8, -2, "nearest", True)):
        q = fake_quant(v, bits, exp, mode, sat)
        assert np.array_equal(fake_quant(q, bits, exp, mode, sat), q)
        n = q.astype(np.float64) * 2.0 ** exp
        assert np.array_equal(n, np.round(n))
        if sat:
            assert n.min() >= -2 ** (bits - 1) and n.max() <= 2 ** (bits - 1) - 1
        assert (np.diff(fake_quant(np.sort(v), bits, exp, mode, sat)) >= 0).all()  # monotone


def test_fq_spec_follows_quantiser_of():
    from sparsernns_amd import floatmodel as F

    for recipe in RECIPES:
        _, qc, dims = model(0.25, recipe)
        keys = F.stat_keys(dims["n_layers"])
        spec = F.fq_spec(qc, dims["n_layers"])
        assert spec.dtype == F.FQ_SITE and spec.dtype.itemsize == 4 and spec.shape == (34,) and spec.flags["C_CONTIGUOUS"]
        for k, s in zip(keys, spec):
            assert (int(s["bits"]), int(s["exp"])) == F.quantiser_of(k, qc), k
            assert int(s["mode"]) == 0 and int(s["saturate"]) == (0 if k.split(".")[-1] in ("x_re", "x_im") else 1), k
        near = F.fq_spec(qc, dims["n_layers"], mode="nearest")
        assert (near["mode"] == 1).all() and np.array_equal(near["bits"], spec["bits"]) and np.array_equal(near["exp"], spec["exp"])
        some = F.fq_spec(qc, dims["n_layers"], ["l1.y", "decoder.out"])
        on = [keys.index("l1.y"), keys.index("decoder.out")]
        assert np.array_equal(some[on], spec[on])
        off = np.delete(some, on)
        assert not off.view(np.uint8).any()  # off sites are all zero
        assert not F.fq_spec(qc, dims["n_layers"], []).view(np.uint8).any()
    _, qc, dims = model(0.25, "w8a8")
    with pytest.raises(ValueError, match="l3.y"):
        F.fq_spec(qc, dims["n_layers"], ["l3.y"])
    with pytest.raises(ValueError):
        F.fq_spec(qc, dims["n_layers"], mode="trunc")
    import copy
    bad = copy.deepcopy(qc)
    bad["decoder"]["out_bits"] = 32  # the entry takes 2..24 bits
    with pytest.raises(ValueError, match="decoder.out"):
        F.fq_spec(bad, dims["n_layers"])
    assert F.fq_spec(bad, dims["n_layers"], ["l0.u"])["bits"].sum() == 8  # a refused quantiser only matters where it is on
    bad = copy.deepcopy(qc)
    bad["blocks"]["out2"]["inp_exp"] = 41
    with pytest.raises(ValueError, match="out2.inp"):
        F.fq_spec(bad, dims["n_layers"])


def test_float_forward_with_a_spec():
    from sparsernns_amd import floatmodel as F

    md, qc, dims = model(0.25, "w8a8")
    n = dims["n_layers"]
    x = make_x(dims, (2, 20, 12), "w8a8")
    st0, st1, act0, act1 = {}, {}, {}, {}
    y0 = synth.float_forward(md, x, n, stats=st0, activations=act0)
    y1 = synth.float_forward(md, x, n, stats=st1, activations=act1, fq=F.fq_spec(qc, n, []))
    assert same_bits(y0, y1) and st0 == st1  # an all-off spec is no spec, to the bit
    assert all(same_bits(act0["encoder"][f"layers_{i}"][k], act1["encoder"][f"layers_{i}"][k])
               for i in range(n) for k in ("input", "pre_s5", "pre_C", "pre_GLU", "post_GLU", "__call__"))
    # only encoder.inp on: the model of the quantised input, and the observer still sees the raw one
    spec = F.fq_spec(qc, n, ["encoder.inp"])
    st = {}
    y = synth.float_forward(md, x, n, stats=st, fq=spec)
    st_q = {}
    assert same_bits(y, synth.float_forward(md, fq_of("encoder.inp", spec, n)(x), n, stats=st_q)) and not same_bits(y, y0)
    assert st["encoder.inp"] == st0["encoder.inp"] and all(st[k] == st_q[k] for k in st if k != "encoder.inp")
    # all sites on: every output value lies on the decoder's grid, inside its bounds
    full = F.fq_spec(qc, n)
    yq = synth.float_forward(md, x, n, fq=full)
    bits, exp = F.quantiser_of("decoder.out", qc)
    k = yq.astype(np.float64) * 2.0 ** exp
    assert yq.dtype == np.float32 and np.array_equal(k, np.round(k)) and k.min() >= -2 ** (bits - 1) and k.max() <= 2 ** (bits - 1) - 1
    with pytest.raises(ValueError):
        synth.float_forward(md, x, n, fq=full[:-1])


def test_float_engine_without_the_kernels_is_float_forward_with_the_spec(monkeypatch):
    import torch
    from sparsernns_amd import floatmodel as F

    md, qc, dims = model(0.25, "w8a8")
    n = dims["n_layers"]
    x = make_x(dims, (2, 9, 5), "w8a8")
    spec = F.fq_spec(qc, n)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    eng = F.FloatEngine(md, n)
    assert eng.on_device is False
    st, st_ref = {}, {}
    y = eng.forward(x, stats=st, fq=spec)
    ref = synth.float_forward(md, x, n, stats=st_ref, fq=spec)
    assert same_bits(y, ref) and st == st_ref and not same_bits(y, eng.forward(x))
    assert torch.equal(eng.forward(torch.from_numpy(x), fq=spec), torch.from_numpy(ref))
    clips = eng.forward_clips([x[0, :4], x[1]], fq=spec)
    assert same_bits(clips[0], synth.float_forward(md, x[:1, :4], n, fq=spec)[0]) and same_bits(clips[1], ref[1])
    # fake quantisation and the histogram are not offered together; a malformed spec is named
    for call in (lambda: eng.forward(x, hist={}, fq=spec), lambda: eng.forward_clips([x[0]], hist={}, fq=spec),
                 lambda: eng.forward(x, fq=spec[:-1]), lambda: eng.forward(x, fq=np.zeros(34, dtype=np.int32))):
        with pytest.raises(ValueError):
            call()
    bad = spec.copy()
    bad["saturate"][F.stat_keys(n).index("l1.x_im")] = 1
    with pytest.raises(ValueError, match="l1.x_im"):
        eng.forward(x, fq=bad)
    bad = spec.copy()
    bad["bits"][0] = 1
    with pytest.raises(ValueError, match="encoder.inp"):
        eng.forward(x, fq=bad)


def test_sensitivity_on_the_tiny_model(monkeypatch):
    import torch
    from sparsernns_amd import floatmodel as F

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dims = synth.tiny_dims()
    md, qc, _ = synth.make_model(dims=dims)
    n = dims["n_layers"]
    xa, xb = synth.make_input(2, 12, dims["d_in"], seed=3), synth.make_input(3, 7, dims["d_in"], seed=4)
    keys = F.stat_keys(n)
    s = F.sensitivity(md, [xa, (xb, [7, 0, 3])], qc, n)
    assert list(s) == keys + ["all"] and all(math.isfinite(v) for v in s.values())
    assert s["all"] <= max(s.values())
    # the definition, by hand, on the real frames only
    ys = lambda fq: np.concatenate([synth.float_forward(md, v, n, fq=fq).astype(np.float64).ravel()
                                    for v in (xa, xb[:1], xb[2:, :3])])
    y = ys(None)
    for g in ("l0.y", "all"):
        d = ys(F.fq_spec(qc, n, None if g == "all" else [g])) - y
        assert s[g] == pytest.approx(10 * math.log10((y * y).sum() / (d * d).sum()), rel=1e-10)
    # groups of several keys; a group that changes nothing gives inf
    g2 = F.sensitivity(md, [xa], qc, n, groups={"states": [k for k in keys if k.endswith(("x_re", "x_im"))], "io": ["encoder.inp", "decoder.out"]},
                       mode="nearest")
    assert list(g2) == ["states", "io", "all"] and all(math.isfinite(v) for v in g2.values())
    exact = F.sensitivity(md, [np.zeros((1, 3, dims["d_in"]), dtype=np.float32)], qc, n, groups={"inp": ["encoder.inp"]})
    assert exact["inp"] == math.inf and exact["all"] == math.inf  # q(0) = 0: no difference at all
    with pytest.raises(ValueError):
        F.sensitivity(md, [], qc, n)
    with pytest.raises(ValueError):
        F.sensitivity(md, [xa], qc, n, groups={"g": ["l9.y"]})


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def engine(dim, recipe):
    from sparsernns_amd import floatmodel

    md, _, dims = model(dim, recipe)
    eng = floatmodel.FloatEngine(md, dims["n_layers"])
    assert eng.on_device
    return eng


@functools.lru_cache(maxsize=None)
def full_spec(dim, recipe):
    from sparsernns_amd import floatmodel

    _, qc, dims = model(dim, recipe)
    return floatmodel.fq_spec(qc, dims["n_layers"])


def host_planes(t):
    return {k: v.cpu().numpy() for k, v in t.items()}


def _plain(dim, case, recipe):
    _, _, dims = model(dim, recipe)
    x = make_x(dims, case, recipe)
    out = host_planes(engine(dim, recipe).forward_traced(x))
    out["x"] = x
    return out


_plain_small = functools.lru_cache(maxsize=None)(_plain)
_plain_stride = functools.lru_cache(maxsize=1)(_plain)  # up to 300 MB each: only the latest is kept


def plain(dim, case, recipe):
    """One plain traced forward per (dim, case, recipe), shared and never modified; host copies of every plane."""
    return (_plain_stride if case == STRIDE[1] else _plain_small)(dim, case, recipe)


def plane_order(n_layers):
    """The stored planes in the order the pipeline produces them."""
    return ["h_enc"] + [f"l{i}.{k}" for i in range(n_layers) for k in ("u", "Bu", "xs", "y", "g_in", "g", "h_out")] + ["out"]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", GRID + STRIDES_UP, ids=IDS + STRIDE_UP_IDS)
def test_no_spec_and_an_all_off_spec_are_the_plain_forward(dim, case):
    import torch
    from sparsernns_amd import floatmodel as F
    from sparsernns_amd._lib import lib

    recipe = "w8a8"
    eng = engine(dim, recipe)
    _, qc, dims = model(dim, recipe)
    t0 = plain(dim, case, recipe)
    off = F.fq_spec(qc, dims["n_layers"], [])
    for fq in (None, off):
        t = host_planes(eng.forward_traced(t0["x"], fq=fq))
        assert set(t) | {"x"} == set(t0)
        for k in t:
            assert same_bits(t[k], t0[k]), k
    x = torch.from_numpy(t0["x"]).to(eng.device)
    st = eng.new_stats()
    y = eng.forward_device(x, st, fq=off)
    assert same_bits(y.cpu().numpy(), t0["out"]) and same_bits(st.cpu().numpy(), t0["stats"])
    # the entry itself with fq = NULL
    B, L = x.shape[:2]
    n = lib.s5fxp_float_workspace_bytes(eng._h, B, L, 0)
    ws, yn, sn = torch.empty(n // 4, dtype=torch.float32, device=eng.device), torch.empty_like(y), eng.new_stats()
    assert lib.s5fxp_float_model_forward_fq(eng._h, x.data_ptr(), B, L, yn.data_ptr(), sn.data_ptr(), None, None, ws.data_ptr(), n,
                                            torch.cuda.current_stream().cuda_stream) == 0
    assert same_bits(yn.cpu().numpy(), t0["out"]) and same_bits(sn.cpu().numpy(), t0["stats"])


ONE_SITE = (0.25, CASES[0], "w8a8")
# per layer key: how many of the layer's planes (u, Bu, xs, y, g_in, g, h_out) lie upstream of the site, and the plane the
# site's own output is stored in
UPSTREAM = {"u": (0, "u"), "Bu_re": (1, "Bu"), "Bu_im": (1, "Bu"), "x_re": (3, None), "x_im": (3, None), "y": (3, "y"),
            "out2.inp": (4, None), "out2.out": (4, "g_in"), "gate.l": (6, None), "gate.r": (5, "g")}


def check_one_site(key, mode):
    from sparsernns_amd import floatmodel as F

    dim, case, recipe = ONE_SITE
    _, qc, dims = model(dim, recipe)
    n = dims["n_layers"]
    keys, order = F.stat_keys(n), plane_order(n)
    t0 = plain(dim, case, recipe)
    spec = F.fq_spec(qc, n, [key], mode=mode)
    t = host_planes(engine(dim, recipe).forward_traced(t0["x"], fq=spec))
    q = fq_of(key, spec, n)
    j = keys.index(key)
    # every observer up to and including the site's own
    assert same_bits(t["stats"][:j + 1], t0["stats"][:j + 1]), [k for k, a, b in zip(keys[:j + 1], t["stats"], t0["stats"]) if a != b]
    parts = key.split(".", 1)
    if parts[0] == "encoder":
        upstream, own = 0, None  # x is not stored, and h_enc lies behind the ReLU
    elif parts[0] == "decoder":
        upstream, own = len(order) - 1, "out" if parts[1] == "out" else None
    else:
        i = int(parts[0][1:])
        up, own = UPSTREAM[parts[1]]
        upstream, own = 1 + 7 * i + up, own and f"l{i}.{own}"
    for k in order[:upstream]:
        assert same_bits(t[k], t0[k]), (key, k)
    # the first plane behind the site is the one the quantiser must have moved
    behind = order[upstream] if own is None else own
    assert not np.array_equal(t[behind], t0[behind]), (key, behind)
    if own is None:
        return
    if parts[-1] == "Bu_re":
        assert np.array_equal(t[own].real, q(t0[own].real)) and same_bits(t[own].imag, t0[own].imag)
    elif parts[-1] == "Bu_im":
        assert np.array_equal(t[own].imag, q(t0[own].imag)) and same_bits(t[own].real, t0[own].real)
    else:
        assert np.array_equal(t[own], q(t0[own])), (key, own, int(np.count_nonzero(t[own] != q(t0[own]))))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["encoder.inp", "encoder.out"] + [f"l{i}.{k}" for i in range(3) for k in LAYER_KEYS] + ["decoder.inp", "decoder.out"])
def test_one_site_alone_is_exact(key):
    check_one_site(key, "floor")


@pytest.mark.gpu
def test_one_site_alone_is_exact_with_round_to_nearest():
    check_one_site("l1.y", "nearest")


def sandwich(dev, ref, lim, q, what, shares, post=lambda v: v):
    """q(ref - lim) <= dev <= q(ref + lim) element-wise; records the share of elements at which the two ends differ."""
    lo, hi = post(q(ref - lim)), post(q(ref + lim))
    loose = float(np.count_nonzero(lo != hi)) / lo.size
    shares[what] = max(shares.get(what, 0.0), loose)
    bad = np.count_nonzero((dev < lo) | (dev > hi) | np.isnan(dev))
    assert bad == 0, (what, int(bad), dev.size)


def sigmoid_bound(g_in):
    """|float32 1 / (1 + expf(-x)) - sigmoid(x)| for float32 x, derived; never above the 1e-6 the plain model's test uses.

    That 1e-6 cannot pin q here.  Under fake quantisation g_in is itself on a grid, and the sigmoid of some of its grid
    values lies next to a grid point of gate.r: sigmoid(0) = 0.5 IS one, sigmoid(+-2^-5) is 6.4e-7 from one, sigmoid(+-2^-6)
    7.9e-8 (1.3 ulp) -- and those few values of g_in hold 3 ... 17 % of the elements.  So the chain is bounded step by step:
    e^ = expf(-x) is within one ulp(e) of e (the HIP math API's stated accuracy), s^ = fl(1 + e^) adds at most ulp(s) / 2, and
    the correctly rounded division at most ulp(g) / 2; to first order
        |g^ - g| <= g / (1 + e) * (ulp(e) + ulp(1 + e) / 2) + ulp(g) / 2,
    taken with 2^-20 of relative slack for the second-order terms and for a result in the next binade.  At x = 0 nothing
    rounds at all -- expf(-0) is 1 (C Annex F), 1 + 1 and 1 / 2 are exact -- so the bound is 0 there and the device must
    give q(0.5) itself."""
    x = g_in.astype(np.float64)
    e = np.exp(-x)
    g = 1.0 / (1.0 + e)
    slack = 1 + 2.0 ** -20
    ulp = lambda v: 2.0 ** (np.floor(np.log2(v * slack)) - 23)
    b = (g / (1.0 + e) * (ulp(e) + ulp(1.0 + e) / 2) + ulp(g) / 2) * slack
    assert b.max() <= 1e-6
    return np.where(x == 0, 0.0, b)


def on_grid(plane, bits, exp, saturate, what):
    k = plane.astype(np.float64) * 2.0 ** exp
    assert np.array_equal(k, np.round(k)), what
    if saturate:
        assert k.min() >= -2 ** (bits - 1) and k.max() <= 2 ** (bits - 1) - 1, what


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("dim,case", GRID, ids=IDS)
def test_all_sites_on_every_stage_between_the_quantised_ends_of_its_bound(dim, case, recipe):
    check_all_sites_on(dim, case, recipe)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", STRIDES_UP, ids=STRIDE_UP_IDS)
def test_all_sites_on_where_workgroups_walk_two_tiles_at_the_other_dim_scales(dim, case):
    """GRID holds the walk at dim_scale 0.25 only; one recipe there, since the walk does not depend on it."""
    check_all_sites_on(dim, case, "w8a8")


def check_all_sites_on(dim, case, recipe, t=None):
    """``t``: host copies of the planes of a traced forward of ``make_x(dims, case, recipe)`` under ``full_spec(dim, recipe)`` that
    the caller ran on buffers of its own (tests/test_caller_memory.py); None: ``forward_traced`` runs it here."""
    from sparsernns_amd import floatmodel as F

    md, qc, dims = model(dim, recipe)
    n, H, P = dims["n_layers"], dims["H"], dims["P"]
    x = make_x(dims, case, recipe)
    spec = full_spec(dim, recipe)
    if t is None:
        t = host_planes(engine(dim, recipe).forward_traced(x, fq=spec))
    Q = lambda key: fq_of(key, spec, n)
    shares = {}
    relu = lambda v: np.maximum(v, 0)
    enc = md["encoder"]
    # every stored post-quantiser plane lies on its grid and inside its bounds
    for key, plane in ([("encoder.out", t["h_enc"]), ("decoder.out", t["out"])]
                       + [(f"l{i}.{k}", p) for i in range(n) for k, p in (("u", t[f"l{i}.u"]), ("Bu_re", t[f"l{i}.Bu"].real),
                                                                         ("Bu_im", t[f"l{i}.Bu"].imag), ("y", t[f"l{i}.y"]),
                                                                         ("out2.out", t[f"l{i}.g_in"]), ("gate.r", t[f"l{i}.g"]))]):
        bits, exp = F.quantiser_of(key, qc)
        on_grid(plane, bits, exp, True, key)
    v, S = R.stage_dense(Q("encoder.inp")(x), enc["encoder"]["kernel"], enc["encoder"]["bias"])
    sandwich(t["h_enc"], v, R.bound(257, S), Q("encoder.out"), "encoder.out", shares, post=relu)
    h = t["h_enc"]
    for i in range(n):
        layer = enc[f"layers_{i}"]
        lam_bar, B_bar, Cc = synth.zoh(layer["mixer"])
        u, y, g_in, g, h_out = (t[f"l{i}.{k}"] for k in ("u", "y", "g_in", "g", "h_out"))
        Bu, xs = t[f"l{i}.Bu"], t[f"l{i}.xs"]
        v, S = R.stage_u(h, layer["norm"])
        sandwich(u, v, R.bound(0, S), Q(f"l{i}.u"), "u", shares)
        (vr, Sr), (vi, Si) = R.stage_bu(u, B_bar)
        sandwich(Bu.real, vr, R.bound(H, Sr), Q(f"l{i}.Bu_re"), "Bu_re", shares)
        sandwich(Bu.imag, vi, R.bound(H, Si), Q(f"l{i}.Bu_im"), "Bu_im", shares)
        ref = R.scan_f64(lam_bar, Bu)  # the scan is the plain one, on the quantised Bu
        assert np.abs(xs - ref).max() <= 1e-5 * np.abs(ref).max()
        xq = (Q(f"l{i}.x_re")(xs.real) + 1j * Q(f"l{i}.x_im")(xs.imag)).astype(np.complex64)  # non-saturating, then the complex ReLU
        v, S = R.stage_y(xq, u, Cc, layer["mixer"]["D"])
        sandwich(y, v, R.bound(P, S), Q(f"l{i}.y"), "y", shares)
        x1 = relu(y)
        v, S = R.stage_dense(Q(f"l{i}.out2.inp")(x1), layer["out2"]["kernel"], layer["out2"]["bias"])
        sandwich(g_in, v, R.bound(H, S), Q(f"l{i}.out2.out"), "out2.out", shares)
        sig = R.sigmoid64(g_in)
        sandwich(g, sig, sigmoid_bound(g_in), Q(f"l{i}.gate.r"), "gate.r", shares)
        v, S = R.stage_hout(Q(f"l{i}.gate.l")(x1), g, h)  # no site on h': the plain chain bound
        assert (np.abs(h_out.astype(np.float64) - v) <= R.bound(0, S)).all(), f"l{i}.h_out"
        h = h_out
    v, S = R.stage_dense(Q("decoder.inp")(h), md["decoder"]["kernel"], md["decoder"]["bias"])
    sandwich(t["out"], v, R.bound(H, S), Q("decoder.out"), "decoder.out", shares)
    print(f"{recipe} dim {dim} {case[:2]}: share of elements not pinned (largest over the layers), per site: "
          + ", ".join(f"{k} {100 * s:.2f} %" for k, s in shares.items()))
    if recipe != "w8a16":  # at 16 bits the bound is wider than an LSB in places: the sandwich alone
        assert all(s <= 1.0 - PINNED_SHARE for s in shares.values()), shares
    # the observers: a site's observer holds the absmax of what entered it, so the quantised plane's absmax cannot exceed
    # q(observer) -- and the plain forward's observers are no longer these
    st = dict(zip(F.stat_keys(n), t["stats"]))
    for key, plane in (("decoder.out", t["out"]), ("l0.u", t["l0.u"]), (f"l{n - 1}.gate.r", t[f"l{n - 1}.g"])):
        assert np.abs(plane).max() <= max(abs(float(Q(key)(st[key]))), abs(float(Q(key)(-st[key])))), key


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [0.25, 0.5, 0.75, 1.0])  # every DS: the only runs of the k_*_clips_fq kernels
def test_clips_get_what_their_own_forward_gets(dim):
    import torch

    recipe = "w8a8"
    eng = engine(dim, recipe)
    _, _, dims = model(dim, recipe)
    spec = full_spec(dim, recipe)
    lens = [0, 1, 31, 32, 33, 70]
    x = torch.from_numpy(make_x(dims, (len(lens), 70, 21), recipe)).to(eng.device)
    ld = torch.tensor(lens, dtype=torch.int32, device=eng.device)
    y = torch.full_like(x, -7.25)
    st = eng.new_stats()
    assert eng.forward_clips_device(x, ld, st, out=y, fq=spec) is y
    want = eng.new_stats()
    for e, n in enumerate(lens):
        assert bool((y[e, n:] == -7.25).all()), e  # rows from len_e on keep the sentinel
        if n:
            ye = eng.forward_device(x[e:e + 1, :n], want, fq=spec)
            assert same_bits(y[e, :n].cpu().numpy(), ye[0].cpu().numpy()), e
    assert same_bits(st.cpu().numpy(), want.cpu().numpy())
    # and it is not the plain clip forward
    assert not torch.equal(eng.forward_clips_device(x, ld)[5], y[5])
    # the list form
    outs = eng.forward_clips([x[e, :n] for e, n in enumerate(lens)], fq=spec)
    assert all(torch.equal(o, y[e, :n]) for e, (o, n) in enumerate(zip(outs, lens)))


@pytest.mark.gpu
def test_a_nan_in_the_input_reaches_the_output():
    import torch

    dim, recipe = 0.25, "w8a8"
    eng = engine(dim, recipe)
    t0 = plain(dim, CASES[0], recipe)
    for mode_spec in (full_spec(dim, recipe), None):
        x = torch.from_numpy(t0["x"]).to(eng.device).clone()
        x[1, 7, 100] = float("nan")
        st = eng.new_stats()
        y = eng.forward_device(x, st, fq=mode_spec)
        assert bool(torch.isnan(y[1, 7]).all()) and bool(torch.isnan(st[0])) and bool(torch.isnan(st[-1]))
        assert not bool(torch.isnan(y[0]).any()) and not bool(torch.isnan(y[1, :7]).any())


@pytest.mark.gpu
def test_entries_refuse_a_bad_site_before_anything_is_launched():
    import torch
    from sparsernns_amd import floatmodel as F
    from sparsernns_amd._lib import lib

    dim, recipe = 0.25, "w8a8"
    eng = engine(dim, recipe)
    keys = eng.keys
    x = torch.from_numpy(plain(dim, CASES[0], recipe)["x"]).to(eng.device)
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

    good = full_spec(dim, recipe)
    for key, field, value in (("encoder.inp", "bits", 1), ("l0.u", "bits", 25), ("l1.y", "bits", -8), ("decoder.out", "exp", 41),
                              ("l2.gate.r", "exp", -25), ("l0.Bu_im", "mode", 2), ("l1.out2.inp", "saturate", 2),
                              ("l2.x_re", "saturate", 1), ("l0.x_im", "saturate", 1)):
        bad = good.copy()
        bad[field][keys.index(key)] = value
        assert both(bad) == -1, (key, field, value)
        with pytest.raises(ValueError, match=key):
            eng.forward_device(x, fq=bad)
    edge = good.copy()  # the ends of the accepted fields are accepted; what an off site holds besides bits = 0 is not read
    edge[0], edge[1], edge[2] = (2, -24, 1, 0), (24, 40, 0, 1), (0, 99, 9, 9)
    assert both(edge, need - 1) == -5  # the sites pass, the workspace does not
    assert both(good, need - 1) == -5
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and not bool(st.any())
    with pytest.raises(ValueError):
        eng.forward_device(x, hist_dev=eng.new_hist(), fq=good)
    with pytest.raises(ValueError):
        eng.forward_traced(x, hist=True, fq=good)


@pytest.mark.gpu
def test_sensitivity_on_the_device_is_the_hand_written_loop():
    import torch
    from sparsernns_amd import floatmodel as F

    dim, recipe = 0.25, "w8a8"
    md, qc, dims = model(dim, recipe)
    n = dims["n_layers"]
    eng = engine(dim, recipe)
    xa = make_x(dims, (2, 70, 31), recipe)
    xb = torch.from_numpy(make_x(dims, (3, 40, 32), recipe)).to(eng.device)
    lens = [40, 0, 17]
    got = F.sensitivity(md, [xa, (xb, lens)], qc, n, engine=eng)
    assert list(got) == F.stat_keys(n) + ["all"]

    def frames(fq):
        ya = eng.forward_device(torch.from_numpy(xa).to(eng.device), fq=fq).double().flatten()
        yb = [eng.forward_device(xb[e:e + 1, :m], fq=fq).double().flatten() for e, m in enumerate(lens) if m]
        return ya, torch.cat(yb)

    pa, pb = frames(None)
    num = float((pa * pa).sum() + (pb * pb).sum())
    for g in ("encoder.inp", "l0.x_re", "l1.y", "l2.gate.l", "decoder.out", "all"):
        qa, qb = frames(F.fq_spec(qc, n, None if g == "all" else [g]))
        den = float(((qa - pa) ** 2).sum() + ((qb - pb) ** 2).sum())
        assert got[g] == pytest.approx(10 * math.log10(num / den), rel=1e-9), g  # the same float64 sums in another order
    assert all(math.isfinite(v) for v in got.values())
    mixed = F.sensitivity(md, [xa], qc, n, groups={"layer1": [f"l1.{k}" for k in LAYER_KEYS]}, mode="nearest", engine=eng)
    assert list(mixed) == ["layer1", "all"] and mixed["layer1"] == mixed["all"]


@pytest.mark.gpu
def test_audio_wrappers_pass_the_spec_on():
    import torch
    from sparsernns_amd import audio

    dim, recipe = 0.5, "w8a8"
    eng = engine(dim, recipe)
    spec = full_spec(dim, recipe)
    rng = np.random.default_rng(4)
    T = 512 + 128 * 9
    noisy = torch.from_numpy((0.05 * rng.standard_normal((2, T))).astype(np.float32)).to(eng.device)
    clean = torch.from_numpy((0.05 * rng.standard_normal((2, T))).astype(np.float32)).to(eng.device)
    x = audio.stft_mag(noisy)
    mask = eng.forward(x, fq=spec)
    assert not torch.equal(mask, eng.forward(x))
    cleaned, cm = audio.mask_istft(noisy, mask, cleaned_mag=True)
    for a, b in zip(audio.denoise_float(eng, noisy, fq=spec), (cleaned, cm, x, mask)):
        assert torch.equal(a, b)
    loss, snr = audio.validate_float(eng, noisy, clean, lam=0.001, fq=spec)
    wl, ws, _ = audio.score_fused(noisy, clean, mask, 0.001)
    assert torch.equal(loss, wl) and torch.equal(snr, ws)
    # the clip forms: per clip bit for bit the rectangular wrapper on that clip alone
    Ts = (512, 512 + 128 * 9, 512 + 128 * 4 + 77)
    nc = [noisy[e % 2, :T_] for e, T_ in enumerate(Ts)]
    cc = [clean[e % 2, :T_] for e, T_ in enumerate(Ts)]
    cl, cs = audio.validate_float_clips(eng, nc, cc, lam=0.001, fq=spec)
    for e in range(len(Ts)):
        l1, s1 = audio.validate_float(eng, nc[e][None], cc[e][None], lam=0.001, fq=spec)
        assert torch.equal(cl[e:e + 1], l1) and torch.equal(cs[e:e + 1], s1), e
    for got, c in zip(audio.denoise_float_clips(eng, nc, fq=spec), nc):
        for a, b in zip(got, audio.denoise_float(eng, c[None], fq=spec)):
            assert torch.equal(a, b[0])
    assert not torch.equal(cs, audio.validate_float_clips(eng, nc, cc, lam=0.001)[1])
