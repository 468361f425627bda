"""Exponent histograms of the float model's observers and the clip-aware calibration built on them.

The reference of every test is ``floatmodel.exp_hist``, the NumPy statement of the histogram: bin clamp(E - 87, 0, 63) of the
float32 exponent field.  On the device a row must equal ``exp_hist`` of the device's OWN plane, integer for integer; the
calibration rule is checked on constructed histograms and against the host's configuration.  The shape at which workgroups
accumulate over two tiles (STRIDES) runs at every dim_scale: each is a kernel instantiation of its own.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import float_model_ref as R
from sparsernns_amd import synth

CASES = [(1, 1, 13), (2, 70, 11), (3, 33, 12)]  # test_float_model.py's shapes and seeds
DIMS_FOR = {(1, 1, 13): (0.25, 0.5), (2, 70, 11): (0.25, 0.5, 0.75, 1.0), (3, 33, 12): (0.25, 0.5)}
GRID = [(d, c) for c in CASES for d in DIMS_FOR[c]]
IDS = [f"dim{d}-B{c[0]}L{c[1]}" for d, c in GRID]
STRIDE_CASE = (5, 3300, 14)  # 516 tiles of 32 frames on a launch of at most 512 workgroups: four workgroups walk two tiles
STRIDES = [(d, STRIDE_CASE) for d in (0.25, 0.5, 0.75, 1.0)]  # every dim_scale is a kernel instantiation of its own
STRIDE_IDS = [f"dim{d}-B{c[0]}L{c[1]}" for d, c in STRIDES]
MARGIN = 2e-4
P_CLIP = 1e-3


@functools.lru_cache(maxsize=None)
def model(dim):
    return synth.make_model(dim)


@functools.lru_cache(maxsize=None)
def host_run(dim, case):
    """(x, stats, hist, planes) of synth.float_forward; planes = the observed tensors themselves, by key."""
    from sparsernns_amd import floatmodel

    md, _, dims = model(dim)
    x = synth.make_input(case[0], case[1], dims["d_in"], seed=case[2])
    st, hist, seen = {}, {}, []
    real = floatmodel.exp_hist

    def recording(v):
        seen.append(np.array(v, dtype=np.float32))
        return real(v)

    floatmodel.exp_hist = recording
    try:
        synth.float_forward(md, x, dims["n_layers"], stats=st, hist=hist)
    finally:
        floatmodel.exp_hist = real
    assert list(hist) == list(st) and len(seen) == len(st)
    return x, st, hist, dict(zip(st, seen))


def element_counts(dims, N):
    from sparsernns_amd import floatmodel

    out = {}
    for k in floatmodel.stat_keys(dims["n_layers"]):
        last = k.split(".")[-1]
        out[k] = N * (257 if k in ("encoder.inp", "decoder.out") else dims["P"] if last in ("Bu_re", "Bu_im", "x_re", "x_im")
                      else dims["H"])
    return out


def top_bin(row):
    return int(np.nonzero(row)[0].max())


def same_ints(a, b, path=""):
    assert set(a) == set(b), path
    for k in a:
        if isinstance(a[k], dict):
            same_ints(a[k], b[k], f"{path}.{k}")
        elif isinstance(a[k], (int, np.integer)):
            assert a[k] == b[k], (f"{path}.{k}", a[k], b[k])


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def test_exp_hist_on_hand_written_values():
    from sparsernns_amd import floatmodel

    f = np.float32
    vals = [f(0.0), f(-0.0), f(1e-40), f(2.0 ** -40), np.nextafter(f(2.0 ** -39), f(0)), f(2.0 ** -39), f(1.0),
            np.nextafter(f(2.0), f(0)), f(2.0 ** 23), f(np.inf), f(np.nan)]
    bins = [0, 0, 0, 0, 0, 1, 40, 40, 63, 63, 63]
    assert floatmodel.HIST_BINS == 64 and floatmodel.HIST_EMIN == -40
    for v, b in zip(vals, bins):
        for s in (v, -v):
            h = floatmodel.exp_hist(np.array([s], dtype=np.float32))
            assert h.dtype == np.int64 and h.shape == (64,) and h.sum() == 1 and h[b] == 1, (v, b, np.nonzero(h))
    want = np.bincount(bins, minlength=64)
    assert np.array_equal(floatmodel.exp_hist(np.array(vals, dtype=np.float32).reshape(1, 11)), want)
    # T(k) is the count of |v| >= 2^k
    row = floatmodel.exp_hist(np.array(vals))
    assert floatmodel.tail_count(row, 0) == 5 and floatmodel.tail_count(row, 1) == 3 and floatmodel.tail_count(row, -39) == 6
    assert floatmodel.tail_count(row, 23) == 3
    for k in (-40, 24):
        with pytest.raises(ValueError):
            floatmodel.tail_count(row, k)


def test_library_exports_the_hist_entry_and_keeps_its_version():
    from sparsernns_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    name = "s5fxp_float_model_forward_hist"
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and hasattr(_lib.lib, name)
    assert _lib.lib.s5fxp_version() == 115
    fake = 0x1000  # never dereferenced: the argument checks fail first
    assert _lib.lib.s5fxp_float_model_forward_hist(None, fake, 1, 1, fake, None, None, None, fake, 1 << 20, None) == -1


@pytest.mark.parametrize("dim,case", GRID, ids=IDS)
def test_host_histograms_count_every_element_once(dim, case):
    from sparsernns_amd import floatmodel

    _, _, dims = model(dim)
    _, st, hist, planes = host_run(dim, case)
    counts = element_counts(dims, case[0] * case[1])
    assert list(hist) == floatmodel.stat_keys(dims["n_layers"])
    for k, row in hist.items():
        assert row.dtype == np.int64 and row.shape == (64,) and int(row.sum()) == counts[k] == planes[k].size, k
        assert top_bin(row) == top_bin(floatmodel.exp_hist(np.float32(st[k]))), k
    # hist=None changes nothing
    x = host_run(dim, case)[0]
    md = model(dim)[0]
    st2 = {}
    synth.float_forward(md, x, dims["n_layers"], stats=st2)
    assert st2 == st


def test_clip_at_zero_is_the_identity(monkeypatch):
    import torch
    from sparsernns_amd import floatmodel

    dim, case = 0.25, CASES[1]
    md, _, dims = model(dim)
    x, st, hist, _ = host_run(dim, case)
    assert floatmodel.clip_absmax(st, hist, 0.0) == st
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    md8 = synth.make_model(dim, quantization="w8a8", bn_stats="random", input_scale=300.0)[0]  # test_gpu_parity.py's 8-bit recipe
    for q, m, xs in (("w8a16", md, x), ("w8a8", md8, x * np.float32(300.0))):
        s0, qc0 = floatmodel.calibrate(m, [xs, xs[:1]], dims["n_layers"], quantization=q, state_headroom_bits=1)
        s1, h1, eff, qc1 = floatmodel.calibrate_clipped(m, [xs, xs[:1]], dims["n_layers"], 0.0, quantization=q,
                                                        state_headroom_bits=1)
        assert s1 == s0 == eff and qc1 == qc0
        assert all(int(h1[k].sum()) == (140 + 70) * n // 140 for k, n in element_counts(dims, 140).items())
    with pytest.raises(ValueError):
        floatmodel.calibrate_clipped(md, [], dims["n_layers"], 0.0)
    with pytest.raises(ValueError):
        floatmodel.clip_absmax(st, hist, 1.0)


def test_clip_rule_on_constructed_histograms():
    from sparsernns_amd import floatmodel

    below = lambda k: float(np.nextafter(np.float32(2.0 ** k), np.float32(0)))

    def row(**bins):
        r = np.zeros(64, dtype=np.int64)
        for b, n in bins.items():
            r[int(b[1:])] = n
        return r

    # 1000 values: 990 in [2^-3, 2^-2), 9 in [2^2, 2^3), 1 in [2^5, 2^6); absmax 40 (intbits 6)
    h = row(b37=990, b42=9, b45=1)
    stats = {"l0.u": 40.0, "l0.x_re": 40.0, "l0.x_im": 40.0, "enc.other": 40.0}
    hist = {k: h for k in stats}
    # allowance 1: T(3) = T(4) = T(5) = 1 <= 1 and T(2) = 10 -> k* = 3, below the absmax's exponent
    out = floatmodel.clip_absmax(stats, hist, 1e-3)
    assert out["l0.u"] == below(3) and synth.get_intbits(out["l0.u"]) == 3 < synth.get_intbits(40.0) == 6
    assert out["l0.x_re"] == 40.0 and out["l0.x_im"] == 40.0  # keep
    assert floatmodel.clip_absmax(stats, hist, 1e-3, keep=("u",))["l0.u"] == 40.0
    assert floatmodel.clip_absmax(stats, hist, 1e-3, keep=())["l0.x_re"] == below(3)
    # allowance 10 reaches past the nine: T(-2) = 10 <= 10, T(-3) = 1000 -> k* = -2
    assert floatmodel.clip_absmax(stats, hist, 1e-2)["l0.u"] == below(-2)
    # allowance floor(p n) = 0: k* = 6 is the first k with T(k) = 0, above the absmax's exponent -> min() keeps the absmax
    assert floatmodel.clip_absmax(stats, hist, 0.9e-3)["l0.u"] == 40.0
    assert floatmodel.clip_absmax(stats, hist, 0.0) == stats
    # an absmax that is a power of two (get_intbits gives it one bit more): allowance 0 leaves it alone
    assert floatmodel.clip_absmax({"l0.y": 32.0}, {"l0.y": h}, 0.0)["l0.y"] == 32.0
    # k* at the absmax's exponent: one outlier exactly one bin up, absmax drops to just below 2^5
    h2 = row(b44=999, b45=1)
    assert floatmodel.clip_absmax({"l0.y": 40.0}, {"l0.y": h2}, 1e-3)["l0.y"] == below(5)
    assert synth.get_intbits(below(5)) == 5
    # everything in bin 63: T(23) = n > allowance for every k in range -> no clipping
    h3 = row(b63=1000)
    assert floatmodel.clip_absmax({"l0.y": 1e9}, {"l0.y": h3}, 0.5)["l0.y"] == 1e9
    # everything in bin 0: k* = -39, the effective absmax is min(absmax, just below 2^-39) = the absmax
    assert floatmodel.clip_absmax({"l0.y": 1e-30}, {"l0.y": row(b0=10)}, 0.5)["l0.y"] == 1e-30


def test_clip_rule_on_an_input_with_scaled_frames():
    """4 of the 2 x 70 frames are 64 times louder; a clip fraction above their share must size encoder.inp for the others."""
    from sparsernns_amd import floatmodel

    dim = 0.25
    md, _, dims = model(dim)
    x = synth.make_input(2, 70, dims["d_in"], seed=11, scale=300.0).copy()
    quiet_absmax = float(np.abs(x).max())
    for b, t in ((0, 3), (0, 40), (1, 0), (1, 69)):
        x[b, t] *= 64.0
    st, hist = {}, {}
    synth.float_forward(md, x, dims["n_layers"], stats=st, hist=hist)
    p = 0.03  # the loud frames are 4 / 140 = 2.86 % of the values
    row = floatmodel.exp_hist(x)
    assert np.array_equal(hist["encoder.inp"], row)
    allow = math.floor(p * x.size)
    kstar = min(k for k in range(-39, 24) if int(row[k + 40:].sum()) <= allow)
    want_intbits = max(0, kstar)
    eff = floatmodel.clip_absmax(st, hist, p)
    qc = synth.derive_qconfig(md, eff, dims["n_layers"])
    qc_abs = synth.derive_qconfig(md, st, dims["n_layers"])
    print(f"k* {kstar}, intbits {want_intbits} against absmax's {qc_abs['encoder']['inp_intbits']}; quiet absmax {quiet_absmax}")
    assert qc["encoder"]["inp_intbits"] == want_intbits < qc_abs["encoder"]["inp_intbits"] == synth.get_intbits(st["encoder.inp"])
    assert want_intbits <= synth.get_intbits(quiet_absmax)
    assert qc["encoder"]["inp_exp"] > qc_abs["encoder"]["inp_exp"]


def test_oracle_runs_the_clipped_configuration(monkeypatch):
    import torch
    from oracle import fxp_oracle as O
    from sparsernns_amd import floatmodel

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dim, case = 0.25, CASES[1]
    md, _, dims = model(dim)
    x, st, _, _ = host_run(dim, case)
    stats, hist, eff, qc = floatmodel.calibrate_clipped(md, [x], dims["n_layers"], P_CLIP)
    assert stats == st and sum(eff[k] != st[k] for k in st) > 0
    om = O.RegressionModel(md, qc, dims["n_layers"])
    y = om(O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR))
    assert y.data.shape == x.shape


def test_range_report_against_brute_force_counts():
    from sparsernns_amd import floatmodel

    dim, case = 0.25, CASES[1]
    md, _, dims = model(dim)
    _, st, hist, planes = host_run(dim, case)
    qc = synth.cap_result_exponents(synth.derive_qconfig(md, st, dims["n_layers"]))
    rep = floatmodel.range_report(hist, qc, dims["n_layers"])
    assert list(rep) == floatmodel.stat_keys(dims["n_layers"])
    some_below = 0
    for k, r in rep.items():
        bits, exp = floatmodel.quantiser_of(k, qc)
        a = np.abs(planes[k].astype(np.float64))
        assert r["total"] == a.size
        assert r["saturates"] == np.count_nonzero(a >= 2.0 ** (bits - 1 - exp)) / a.size, k
        assert r["below_lsb"] == 1.0 - np.count_nonzero(a >= 2.0 ** -exp) / a.size, k
        assert r["saturates"] == 0.0  # an absmax configuration saturates nothing it was calibrated on
        some_below += r["below_lsb"] > 0
    assert some_below
    assert floatmodel.quantiser_of("encoder.inp", qc) == (qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"])
    assert floatmodel.quantiser_of("l1.gate.r", qc) == (qc["blocks"]["multgate"]["r_bits"], qc["blocks"]["multgate"]["r_exp"])
    assert floatmodel.quantiser_of("l2.out2.out", qc) == (qc["blocks"]["out2"]["out_bits"], qc["blocks"]["out2"]["out_exp"])
    assert floatmodel.quantiser_of("l0.x_im", qc)[1] == qc["blocks"]["ssm"]["activations"]["x_im"]["exp"]
    # a clipped configuration does saturate: the report says how much
    eff = floatmodel.clip_absmax(st, hist, 1e-2)
    qcc = synth.cap_result_exponents(synth.derive_qconfig(md, eff, dims["n_layers"]))
    repc = floatmodel.range_report(hist, qcc, dims["n_layers"])
    assert 0.0 < max(r["saturates"] for r in repc.values()) <= 1e-2
    # thresholds the histogram cannot answer
    import copy
    bad = copy.deepcopy(qc)
    bad["encoder"]["inp_exp"] = 45  # LSB 2^-45 < 2^-39
    with pytest.raises(ValueError):
        floatmodel.range_report(hist, bad, dims["n_layers"])
    bad = copy.deepcopy(qc)
    bad["decoder"]["out_bits"], bad["decoder"]["out_exp"] = 32, 0  # saturation at 2^31 > 2^23
    with pytest.raises(ValueError):
        floatmodel.range_report(hist, bad, dims["n_layers"])


def test_float_engine_without_the_kernels_gathers_host_histograms(monkeypatch):
    import torch
    from sparsernns_amd import floatmodel

    dim, case = 0.25, CASES[2]
    md, _, dims = model(dim)
    x, st, hist, _ = host_run(dim, case)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    eng = floatmodel.FloatEngine(md, dims["n_layers"])
    got, got_st = {}, {}
    eng.forward(x, stats=got_st, hist=got)
    eng.forward(x, hist=got)
    assert got_st == st and all(np.array_equal(got[k], 2 * hist[k]) for k in hist)
    h0 = eng.new_hist()
    assert h0.dtype == torch.int64 and tuple(h0.shape) == (34, 64) and not h0.any()


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def engine(dim):
    from sparsernns_amd import floatmodel

    md, _, dims = model(dim)
    eng = floatmodel.FloatEngine(md, dims["n_layers"])
    assert eng.on_device
    return eng


def _traced(dim, case):
    md, _, dims = model(dim)
    x = synth.make_input(case[0], case[1], dims["d_in"], seed=case[2])
    t = engine(dim).forward_traced(x, hist=True)
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["x"] = x
    return out


_traced_small = functools.lru_cache(maxsize=None)(_traced)
_traced_stride = functools.lru_cache(maxsize=1)(_traced)  # up to 300 MB each: only the latest is kept


def traced(dim, case):
    """One traced forward with histograms per (dim, case), shared and never modified; host copies of every plane."""
    return (_traced_stride if case == STRIDE_CASE else _traced_small)(dim, case)


def device_planes(t, n_layers):
    want = {"encoder.inp": t["x"], "decoder.inp": t[f"l{n_layers - 1}.h_out"], "decoder.out": t["out"]}
    for i in range(n_layers):
        x1 = np.maximum(t[f"l{i}.y"], 0)
        want.update({f"l{i}.u": t[f"l{i}.u"], f"l{i}.Bu_re": t[f"l{i}.Bu"].real, f"l{i}.Bu_im": t[f"l{i}.Bu"].imag,
                     f"l{i}.x_re": t[f"l{i}.xs"].real, f"l{i}.x_im": t[f"l{i}.xs"].imag, f"l{i}.y": t[f"l{i}.y"],
                     f"l{i}.out2.inp": x1, f"l{i}.out2.out": t[f"l{i}.g_in"], f"l{i}.gate.l": x1, f"l{i}.gate.r": t[f"l{i}.g"]})
    return want


@functools.lru_cache(maxsize=None)  # a (dim, case) that passed is not counted through again; a failure is never cached
def check_rows_equal_planes(dim, case):
    from sparsernns_amd import floatmodel

    _, _, dims = model(dim)
    t = traced(dim, case)
    keys = floatmodel.stat_keys(dims["n_layers"])
    hist = dict(zip(keys, t["hist"]))
    stats = dict(zip(keys, t["stats"]))
    assert t["hist"].dtype == np.int64 and t["hist"].shape == (len(keys), 64)
    want = device_planes(t, dims["n_layers"])
    assert set(hist) == set(want) | {"encoder.out"}
    for k, plane in want.items():
        assert np.array_equal(hist[k], floatmodel.exp_hist(plane)), (k, np.nonzero(hist[k] - floatmodel.exp_hist(plane)))
    counts = element_counts(dims, case[0] * case[1])
    for k in keys:
        assert int(hist[k].sum()) == counts[k], k
    # encoder.out is observed before the ReLU and stored behind it
    row, post = hist["encoder.out"], floatmodel.exp_hist(t["h_enc"][t["h_enc"] > 0])
    assert top_bin(row) == top_bin(floatmodel.exp_hist(stats["encoder.out"]))
    assert (row[1:] >= post[1:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", GRID + STRIDES, ids=IDS + STRIDE_IDS)
def test_rows_equal_exp_hist_of_the_device_planes(dim, case):
    check_rows_equal_planes(dim, case)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", STRIDES, ids=STRIDE_IDS)
def test_grid_stride_workgroups_accumulate_over_several_tiles(dim, case):
    assert (case[0] * case[1] + 31) // 32 > 512
    check_rows_equal_planes(dim, case)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", GRID + STRIDES, ids=IDS + STRIDE_IDS)
def test_hist_changes_nothing_else_and_trace_changes_no_hist(dim, case):
    import torch
    from sparsernns_amd._lib import lib

    eng = engine(dim)
    t = traced(dim, case)
    x = torch.from_numpy(t["x"]).to(eng.device)
    B, L = x.shape[:2]
    # trace mode, without hist: y, stats, trace planes and the workspace planes (h, Bu, xs of every layer)
    st = eng.new_stats()
    y, tr, ws = eng.forward_device(x, st, trace=True)
    n_ws = lib.s5fxp_float_workspace_bytes(eng._h, B, L, 1) // 4
    y0, tr0, ws0 = y.clone(), tr.clone(), ws[:n_ws].clone()
    hd, st1 = eng.new_hist(), eng.new_stats()
    y1, tr1, ws1 = eng.forward_device(x, st1, trace=True, hist_dev=hd)
    assert torch.equal(y1.view(torch.int32), y0.view(torch.int32)) and torch.equal(st1.view(torch.int32), st.view(torch.int32))
    assert torch.equal(tr1.view(torch.int32), tr0.view(torch.int32)) and torch.equal(ws1[:n_ws].view(torch.int32), ws0.view(torch.int32))
    assert np.array_equal(hd.cpu().numpy(), t["hist"]) and np.array_equal(y0.cpu().numpy().view(np.uint32), t["out"].view(np.uint32))
    # hot mode: with and without hist, and the same histogram as in trace mode
    sa, sb, hb = eng.new_stats(), eng.new_stats(), eng.new_hist()
    ya = eng.forward_device(x, sa)
    yb = eng.forward_device(x, sb, hist_dev=hb)
    assert torch.equal(ya.view(torch.int32), y0.view(torch.int32)) and torch.equal(yb.view(torch.int32), y0.view(torch.int32))
    assert torch.equal(sa.view(torch.int32), st.view(torch.int32)) and torch.equal(sb.view(torch.int32), st.view(torch.int32))
    assert torch.equal(hb, hd)
    # hist without stats
    hc = eng.new_hist()
    assert torch.equal(eng.forward_device(x, None, hist_dev=hc).view(torch.int32), y0.view(torch.int32)) and torch.equal(hc, hd)
    # the new entry with hist = NULL is the old entry
    n = lib.s5fxp_float_workspace_bytes(eng._h, B, L, 0)
    wsn = torch.empty(n // 4, dtype=torch.float32, device=eng.device)
    yn, sn = torch.empty_like(y0), eng.new_stats()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.s5fxp_float_model_forward_hist(eng._h, x.data_ptr(), B, L, yn.data_ptr(), sn.data_ptr(), None, None,
                                              wsn.data_ptr(), n, stream) == 0
    assert torch.equal(yn.view(torch.int32), y0.view(torch.int32)) and torch.equal(sn.view(torch.int32), st.view(torch.int32))


@pytest.mark.gpu
def test_histogram_array_semantics():
    import torch
    from sparsernns_amd import floatmodel
    from sparsernns_amd._lib import lib

    dim = 0.5
    eng = engine(dim)
    _, _, dims = model(dim)
    ta, tb = traced(dim, CASES[1]), traced(dim, CASES[2])
    xa, xb = torch.from_numpy(ta["x"]).to(eng.device), torch.from_numpy(tb["x"]).to(eng.device)
    nk = len(eng.keys)
    # two inputs into one array = the sum of the two arrays; the words before and after are never touched
    buf = torch.zeros(nk * 64 + 2, dtype=torch.int64, device=eng.device)
    buf[0], buf[-1] = -1234567890123, 987654321987
    eng.forward_device(xa, None, hist_dev=buf[1:-1])
    eng.forward_device(xb, None, hist_dev=buf[1:-1])
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:-1].reshape(nk, 64), ta["hist"] + tb["hist"]) and not np.array_equal(ta["hist"], tb["hist"])
    assert got[0] == -1234567890123 and got[-1] == 987654321987
    # counts above 2^32 survive: the global counters are 64-bit
    big = eng.new_hist() + (1 << 40)
    eng.forward_device(xa, None, hist_dev=big)
    assert np.array_equal(big.cpu().numpy(), ta["hist"] + (1 << 40))
    # one NaN in the input: one more value in bin 63 of encoder.inp, and every row still counts every element
    xn = xa.clone()
    xn[1, 7, 100] = float("nan")
    hn = eng.new_hist()
    eng.forward_device(xn, None, hist_dev=hn)
    hn = hn.cpu().numpy()
    old_bin = top_bin(floatmodel.exp_hist(ta["x"][1, 7, 100]))
    want = ta["hist"][0].copy()
    want[63] += 1
    want[old_bin] -= 1
    assert np.array_equal(hn[0], want) and ta["hist"][0][63] == 0
    counts = element_counts(dims, xa.shape[0] * xa.shape[1])
    assert [int(r.sum()) for r in hn] == [counts[k] for k in eng.keys]
    assert hn[-1][63] == 257  # the frame's whole output row is NaN
    # the entry's own argument checks, on a live handle: nothing is launched
    B, L = xa.shape[:2]
    need = lib.s5fxp_float_workspace_bytes(eng._h, B, L, 0)
    ws, y = torch.empty(need // 4, device=eng.device), torch.full_like(xa, 7.0)
    h = eng.new_hist()
    call = lambda b, l, hp, n: lib.s5fxp_float_model_forward_hist(eng._h, xa.data_ptr(), b, l, y.data_ptr(), None, hp, None,
                                                                   ws.data_ptr(), n, None)
    assert call(B, L, h.data_ptr() + 4, need) == -1  # misaligned
    assert call(B, L, h.data_ptr(), need - 1) == -5
    assert call(0, L, h.data_ptr(), need) == -1
    assert call(1 << 17, 1 << 16, h.data_ptr(), need) == -1  # 2^33 frames: a 32-bit LDS counter could wrap
    assert call(1 << 17, 1 << 16, None, need) == -5  # without hist only the workspace is too small
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and not h.any()
    # forward() adds rows under float_forward's keys
    hd = {"l0.u": np.ones(64, dtype=np.int64)}
    eng.forward(ta["x"], hist=hd)
    assert list(hd)[0] == "l0.u" and set(hd) == set(eng.keys) and np.array_equal(hd["l0.u"], ta["hist"][2] + 1)
    assert np.array_equal(hd["decoder.out"], ta["hist"][-1]) and np.array_equal(eng.hist_dict(eng.new_hist() + 3)["l2.y"], np.full(64, 3))


# seed 19 at dim 0.25: with test_float_model.py's seed 12 one host count (l1.u at 2^2) equals its allowance, which is the
# precondition below, not a property of the code
CLIP_GRID = [(0.25, CASES[1]), (0.5, CASES[1]), (0.25, (3, 33, 19)), (0.5, CASES[2])]


def counts_on_their_allowance(hist, p):
    """The (key, k) at which a count the rule compares EQUALS its allowance, so that one value rounding across 2^k on the
    device could change k*.  With an allowance of 0 the rule cannot move an observer whatever the counts are (T(k) = 0 says
    absmax < 2^k already), so those keys have nothing to compare."""
    from sparsernns_amd import floatmodel

    out = []
    for k, row in hist.items():
        allow = math.floor(p * int(row.sum()))
        if k.split(".")[-1] in ("x_re", "x_im") or allow == 0:
            continue
        out += [(k, kk) for kk in range(-39, 24) if floatmodel.tail_count(row, kk) == allow]
    return out


@pytest.mark.parametrize("dim,case", CLIP_GRID, ids=[f"dim{d}-B{c[0]}L{c[1]}" for d, c in CLIP_GRID])
def test_host_counts_keep_clear_of_their_allowances(dim, case):
    """The preconditions of the device test, asserted on the CPU too (never skipped)."""
    _, st, hist, _ = host_run(dim, case)
    assert min(R.threshold_margin(v) for v in st.values()) >= MARGIN
    assert not counts_on_their_allowance(hist, P_CLIP)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", CLIP_GRID, ids=[f"dim{d}-B{c[0]}L{c[1]}" for d, c in CLIP_GRID])
def test_calibrate_clipped_on_the_device_gives_the_host_qconfig(dim, case):
    from sparsernns_amd import floatmodel

    md, _, dims = model(dim)
    x, st, hist, _ = host_run(dim, case)
    assert min(R.threshold_margin(v) for v in st.values()) >= MARGIN
    assert not counts_on_their_allowance(hist, P_CLIP)
    eff_host = floatmodel.clip_absmax(st, hist, P_CLIP)
    want = synth.cap_result_exponents(synth.derive_qconfig(md, eff_host, dims["n_layers"]))
    # two batches of whole sequences: the arrays are carried across them
    stats, h, eff, qc = floatmodel.calibrate_clipped(md, [x[:1], x[1:]], dims["n_layers"], P_CLIP, engine=engine(dim))
    assert set(h) == set(hist) and all(int(h[k].sum()) == int(hist[k].sum()) for k in hist)
    clipped = sorted(k for k in st if eff_host[k] != st[k])
    print(f"{len(clipped)} observers clipped: {clipped}")
    assert sorted(k for k in stats if eff[k] != stats[k]) == clipped
    assert all(eff[k] == eff_host[k] for k in clipped)
    same_ints(qc, want)


@pytest.mark.gpu
def test_integer_model_from_the_clipped_configuration_equals_the_c_reference():
    import torch
    from oracle import cref
    from sparsernns_amd import _lib, floatmodel
    from sparsernns_amd.fxparray import RoundingMode, fxp_from_fp
    from sparsernns_amd.fxpmodel import build_regression_model

    dim, case = 0.25, CASES[1]
    md, _, dims = model(dim)
    x, st, _, _ = host_run(dim, case)
    stats, _, eff, qc = floatmodel.calibrate_clipped(md, [x], dims["n_layers"], P_CLIP, engine=engine(dim))
    assert sum(eff[k] != stats[k] for k in stats) > 0
    m = build_regression_model(md, qc, dims["n_layers"])
    x2 = synth.make_input(2, 70, dims["d_in"], seed=21)
    fx = fxp_from_fp(x2, bits=qc["encoder"]["inp_bits"], exp=qc["encoder"]["inp_exp"], signed=True, round_mode=RoundingMode.FLOOR)
    y = m(fx)
    torch.cuda.synchronize()
    status = int(m.engine().status.cpu().numpy()[0])
    assert not status & (_lib.ST_NEGSHIFT | _lib.ST_NEGEXP), status
    ref, rb, re_, _ = cref.CModel(m.export()).forward(fx.numpy(), fx.bits, fx.exp)
    assert (y.bits, y.exp) == (rb, re_)
    assert torch.equal(torch.from_numpy(y.numpy()), torch.from_numpy(ref))
