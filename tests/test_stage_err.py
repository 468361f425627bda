"""s5fxp_stage_err and sparsernns_amd.verify: two forwards compared stage by stage where their planes lie.

The reference of every check is ``verify.stage_errors_host``, the NumPy float64 statement of the kernel's arithmetic, itself
held against ``fxpreporter.compute_error``.  Bounds (stated by the arithmetic, not measured):
  * counts, both histograms, max_abs and max_rel: exact;
  * each of the four sums adds n non-negative doubles, so any summation order is within (n - 1) * 2^-53 relative of the exact
    value: device and NumPy differ by at most 2 n 2^-53 relative;
  * the variance sum_sq / n - mean^2: 4 n 2^-53 * sum_sq / n absolute, the cancellation bound of its formula.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from sparsernns_amd import synth

EPS = 2.0 ** -53
EXACT = ("n", "n_nonfinite", "n_equal", "n_ref_nonzero", "max_abs", "max_rel")
SUM_KEYS = ("sum_abs", "sum_sq", "sum_ref_sq", "sum_rel")
I32_MIN = -2 ** 31


def variance(r):
    nf = r["n"] - r["n_nonfinite"]
    return r["sum_sq"] / nf - (r["sum_abs"] / nf) ** 2 if nf else 0.0


def assert_record(got, want, what):
    """A device record against the host record of the same values, to the bounds of the module docstring."""
    for k in EXACT:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("hist_abs", "hist_rel"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    n = want["n"]
    for k in SUM_KEYS:
        assert abs(got[k] - want[k]) <= 2 * n * EPS * abs(want[k]), (what, k, got[k], want[k])
    assert abs(variance(got) - variance(want)) <= 4 * EPS * want["sum_sq"], (what, variance(got), variance(want))
    for k in ("abs_error_med_lo", "abs_error_med_hi", "rel_error_med_lo", "rel_error_med_hi", "equal_share"):
        assert got[k] == want[k], (what, k)


def make_values(shape, kind, a_exp, seed):
    """(a, b): an int32 a over the full range (INT32_MIN included) or a float32 a, and a float32 b that equals a's value on
    part of the elements, is near it on others and far on the rest, with zeros of both signs, a NaN and both infinities."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == "i32":
        a = rng.integers(I32_MIN, 2 ** 31, size=n, dtype=np.int64)
        small = rng.random(n) < 0.5
        a[small] = rng.integers(-2 ** 20, 2 ** 20, size=int(small.sum()))
        if n > 3:
            a[0], a[1], a[2] = I32_MIN, 2 ** 31 - 1, 0
        a = a.astype(np.int32)
        va = a.astype(np.float64) * 2.0 ** -a_exp
    else:
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, size=n)).astype(np.float32)
        va = a.astype(np.float64)
    b = va.astype(np.float32)
    u = rng.random(n)
    near = (u > 0.4) & (u <= 0.8)
    b[near] = (va[near] * (1 + 1e-3 * rng.standard_normal(int(near.sum())))).astype(np.float32)
    far = u > 0.8
    b[far] = rng.standard_normal(int(far.sum())).astype(np.float32)
    if n >= 48:
        b[5], b[6], b[7], b[8], b[9] = 0.0, -0.0, np.nan, np.inf, -np.inf
        a[10], b[10] = 0, -0.0     # -0 equals +0
        a[11], b[11] = 0, 0.0
        if kind == "f32":
            a[12], a[13] = np.nan, -np.inf
    return a.reshape(shape), b.reshape(shape)


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,a_exp,relu", [("i32", 0, False), ("i32", 15, False), ("i32", 31, True), ("i32", 40, False),
                                             ("f32", 0, False), ("f32", 0, True)])
def test_host_statement_against_compute_error(kind, a_exp, relu):
    from sparsernns_amd import verify
    from sparsernns_amd.floatmodel import exp_hist
    from sparsernns_amd.fxpreporter import compute_error

    a, b = make_values((3, 41, 37), kind, a_exp, seed=7 + a_exp)
    fin = np.isfinite(b) & (np.isfinite(a) if kind == "f32" else True)
    r = verify.stage_errors_host([(a, b, a_exp, relu)])[0]
    va = a.astype(np.float64) * (2.0 ** -a_exp if kind == "i32" else 1.0)
    if relu:
        va = np.maximum(va, 0.0)
    xrec, xhat = va[fin], b.astype(np.float64)[fin]
    m = compute_error(xrec, xhat)
    n = a.size
    assert r["n"] == n and r["n_nonfinite"] == n - int(fin.sum()) > 0
    assert r["abs_error_max"] == m["abs_error_max"] and r["rel_error_max"] == m["rel_error_max"]
    assert abs(r["abs_error_mean"] - m["abs_error_mean"]) <= 2 * n * EPS * m["abs_error_mean"]
    assert abs(r["rel_error_mean"] - m["rel_error_mean"]) <= 2 * n * EPS * m["rel_error_mean"]
    assert abs(r["abs_error_std"] ** 2 - m["abs_error_std"] ** 2) <= 4 * EPS * r["sum_sq"] + 4 * EPS * m["abs_error_std"] ** 2
    assert r["abs_error_med_lo"] <= m["abs_error_med"] <= r["abs_error_med_hi"]
    assert r["rel_error_med_lo"] <= m["rel_error_med"] <= r["rel_error_med_hi"]
    e = np.abs(xrec - xhat)
    with np.errstate(over="ignore"):
        assert np.array_equal(r["hist_abs"], exp_hist(e.astype(np.float32)))
        assert np.array_equal(r["hist_rel"], exp_hist((e[xhat != 0] / np.abs(xhat[xhat != 0])).astype(np.float32)))
    assert r["n_equal"] == int(np.count_nonzero(e == 0)) > 0 and r["n_ref_nonzero"] == int(np.count_nonzero(xhat != 0))
    assert r["equal_share"] == r["n_equal"] / fin.sum()
    assert abs(r["sqnr_db"] - 10 * np.log10(r["sum_ref_sq"] / r["sum_sq"])) < 1e-9


def test_host_statement_edges():
    from sparsernns_amd import verify

    a = np.arange(-4, 4, dtype=np.int32).reshape(2, 4)
    same = verify.stage_errors_host([(a, (a / 4.0).astype(np.float32), 2)])[0]
    assert same["n_equal"] == same["n"] == 8 and same["sum_sq"] == 0.0 and same["sqnr_db"] == np.inf and same["equal_share"] == 1.0
    assert same["abs_error_med_lo"] == 0.0 and same["rel_error_max"] == 0.0 and same["n_ref_nonzero"] == 7
    empty = verify.stage_errors_host([(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), 0)])[0]
    assert empty["n"] == 0 and empty["abs_error_mean"] == 0.0 and not empty["hist_abs"].any()
    # even count, the two middle elements in different bins: the bracket spans both
    e = np.array([0.25, 0.25, 1.5, 1.5], dtype=np.float32)
    r = verify.stage_errors_host([(np.zeros(4, np.float32), e)])[0]
    assert r["abs_error_med_lo"] <= np.median(e) <= r["abs_error_med_hi"] and r["abs_error_med_lo"] <= 0.25 and r["abs_error_med_hi"] >= 1.5
    with pytest.raises(ValueError):
        verify.stage_errors_host([(np.zeros(3, np.int16), np.zeros(3, np.float32), 0)])


def test_pair_describes_strided_views_without_a_copy():
    import torch
    from sparsernns_amd import _lib, verify

    B, L, P, H = 3, 5, 4, 6
    bu = torch.arange(B * L * P * 2, dtype=torch.float32).view(B, L, P, 2)
    bu_c = torch.view_as_complex(bu)
    ai = torch.arange(B * L * P, dtype=torch.int32).view(B, L, P)
    d = _lib.StagePair()
    for half in (0, 1):
        p = verify.pair(ai, torch.view_as_real(bu_c)[..., half], a_exp=3)
        assert p.shape == (B, L, P) and p.a_stride == (L * P, P, 1) and p.b_stride == (2 * L * P, 2 * P, 2)
        p.fill(d)
        assert d.b == bu.data_ptr() + 4 * half and d.a == ai.data_ptr() and (d.a_kind, d.a_exp, d.flags) == (_lib.STAGE_I32, 3, 0)
        assert (d.nb, d.rows, d.cols) == (B, L, P) and list(d.b_stride) == [2 * L * P, 2 * P, 2]
    plane, ref = torch.zeros(B, L, H, dtype=torch.int32), torch.ones(B, L, H)
    s = verify.pair(plane[2], ref[2], a_exp=0, relu_a=True)       # one sequence
    s.fill(d)
    assert s.shape == (1, L, H) and s.a_stride == (0, H, 1) and d.a == plane.data_ptr() + 4 * 2 * L * H and d.flags == _lib.STAGE_RELU_A
    t = verify.pair(plane[:, 1:3], ref[:, 1:3], a_exp=0)          # one time bucket
    t.fill(d)
    assert t.shape == (B, 2, H) and t.a_stride == (L * H, H, 1) and d.b == ref.data_ptr() + 4 * H
    f = verify.pair(ref, ref)                                     # a float32 a needs no exponent
    assert f.kind == _lib.STAGE_F32 and f.a_exp == 0
    z = verify.pair(plane[:, 2:2], ref[:, 2:2], a_exp=0)
    z.fill(d)
    assert z.n == 0 and d.a is None and d.rows == 0
    for bad in (lambda: verify.pair(plane.to(torch.int16), ref, 0), lambda: verify.pair(plane, ref.double(), 0),
                lambda: verify.pair(plane, ref[:, :2], 0), lambda: verify.pair(plane, ref), lambda: verify.pair(plane, ref, 41),
                lambda: verify.pair(plane[None], ref[None], 0)):
        with pytest.raises(ValueError):
            bad()
    # pairs that are not on a GPU take the host statement, views included
    a, b = make_values((B, L, H), "i32", 9, seed=1)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    got = verify.stage_errors([verify.pair(ta[:, 1:4], tb[:, 1:4], 9), verify.pair(ta[1], tb[1], 9, relu_a=True)])
    want = verify.stage_errors_host([(a[:, 1:4], b[:, 1:4], 9), (a[1], b[1], 9, True)])
    for g, w in zip(got, want):
        assert all(np.array_equal(g[k], w[k]) for k in w)


def test_entry_refuses_bad_arguments_before_the_device():
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib

    FAKE = 1 << 20

    def one(**kw):
        arr = (_lib.StagePair * 1)()
        d = arr[0]
        d.a, d.b, d.a_kind, d.a_exp, d.nb, d.rows, d.cols, d.flags = FAKE, FAKE, _lib.STAGE_I32, 15, 2, 3, 4, 0
        for k in range(3):
            d.a_stride[k] = d.b_stride[k] = (12, 4, 1)[k]
        for k, v in kw.items():
            setattr(d, k, v)
        return arr

    need = lib.s5fxp_stage_err_workspace_bytes(1)
    assert need == 256 + 512 * C.sizeof(_lib.StageErrRec) and C.sizeof(_lib.StageErrRec) == 1104 and C.sizeof(_lib.StagePair) == 88
    assert lib.s5fxp_stage_err_workspace_bytes(0) == 0 and lib.s5fxp_stage_err_workspace_bytes(4097) == 0
    # the budget of workgroups per launch bounds the partial records of a call of many pairs
    assert 4096 * 4 * 1104 <= lib.s5fxp_stage_err_workspace_bytes(4096) < 32 << 20
    call = lambda arr, n=1, out=FAKE, ws=FAKE, nbytes=need: lib.s5fxp_stage_err(arr, n, out, ws, nbytes, None)
    assert call(None) == _lib.S5FXP_EBADARG
    assert call(one(), out=None) == _lib.S5FXP_EBADARG and call(one(), ws=None) == _lib.S5FXP_EBADARG
    assert call(one(), n=0) == _lib.S5FXP_EBADARG and call(one(), n=4097) == _lib.S5FXP_EBADARG
    for kw in (dict(a_kind=2), dict(a_kind=-1), dict(flags=2), dict(flags=-1), dict(a_exp=-1), dict(a_exp=41), dict(nb=-1),
               dict(rows=-1), dict(cols=-1), dict(a=None), dict(b=None),
               dict(nb=2 ** 31 - 1, rows=2 ** 31 - 1, cols=2 ** 31 - 1),   # the wrap rule, far beyond 64 bits
               dict(nb=512, rows=2 ** 31 - 1, cols=2)):                    # ... and just beyond it: 2^41 > 512 * (2^32 - 256)
        assert call(one(**kw)) == _lib.S5FXP_EBADARG, kw
    # everything legal, but no room: refused on the host as well
    for kw in (dict(), dict(a_kind=_lib.STAGE_F32, a_exp=99), dict(flags=_lib.STAGE_RELU_A), dict(a_exp=0), dict(a_exp=40),
               dict(rows=0, a=None, b=None), dict(nb=511, rows=2 ** 31 - 1, cols=2)):
        assert call(one(**kw), nbytes=need - 1) == _lib.S5FXP_EWORKSPACE, kw


def test_symbols_are_declared_and_exported_at_version_115():
    import re
    from sparsernns_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "s5fxp.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("s5fxp_stage_err", "s5fxp_stage_err_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert _lib.lib.s5fxp_version() == 115 and "#define S5FXP_VERSION 115" in hdr


def test_reporter_takes_rows_computed_elsewhere():
    from sparsernns_amd import verify
    from sparsernns_amd.fxpreporter import METRICS, Reporter

    a, b = make_values((2, 9, 8), "i32", 12, seed=3)
    row = verify.stage_errors_host([(a, b, 12)])[0]
    rep = Reporter(None)
    rep.add_block_raw("raw", xhat=np.ones(4), xrec=np.ones(4), verbose=False)
    rep.add_block_metrics("device row", row, verbose=False)
    got = rep.results_data[1]
    assert got["name"] == "device row" and got["abs_error_max"] == row["max_abs"] and got["sqnr_db"] == row["sqnr_db"]
    assert np.isnan(got["abs_error_med"]) and all(k in got for k in METRICS) and "device row" in rep.markdown()
    json.dumps([{k: v for k, v in r.items()} for r in rep.results_data])
    md = verify.table_markdown([dict(name="x", **row)])
    assert "| x |" in md and "equal_share" in md


# ----------------------------------------------------------------------------------------------------------------------
# MI355X
# ----------------------------------------------------------------------------------------------------------------------
def _cases():
    """name -> (a, b, a_exp, relu_a, view): host arrays of the BACKING tensors and the view both sides take."""
    full = lambda t: t
    out = {}
    out["1x1x48 exp0"] = (*make_values((1, 1, 48), "i32", 0, 11), 0, False, full)
    out["2x70x96 exp15"] = (*make_values((2, 70, 96), "i32", 15, 12), 15, False, full)
    out["2x70x96 exp15 relu"] = (*make_values((2, 70, 96), "i32", 15, 12), 15, True, full)
    out["2x70x96 exp31"] = (*make_values((2, 70, 96), "i32", 31, 13), 31, False, full)
    out["2x70x96 exp40 relu"] = (*make_values((2, 70, 96), "i32", 40, 14), 40, True, full)
    out["5x600x128 exp15"] = (*make_values((5, 600, 128), "i32", 15, 15), 15, False, full)   # 64 workgroups, ragged shares
    out["1x3x1367 f32"] = (*make_values((1, 3, 1367), "f32", 0, 16), 0, False, full)         # 4101 elements: two workgroups
    out["2x5x257 f32 relu"] = (*make_values((2, 5, 257), "f32", 0, 17), 0, True, full)
    out["300x3x1 exp7"] = (*make_values((300, 3, 1), "i32", 7, 18), 7, False, full)          # a lane step spans many rows and batches
    out["7x1x5 exp7"] = (*make_values((7, 1, 5), "i32", 7, 19), 7, False, full)
    out["2x3x700 exp20"] = (*make_values((2, 3, 700), "i32", 20, 20), 20, False, full)       # columns beyond one lane step
    out["zero extent"] = (*make_values((3, 4, 8), "i32", 3, 21), 3, False, lambda t: t[:, 2:2])
    out["one sequence of 4x70x96"] = (*make_values((4, 70, 96), "i32", 14, 22), 14, False, lambda t: t[2])
    out["one time slice of 4x70x96"] = (*make_values((4, 70, 96), "i32", 14, 22), 14, True, lambda t: t[:, 16:41])
    out["a 1-D view"] = (*make_values((4, 70, 96), "f32", 0, 23), 0, False, lambda t: t[1, 3])
    return out


@functools.lru_cache(maxsize=None)
def _suite():
    """Every case, the complex-half case and the equal case in ONE call; -> {name: (device record, host record)}."""
    import torch
    from sparsernns_amd import verify

    names, pairs = [], []
    for name, (a, b, a_exp, relu, view) in _cases().items():
        names.append(name)
        pairs.append(verify.pair(view(torch.from_numpy(a).cuda()), view(torch.from_numpy(b).cuda()), a_exp, relu))
    # (3,33,32) against the halves of an interleaved complex64 plane: column stride 2 on b
    a, b = make_values((3, 33, 32), "i32", 12, 24)
    _, b2 = make_values((3, 33, 32), "i32", 12, 25)
    z = torch.view_as_complex(torch.from_numpy(np.stack([b, b2], axis=-1)).cuda())
    ad = torch.from_numpy(a).cuda()
    for half in (0, 1):
        names.append(f"3x33x32 complex half {half}")
        pairs.append(verify.pair(ad, torch.view_as_real(z)[..., half], 12))
    # a equal to b everywhere, both kinds
    ai = np.random.default_rng(26).integers(-2 ** 23, 2 ** 23, size=(2, 70, 96)).astype(np.int32)
    names += ["equal i32", "equal f32"]
    bf = torch.from_numpy((ai * 2.0 ** -9).astype(np.float32)).cuda()
    pairs += [verify.pair(torch.from_numpy(ai).cuda(), bf, 9), verify.pair(bf, bf.clone())]
    got = verify.stage_errors(pairs)
    again = verify.stage_errors(pairs)
    want = verify.stage_errors_host(pairs)   # the same device tensors, copied back
    return {n: (g, w, g2, p) for n, g, w, g2, p in zip(names, got, want, again, pairs)}


SUITE_NAMES = list(_cases()) + ["3x33x32 complex half 0", "3x33x32 complex half 1", "equal i32", "equal f32"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SUITE_NAMES)
def test_records_equal_the_host_statement(name):
    got, want, again, p = _suite()[name]
    print(name, {k: (got[k], want[k]) for k in SUM_KEYS + EXACT})
    assert_record(got, want, name)
    assert want["n"] == p.n
    if name == "zero extent":
        assert got["n"] == 0 and all(not np.any(got[k]) for k in EXACT + SUM_KEYS + ("hist_abs", "hist_rel"))
    elif name.startswith("equal"):
        assert got["n_equal"] == got["n"] == 2 * 70 * 96 and got["sum_sq"] == 0.0 and got["max_abs"] == 0.0
    elif want["n"] >= 48 and "slice" not in name and "sequence" not in name and "view" not in name:
        assert got["n_nonfinite"] >= 3 and 0 < got["n_equal"] < got["n"] and got["n_ref_nonzero"] < got["n"] - got["n_nonfinite"]
    # two runs of the same call: identical bits
    for k in EXACT + SUM_KEYS + ("hist_abs", "hist_rel"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(again[k])), (name, k)


@pytest.mark.gpu
def test_two_hundred_pairs_of_different_sizes_in_one_call():
    import torch
    from sparsernns_amd import verify

    rng = np.random.default_rng(31)
    pairs = []
    for i in range(200):
        shape = (int(rng.integers(1, 4)), int(rng.integers(1, 40)), int(rng.integers(1, 300)))
        kind = "f32" if i % 5 == 0 else "i32"
        a_exp = int(rng.integers(0, 41))
        a, b = make_values(shape, kind, a_exp, 100 + i)
        pairs.append(verify.pair(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), a_exp, relu_a=bool(i % 3 == 0)))
    got, want = verify.stage_errors(pairs), verify.stage_errors_host(pairs)
    assert len(got) == 200
    for i, (g, w) in enumerate(zip(got, want)):
        assert_record(g, w, f"pair {i} {pairs[i].shape}")


RECIPES = ("w8a8", "w8a16")
MODEL_GRID = [(d, r, c) for d in (0.25, 1.0) for r in RECIPES for c in ((2, 70), (1, 1))]
MODEL_IDS = [f"dim{d}-{r}-B{c[0]}L{c[1]}" for d, r, c in MODEL_GRID]


@functools.lru_cache(maxsize=None)
def _model(dim, recipe):
    from sparsernns_amd import floatmodel
    from sparsernns_amd.fxpmodel import build_regression_model

    if recipe == "w8a16":
        md, qc, dims = synth.make_model(dim)
    else:
        md, qc, dims = synth.make_model(dim, quantization=recipe, bn_stats="random", input_scale=300.0)  # test_gpu_parity.py's 8-bit recipe
    n = dims["n_layers"]
    eng = build_regression_model(md, qc, n).engine()
    feng = floatmodel.FloatEngine(md, n)
    assert feng.on_device
    return md, qc, dims, eng, feng


@functools.lru_cache(maxsize=None)
def _quantised_weights_engine(dim, recipe):
    """The float model with the integer model's dequantised weights."""
    from sparsernns_amd import floatmodel

    md, qc, dims, _, _ = _model(dim, recipe)
    qeng = floatmodel.FloatEngine(floatmodel.quantised_modeldict(md, qc, dims["n_layers"]), dims["n_layers"])
    assert qeng.on_device
    return qeng


def _x(dims, recipe, case):
    return synth.make_input(case[0], case[1], dims["d_in"], seed=40 + case[1], scale=1.0 if recipe == "w8a16" else 300.0)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,recipe,case", MODEL_GRID, ids=MODEL_IDS)
def test_trace_exponents_are_the_eager_models(dim, recipe, case):
    from sparsernns_amd import verify
    from sparsernns_amd.fxparray import RoundingMode, fxp_from_fp
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims, eng, _ = _model(dim, recipe)
    x = _x(dims, recipe, case)
    fx = fxp_from_fp(x, bits=eng.inp_bits, exp=eng.inp_exp, signed=True, round_mode=RoundingMode.FLOOR, warn_on_clip=False)
    _, tr = eng.forward(fx, traces=True)
    exps = verify.trace_exponents(eng, qc)
    eager = build_regression_model(md, qc, dims["n_layers"], store_intermediates=True)
    eager(fx)
    for i, layer in enumerate(eager.encoder.seq_layers):
        li, mi = layer.intermediates, layer.mixer.intermediates
        u = li["pre_s5"][0].change_cfg(new_bits=layer.mixer.fxp_qconfig["activations"]["u"]["bits"],
                                       new_exp=layer.mixer.fxp_qconfig["activations"]["u"]["exp"], new_signed=True, warn_on_clip=False)
        want = dict(pre_s5=li["pre_s5"][0], u=u, Bu_re=mi["Bu_elements"][0].real, Bu_im=mi["Bu_elements"][0].imag,
                    xs_re=mi["xs"][0].real, xs_im=mi["xs"][0].imag, ys=mi["ys"][0], out2=layer.out2.intermediates["__call__"][0],
                    out2_sigmoid=li["out2_sigmoid"][0], post_GLU=li["post_GLU"][0], residadd=li["residadd"][0])
        assert set(want) == set(exps[i])
        for k, w in want.items():
            assert exps[i][k] == w.exp, (i, k, exps[i][k], w.exp)
            assert np.array_equal(tr[i][k].cpu().numpy(), w.data.cpu().numpy()), (i, k)  # the plane that exponent belongs to


@pytest.mark.gpu
@pytest.mark.parametrize("dim,recipe,case", MODEL_GRID, ids=MODEL_IDS)
def test_compare_engines_rows_equal_the_host_statement_in_every_mode(dim, recipe, case):
    from sparsernns_amd import verify

    md, qc, dims, eng, feng = _model(dim, recipe)
    x = _x(dims, recipe, case)
    B, L = case
    rows = verify.engine_rows(eng, feng, x, qc)
    assert len(rows) == 2 + 10 * dims["n_layers"]
    by_mode = {}
    for by in ("stage", "sequence", "time"):
        pairs, keys = verify._split(rows, by, 8)
        got, want = verify.stage_errors(pairs), verify.stage_errors_host(pairs)
        assert len(got) == len(rows) * {"stage": 1, "sequence": B, "time": len(range(0, L, -(-L // 8)))}[by]
        for k, g, w in zip(keys, got, want):
            assert_record(g, w, (by, k))
        # the public call: the same forwards again, the same rows, the same bits
        pub = verify.compare_engines(eng, feng, x, qc, by=by)
        assert [{k: r[k] for k in keys[0]} for r in pub] == keys
        for r, g in zip(pub, got):
            assert all(np.array_equal(np.asarray(r[k]), np.asarray(g[k])) for k in g), (by, r["name"])
        by_mode[by] = pub
    names = [r["name"] for r in by_mode["stage"]]
    assert names[0] == "inputs" and names[-1] == "decoder" and "encoder.layers_0.mixer.Bu (imag)" in names
    assert "encoder.layers_0.mixer.output" in names and len(set(names)) == len(names)
    for by in ("sequence", "time"):
        for s in by_mode["stage"]:
            parts = [r for r in by_mode[by] if r["name"] == s["name"]]
            for k in ("n", "n_nonfinite", "n_equal", "n_ref_nonzero", "hist_abs", "hist_rel"):
                assert np.array_equal(sum(np.asarray(r[k]) for r in parts), np.asarray(s[k])), (by, s["name"], k)
    assert by_mode["stage"][0]["n"] == B * L * dims["d_in"] and by_mode["stage"][-1]["n"] == B * L * dims["d_out"]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,recipe,case", MODEL_GRID, ids=MODEL_IDS)
def test_fake_quantised_float_side_agrees_on_more_of_Bu(dim, recipe, case):
    """With every site on, the float side's layer-0 ``Bu`` equals the integer model's on strictly more elements than with
    ``fq=None``.  ``equal_share`` is DESIGN.md §4v's figure, and §4v measures it on the float model that carries the integer
    model's weights (``quantised_modeldict``): that is the float side here.  Two sides that multiply ``u`` by different ``B``
    have no reason to meet on a grid -- on the float model with its own float weights the shares are 0 -> 0.496 (w8a8) and
    0 -> 0.019 (w8a16) at dim_scale 0.25, (2,70), and 0 of 32 -> 0 of 32 at w8a16, (1,1), so there the statement does not
    hold; DESIGN.md §4w has all sixteen figures.  With ``fq=None`` the share is not zero on this float side: the states whose
    row of the quantised ``B`` is all zero have ``Bu = 0`` on both."""
    from sparsernns_amd import floatmodel, verify

    md, qc, dims, eng, _ = _model(dim, recipe)
    n = dims["n_layers"]
    qeng = _quantised_weights_engine(dim, recipe)
    x = _x(dims, recipe, case)
    plain = {r["name"]: r for r in verify.compare_engines(eng, qeng, x, qc)}
    quant = {r["name"]: r for r in verify.compare_engines(eng, qeng, x, qc, fq=floatmodel.fq_spec(qc, n))}
    for name in ("encoder.layers_0.mixer.Bu (real)", "encoder.layers_0.mixer.Bu (imag)"):
        print(name, "n_equal with fq=None", plain[name]["n_equal"], "all sites", quant[name]["n_equal"], "of", quant[name]["n"])
        assert quant[name]["equal_share"] > plain[name]["equal_share"], name


@pytest.mark.gpu
@pytest.mark.parametrize("dim,recipe,case", MODEL_GRID, ids=MODEL_IDS)
def test_compare_float_is_exact_upstream_of_the_one_site(dim, recipe, case):
    from sparsernns_amd import floatmodel, verify

    md, qc, dims, eng, feng = _model(dim, recipe)
    x = _x(dims, recipe, case)
    rows = verify.compare_float(feng, x, floatmodel.fq_spec(qc, dims["n_layers"], ["l1.y"]))
    names = [r["name"] for r in rows]
    assert names[0] == "h_enc" and names[-1] == "out" and len(rows) == 2 + 9 * dims["n_layers"]
    cut = names.index("l1.y")
    for r in rows[:cut]:
        assert r["n_equal"] == r["n"] > 0 and r["sum_sq"] == 0.0, r["name"]
    assert rows[cut]["n_equal"] < rows[cut]["n"] and rows[cut]["sum_sq"] > 0.0
    assert rows[-1]["n_nonfinite"] == 0 and rows[-1]["sqnr_db"] < np.inf
    seq = verify.compare_float(feng, x, floatmodel.fq_spec(qc, dims["n_layers"], ["l1.y"]), by="sequence")
    assert len(seq) == len(rows) * case[0] and sum(r["n_equal"] for r in seq if r["name"] == "l1.y") == rows[cut]["n_equal"]


@pytest.mark.gpu
def test_fxprun_writes_the_device_stage_table(tmp_path):
    from sparsernns_amd import fxprun

    ap = fxprun.build_parser()
    assert ap.parse_args(["--synthetic", "--verify"]).stages == "host"
    rc = fxprun.main(["--synthetic", "--verify", "--stages", "device", "--report", str(tmp_path), "--dim_scale", "0.25",
                      "--bsz", "2", "--seq_len", "70", "--steps", "0"])
    assert rc == 0
    md = open(tmp_path / "stages_device.md").read()
    with open(tmp_path / "stages_device.json") as f:
        js = json.load(f)
    assert len(js["results"]) == 32 and js["results"][0]["name"] == "inputs" and js["results"][0]["n"] == 2 * 70 * 257
    assert "encoder.layers_2.mixer.output" in md and os.path.exists(tmp_path / "report.md")
    rc = fxprun.main(["--synthetic", "--verify", "--stages", "device", "--stage-by", "time", "--report", str(tmp_path / "t"),
                      "--dim_scale", "0.25", "--bsz", "2", "--seq_len", "70", "--steps", "0"])
    assert rc == 0
    with open(tmp_path / "t" / "stages_device.json") as f:
        assert len(json.load(f)["results"]) == 32 * 8
