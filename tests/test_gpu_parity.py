"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on identical integer inputs.

Bit-exact is the bar: every tensor is int32, so every comparison is array_equal.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth

TRACE_MAP = dict(pre_s5="pre_s5", u="u", Bu_re="bu_re", Bu_im="bu_im", xs_re="xs_re", xs_im="xs_im", ys="ys",
                 out2="out2", out2_sigmoid="sigmoid", post_GLU="post_glu", residadd="residadd")


def _make(cfg):
    md, qc, dims = synth.make_model(**cfg)
    return md, qc, dims


def _input(qc, dims, B, L, seed=0, scale=1.0):
    x = synth.make_input(B, L, dims["d_in"], seed=seed, scale=scale)
    return O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)


CASES = {
    "tiny": (dict(dims=synth.tiny_dims()), 3, 50, 1.0),
    "tiny_bnsb": (dict(dims=synth.tiny_dims(H=12, P=6, d_in=7, d_out=9, n_layers=3), bn_scale_bias=True,
                       input_scale=30.0), 2, 77, 30.0),
    "ndns05": (dict(dim_scale=0.5), 2, 200, 1.0),
    "ndns05_sparse": (dict(dim_scale=0.5, sparsity=0.9), 3, 130, 1.0),
    "ndns10": (dict(dim_scale=1.0, calib_L=128), 2, 96, 1.0),
    "ndns05_w4a8": (dict(dim_scale=0.5, quantization="w4a8", bn_stats="random", input_scale=300.0), 2, 100, 300.0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_fused_forward_matches_oracle(name):
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    cfg, B, L, scale = CASES[name]
    md, qc, dims = _make(cfg)
    model = build_regression_model(md, qc, dims["n_layers"])
    fx = _input(qc, dims, B, L, seed=5, scale=scale)
    cm = cref.CModel(model.export())
    ref, rb, re_, rtr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
    eng = model.engine()
    y, tr = eng.forward(FxpArray(fx.data, fx.bits, fx.exp), traces=True)
    exps = eng.layer_exponents()
    for i in range(dims["n_layers"]):
        assert exps[i]["residadd"] == rtr[i]["residadd_exp"], (i, exps[i], rtr[i]["residadd_exp"])
        for k, ck in TRACE_MAP.items():
            got = tr[i][k].cpu().numpy()
            assert np.array_equal(got, rtr[i][ck]), f"layer {i} {k}: {np.count_nonzero(got != rtr[i][ck])} mismatches"
    assert (y.bits, y.exp) == (rb, re_)
    assert np.array_equal(y.numpy(), ref)
    # same result without traces (the production path) and for a 2-D (L, d_in) input
    y2 = model(FxpArray(fx.data, fx.bits, fx.exp))
    assert np.array_equal(y2.numpy(), ref)


def test_two_d_input_and_ragged_tail():
    """(L, d_in) input as run_verification uses (fxprun.py:531-549); L not a multiple of the tile."""
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5))
    model = build_regression_model(md, qc, dims["n_layers"])
    cm = cref.CModel(model.export())
    for L in (1, 63, 65):
        fx = _input(qc, dims, 1, L, seed=L)
        x2 = fx.data[0]
        ref, _, _, _ = cm.forward(x2, fx.bits, fx.exp)
        y = model(FxpArray(x2, fx.bits, fx.exp))
        assert y.shape == (L, dims["d_out"])
        assert np.array_equal(y.numpy(), ref)


def _ran_fused(eng, n_layers, rung=None, lane=0):
    """What the forward that just ran on `lane` reports in its status words: the fused MFMA path, and (optionally) the
    recurrence kernel of every layer (include/s5fxp.h: status[2], status[8 + 8l + 5])."""
    from sparsernns_amd import _lib
    st = eng.lane_status(lane).cpu().numpy()
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    assert st[2] == _lib.PATH_FUSED, st[:8]
    if rung is not None:
        assert [int(st[8 + 8 * i + 5]) for i in range(n_layers)] == [rung] * n_layers, st[8:8 + 8 * n_layers]
    return st


@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("L", [3751, 4097, 7, 1])
def test_fused_path_at_any_sequence_length(B, L):
    """the fused kernels must serve every sequence length -- N-DNS clips are 3751 frames
    (sparseRNNs/dataloaders/dataloading.py:132-134: 3 mod 4), streams come a frame at a time.  The status words must say
    that the MFMA tile kernels and the LDS-fed pair recurrence (code 4) ran, and the output must be the oracle's."""
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5, calib_L=1024, state_headroom_bits=1))   # bench.py's configs[1] model
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    cm = cref.CModel(model.export())
    fx = _input(qc, dims, B, L, seed=40 + L % 7)
    ref, rb, re_, _ = cm.forward(fx.data, fx.bits, fx.exp)
    y = eng.forward(FxpArray(fx.data, fx.bits, fx.exp))
    assert (y.bits, y.exp) == (rb, re_)
    assert np.array_equal(y.numpy(), ref)
    st = _ran_fused(eng, dims["n_layers"], rung=4)
    assert not (st[0] & _lib.ST_REDO) and eng.level == 0   # served by the top rung, no step down
    # the self-contained form (gated exact kernels enqueued, int32 streams) and the traced form take the same tails
    y2, tr = eng.forward(FxpArray(fx.data, fx.bits, fx.exp), traces=True, check_status=False)
    assert np.array_equal(y2.numpy(), ref)
    _ran_fused(eng, dims["n_layers"], rung=1)
    if B == 1:
        _, _, _, rtr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
        for i in range(dims["n_layers"]):
            for k, ck in TRACE_MAP.items():
                assert np.array_equal(tr[i][k].cpu().numpy(), rtr[i][ck]), f"layer {i} {k}"


def test_ragged_tail_does_not_leak_into_the_range_check():
    """The steps of a sequence's last 4-step block beyond L are computed by the recurrence too (the B projection fills them
    with the last frame's Bu).  A sequence that ends on a burst keeps growing through those steps: the states there leave
    every fast kernel's range while the L real ones do not.  They must not raise ST_REDO (a needless step down the
    ladder), whichever rung runs, and the output must be the oracle's."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5, calib_L=1024, state_headroom_bits=1))   # bench.py's configs[1] model
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    cm = cref.CModel(model.export())
    B, L = 3, 61                                               # 61 = 1 mod 4: three computed-but-unreal steps per sequence
    xf = synth.make_input(B, L, dims["d_in"], seed=8)
    xf[:, -1, :] *= 400.0                                      # the burst: saturates Bu in the last frame
    fx = O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    ref, _, _, rtr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
    tops = [max(int(np.abs(t["xs_re"]).max()), int(np.abs(t["xs_im"]).max())) for t in rtr]
    bounds = [_lib.lib.s5fxp_model_recurrence_xmax(eng._h, i) for i in range(dims["n_layers"])]
    assert all(t <= b for t, b in zip(tops, bounds)), (tops, bounds)   # the real states fit the top rung
    # what the kernel computes for the three extra steps of layer 0 = the oracle on the sequence with its last frame
    # repeated (same extremes, hence the same exponents, in layer 0): those states are beyond every 16-bit bound
    xpad = np.concatenate([fx.data, np.repeat(fx.data[:, -1:, :], 3, axis=1)], axis=1)
    _, _, _, ptr = cm.forward(xpad, fx.bits, fx.exp, trace=True)
    assert max(int(np.abs(ptr[0]["xs_re"][:, L:]).max()), int(np.abs(ptr[0]["xs_im"][:, L:]).max())) > 32767
    x = torch.from_numpy(fx.data).cuda()
    for flags, rung in ((_lib.FWD_DEFER_REDO, 4), (_lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, 2), (0, 1), (_lib.FWD_EXACT, 5)):
        y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        eng.enqueue(x, fx.bits, fx.exp, y, B, L, flags=flags)
        st = _ran_fused(eng, dims["n_layers"], rung=rung)
        assert not (st[0] & (_lib.ST_REDO | _lib.ST_WIDE_STATE)), (flags, st[:8])
        assert np.array_equal(y.cpu().numpy(), ref), flags


@pytest.mark.parametrize("case", ["ndns05", "ndns10", "generic"])
def test_grouped_forward_equals_one_forward_per_batch(case):
    """s5fxp_forward_opts::groups: G reference batches in ONE set of launches (gridDim.y = G) must give, group by group, what
    G separate forwards give -- each group its own compute_best exponents (the groups get inputs of different scale, so the
    exponents differ), its own status words, its own streaming carry; ragged L; one group that overflows the fast
    recurrence takes the whole call down the ladder and the result is still the oracle's.  The generic engine takes the
    per-group loop behind the same call."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    cfg = dict(dim_scale=1.0, calib_L=128) if case == "ndns10" else dict(dim_scale=0.5, calib_L=1024, state_headroom_bits=1)
    md, qc, dims = _make(cfg)
    model = build_regression_model(md, qc, dims["n_layers"], engine_flags=_lib.MODEL_FORCE_GENERIC if case == "generic" else 0)
    eng = model.engine()
    cm = cref.CModel(model.export())
    G, B, L = 3, 4, 203 if case != "generic" else 61
    scales = (1.0, 0.25, 2.0)
    parts = [_input(qc, dims, B, L, seed=70 + g, scale=scales[g]) for g in range(G)]
    bits, exp = parts[0].bits, parts[0].exp
    x = np.concatenate([p.data for p in parts])
    refs, ref_state = [], np.zeros((G, dims["n_layers"], 2, B, dims["P"]), dtype=np.int32)
    res_exps = []
    for g in range(G):
        r, rb, re_, rtr = cm.forward(parts[g].data, bits, exp, trace=True, state=ref_state[g])
        refs.append(r)
        res_exps.append([t["residadd_exp"] for t in rtr])
    assert len({tuple(e) for e in res_exps}) > 1       # the groups really choose different exponents
    y = eng.forward_batches(FxpArray(x, bits, exp), B)
    assert (y.bits, y.exp) == (rb, re_)
    assert np.array_equal(y.numpy(), np.concatenate(refs))
    st = eng.lane_status(0, G).cpu().numpy()
    for g in range(G):
        w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
        assert w[2] == (_lib.PATH_GENERIC if case == "generic" else _lib.PATH_FUSED)
        assert [int(w[8 + 8 * i + 4]) for i in range(dims["n_layers"])] == res_exps[g], g
    # the carry, group by group
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
    s_in = torch.zeros((G, dims["n_layers"], 2, B, dims["P"]), dtype=torch.int32, device="cuda")
    s_out = torch.empty_like(s_in)
    eng.run_ladder(lambda fl: eng.enqueue(xd, bits, exp, yd, B, L, flags=fl, groups=G, state_in=s_in, state_out=s_out), eng.check_status)
    assert np.array_equal(s_out.cpu().numpy(), ref_state)
    assert np.array_equal(yd.cpu().numpy(), np.concatenate(refs))
    if case == "generic":
        return
    # one group leaves the fast range: ST_REDO comes back for the call, the ladder repeats it, every group is still right
    big = _input(qc, dims, B, L, seed=99, scale=40.0)
    x2 = np.concatenate([parts[0].data, big.data, parts[2].data])
    rbig, _, _, _ = cm.forward(big.data, bits, exp)
    eng.level = 0
    y2 = eng.forward_batches(FxpArray(x2, bits, exp), B)
    assert np.array_equal(y2.numpy(), np.concatenate([refs[0], rbig, refs[2]]))
    # and the self-contained form (gated exact kernels enqueued for every group)
    eng.enqueue(torch.from_numpy(x2).cuda(), bits, exp, yd, B, L, flags=0, groups=G)
    eng.check_status()
    assert np.array_equal(yd.cpu().numpy(), np.concatenate([refs[0], rbig, refs[2]]))


def test_eager_matches_fused_and_names_intermediates():
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dims=synth.tiny_dims(H=12, P=6, d_in=7, d_out=9, n_layers=2), bn_scale_bias=True,
                              input_scale=30.0))
    fx = _input(qc, dims, 2, 40, seed=1, scale=30.0)
    fused = build_regression_model(md, qc, dims["n_layers"])
    eager = build_regression_model(md, qc, dims["n_layers"], store_intermediates=True)
    yf = fused(FxpArray(fx.data, fx.bits, fx.exp))
    ye = eager(FxpArray(fx.data, fx.bits, fx.exp))
    assert (yf.bits, yf.exp) == (ye.bits, ye.exp)
    assert np.array_equal(yf.numpy(), ye.numpy())
    # the numpy oracle names the same stages
    om = O.RegressionModel(md, qc, dims["n_layers"])
    inter = {}
    yo = om(fx, inter)
    assert np.array_equal(yo.data, ye.numpy())
    l0 = eager.encoder.seq_layers[0]
    for key in ("ssm_input", "pre_s5", "pre_C", "pre_GLU", "out2_sigmoid", "post_GLU", "residadd", "output"):
        assert key in l0.intermediates, key
    for key in ("Bu_elements", "xs", "xs_relu", "Cxs", "2Cxs", "Du", "ys"):
        assert key in l0.mixer.intermediates, key
    for key in ("norm_input", "norm_input_minus_mean", "norm_output_raw", "norm_output_scaled",
                "norm_output_scaled_bias", "norm_output"):
        assert key in l0.norm.intermediates, key
    fl = O.flatten_intermediates(inter)
    chk = {"layers_0.norm.norm_input_minus_mean": l0.norm.intermediates["norm_input_minus_mean"][-1],
           "layers_0.norm.norm_output_scaled": l0.norm.intermediates["norm_output_scaled"][-1],
           "layers_0.mixer.Cxs": l0.mixer.intermediates["Cxs"][-1],
           "layers_0.mixer.Cxs2": l0.mixer.intermediates["2Cxs"][-1],
           "layers_0.mixer.Du": l0.mixer.intermediates["Du"][-1],
           "layers_0.residadd": l0.intermediates["residadd"][-1]}
    for k, got in chk.items():
        assert (got.bits, got.exp) == (fl[k].bits, fl[k].exp), k
        assert np.array_equal(got.numpy(), fl[k].data), k
    data = eager.export()
    assert set(data) == {"params", "qconfig", "intermediates"}
    assert "pre_encoder" in data["intermediates"]["encoder"]


# ------------------------------------------------------------------------------------------
# op level
# ------------------------------------------------------------------------------------------
def _rand(rng, shape, bits):
    return rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=shape, dtype=np.int64).astype(np.int32)


def test_ops_match_numpy_oracle():
    from sparsernns_amd import fxparray as G

    rng = np.random.default_rng(0)
    a = _rand(rng, (3, 37, 24), 16)
    b = _rand(rng, (3, 37, 24), 16)
    v = _rand(rng, (24,), 16)
    A, B, V = G.FxpArray(a, 16, 12), G.FxpArray(b, 16, 9), G.FxpArray(v, 16, 14)
    oa, ob, ov = O.Fx(a, 16, 12), O.Fx(b, 16, 9), O.Fx(v, 16, 14)

    def same(g, o):
        assert (g.bits, g.exp) == (o.bits, o.exp), ((g.bits, g.exp), (o.bits, o.exp))
        assert np.array_equal(g.numpy(), o.data)

    same(G.fxp_add(A, B, result_bits=16, result_exp=10), O.add(oa, ob, 16, 10))
    same(G.fxp_add(A, B, result_bits=16, result_exp=13), O.add(oa, ob, 16, 13))
    same(G.fxp_add(A, V, result_bits=16, result_exp=12), O.add(oa, ov, 16, 12))
    same(G.fxp_sub(A, B, result_bits=16, result_exp=9), O.sub(oa, ob, 16, 9))
    same(G.fxp_add(A, B, result_exp="compute_best"), O.add(oa, ob, None, "compute_best"))
    same(G.fxp_add(A, V, result_exp="compute_best"), O.add(oa, ov, None, "compute_best"))
    same(G.fxp_mul(A, V, result_exp="compute_best"), O.mul(oa, ov, None, "compute_best"))
    same(G.fxp_mul(A, B, result_bits=16, result_exp=8), O.mul(oa, ob, 16, 8))
    same(G.fxp_mul(V, A, result_bits=16, result_exp=11), O.mul(ov, oa, 16, 11))
    same(G.fxp_change_cfg(A, 12, 8, True), O.change_cfg(oa, 12, 8, True))
    same(G.fxp_change_cfg(A, 20, 15, True), O.change_cfg(oa, 20, 15, True))
    same(G.fxp_change_exp(A, 14), O.change_exp(oa, 14))
    same(G.fxp_change_exp(A, 12), O.change_exp(oa, 12))
    with pytest.raises(ValueError):
        G.fxp_mul(A, B, result_bits=16, result_exp=30)
    # int32 wrap in mul and the unclipped pass-through of change_exp
    big = _rand(rng, (1000,), 32)
    same(G.fxp_mul(G.FxpArray(big, 32, 4), G.FxpArray(big[::-1].copy(), 32, 3), result_bits=32, result_exp=2),
         O.mul(O.Fx(big, 32, 4), O.Fx(big[::-1].copy(), 32, 3), 32, 2))
    same(G.fxp_clip(G.FxpArray(big, 16, 4)), O.Fx(O.sat(big, 16), 16, 4))
    # from_fp in the three rounding modes incl. ties
    xf = np.concatenate([rng.normal(0, 3, 5000), np.arange(-40, 40) / 16.0 + 1 / 32.0]).astype(np.float32)
    for mode, om in ((G.RoundingMode.FLOOR, O.FLOOR), (G.RoundingMode.ROUND, O.ROUND), (G.RoundingMode.CEIL, O.CEIL)):
        same(G.fxp_from_fp(xf, 8, 4, True, mode), O.from_fp(xf, 8, 4, True, om))
    g = G.FxpArray(a, 16, 12).to_float().cpu().numpy()
    assert np.array_equal(g, oa.f32())


def test_matmul_generic_wraps_like_int32():
    from sparsernns_amd import fxparray as G

    rng = np.random.default_rng(1)
    for (N, K, M) in ((130, 257, 96), (64, 64, 257), (5, 3, 1), (70, 96, 128)):
        x = _rand(rng, (N, K), 32)  # full-range operands: the accumulation must wrap modulo 2^32
        w = _rand(rng, (K, M), 32)
        got = G.fxp_matmul(G.FxpArray(x, 32, 10), G.FxpArray(w, 32, 5), result_bits=24, result_exp=9)
        ref = O.matmul(O.Fx(x, 32, 10), O.Fx(w, 32, 5), 24, 9)
        assert np.array_equal(got.numpy(), ref.data)
    x = _rand(rng, (2, 33, 40), 16)
    w = _rand(rng, (40, 12), 8)
    got = G.fxp_matmul(G.FxpArray(x, 16, 12), G.FxpArray(w, 8, 7), result_bits=16, result_exp=11)
    assert np.array_equal(got.numpy(), O.matmul(O.Fx(x, 16, 12), O.Fx(w, 8, 7), 16, 11).data)


def test_scan_and_relu_edge_cases():
    import torch
    from sparsernns_amd import fxparray as G
    from sparsernns_amd._lib import check, lib
    from sparsernns_amd.fxpmodel import fxp_relu

    rng = np.random.default_rng(2)
    for (B, L, P, bits, ea, sh) in ((3, 70, 5, 16, 15, 1), (2, 33, 64, 16, 15, -2), (1, 1, 1, 16, 12, 0),
                                    (2, 50, 7, 30, 15, 1)):  # the last one overflows int32 in A*x: wrap must match
        bre, bim = _rand(rng, (B, L, P), bits), _rand(rng, (B, L, P), bits)
        ar, ai = _rand(rng, (P,), 16), _rand(rng, (P,), 16)
        e_bu, e_x = 15, 15 - sh
        orr, oi = O.scan(O.Fx(bre, 16, e_bu), O.Fx(bim, 16, e_bu), O.Fx(ar, 16, ea), O.Fx(ai, 16, ea), e_x, e_x)
        t = lambda a: torch.as_tensor(a).cuda()
        dbre, dbim, dar, dai = t(bre), t(bim), t(ar), t(ai)
        for flags in (0, 1):
            xr, xi = torch.empty_like(dbre), torch.empty_like(dbim)
            check(lib.s5fxp_scan(dbre.data_ptr(), dbim.data_ptr(), dar.data_ptr(), dai.data_ptr(), xr.data_ptr(),
                                 xi.data_ptr(), B, L, P, ea, ea, e_bu, e_bu, e_x, e_x, flags,
                                 torch.cuda.current_stream().cuda_stream))
            if flags:
                er, ei = O.complex_relu(O.Fx(orr, 16, e_x), O.Fx(oi, 16, e_x))
                er, ei = er.data, ei.data
            else:
                er, ei = orr, oi
            assert np.array_equal(xr.cpu().numpy(), er) and np.array_equal(xi.cpu().numpy(), ei)
    # complex ReLU truth table incl. float32 round trip of wide values
    re = np.array([5, 0, 0, 0, -3, 2**24 + 1, -(2**24) - 1, 7, 2**31 - 1], dtype=np.int64).astype(np.int32)
    im = np.array([-9, 4, 0, -4, 8, 2**24 + 3, 5, 2**30 + 1, -(2**31)], dtype=np.int64).astype(np.int32)
    out = fxp_relu(G.ComplexFxpArray(G.FxpArray(re, 16, 3), G.FxpArray(im, 16, 3)))
    er, ei = O.complex_relu(O.Fx(re, 16, 3), O.Fx(im, 16, 3))
    assert np.array_equal(out.real.numpy(), er.data) and np.array_equal(out.imag.numpy(), ei.data)


def test_sigmoid_lut_all_inputs():
    from sparsernns_amd import fxparray as G
    from sparsernns_amd.fxpmodel import FxpSigmoid

    allv = np.arange(-(1 << 15), 1 << 15, dtype=np.int32)
    for (xe_in, bits) in ((12, 16), (6, 16), (4, 16), (9, 8)):
        x_exp, y_exp = min(xe_in, 6), bits - 2
        s = FxpSigmoid(x_exp=x_exp, y_exp=y_exp)
        lut = O.sigmoid_lut(x_exp, y_exp)
        assert np.array_equal(s.lut, lut)
        v = allv if bits == 16 else np.arange(-128, 128, dtype=np.int32)
        got = s.apply(G.FxpArray(v, bits, xe_in))
        ref = O.sigmoid_apply(O.Fx(v, bits, xe_in), x_exp, y_exp, lut)
        assert (got.bits, got.exp) == (ref.bits, ref.exp)
        assert np.array_equal(got.numpy(), ref.data)


def test_compute_best_thresholds_near_powers_of_two():
    """ceil(log2(max + eps)) either side of powers of two: GPU finalize == oracle definition."""
    from sparsernns_amd import fxparray as G

    for k in range(0, 15):
        for delta in (-2, -1, 0, 1, 2, 3, 6):
            v = (1 << k) * 64 + delta  # value/2^6 sits next to 2^k
            if v <= 0 or v >= (1 << 23):
                continue
            a = np.array([v, -3, 0, 1], dtype=np.int32)
            z = np.zeros(4, dtype=np.int32)
            got = G.fxp_add(G.FxpArray(a, 24, 6), G.FxpArray(z, 24, 6), result_exp="compute_best")
            ref = O.add(O.Fx(a, 24, 6), O.Fx(z, 24, 6), None, "compute_best")
            assert got.exp == ref.exp, (k, delta, got.exp, ref.exp)
            assert np.array_equal(got.numpy(), ref.data)


# ------------------------------------------------------------------------------------------
# golden fixtures, fallbacks, hooks
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_a", "tiny_b_bnscale", "ndns05_short"])
def test_golden_fixtures_on_gpu(name):
    from sparsernns_amd.engine import Engine
    from sparsernns_amd.fxparray import FxpArray
    from tests.test_cpu_suite import load_golden

    md, meta, export, x, y, inter = load_golden(name)
    eng = Engine(export)
    got, tr = eng.forward(FxpArray(x, meta["x_bits"], meta["x_exp"]), traces=True)
    assert (got.bits, got.exp) == (meta["y_bits"], meta["y_exp"])
    assert np.array_equal(got.numpy(), y)
    names = dict(xs_re="mixer.xs_re", Bu_im="mixer.Bu_im", ys="mixer.ys", residadd="residadd")
    for i in range(eng.n_layers):
        for gk, ok in names.items():
            key = f"layers_{i}.{ok}"
            if key in inter:
                assert np.array_equal(tr[i][gk].cpu().numpy(), inter[key]), key


def test_state_overflow_takes_the_exact_fallback():
    """States beyond the fast recurrence kernel's exactness bound: the range check must fire and the
    32-bit kernels must reproduce the oracle (the reference never clips the state, fxpmodel.py:147-172)."""
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5))
    model = build_regression_model(md, qc, dims["n_layers"])
    fx = _input(qc, dims, 2, 512, seed=9, scale=6.0)  # calibrated at scale 1
    ref, _, _, rtr = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp, trace=True)
    assert max(int(np.abs(t["xs_re"]).max()) for t in rtr) > 32767, "the case must overflow 16 bits to mean anything"
    eng = model.engine()
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    fxa = FxpArray(fx.data, fx.bits, fx.exp)
    # self-contained forward: the gated exact kernels are enqueued with it and fire on the device
    y = eng.forward(fxa, check_status=False)
    assert np.array_equal(y.numpy(), ref)
    assert int(eng.status[0].item()) & _lib.ST_WIDE_STATE and not int(eng.status[0].item()) & _lib.ST_REDO
    # optimistic forward (the default of Engine.forward): ST_REDO comes back, the exact kernels run in a second call
    import torch
    y2 = torch.empty_like(y.data)
    eng.enqueue(fxa.data, fx.bits, fx.exp, y2, 2, 512, flags=_lib.FWD_DEFER_REDO)
    assert int(eng.status[0].item()) & _lib.ST_REDO
    eng.enqueue(fxa.data, fx.bits, fx.exp, y2, 2, 512, flags=_lib.FWD_EXACT)
    assert not int(eng.status[0].item()) & _lib.ST_REDO
    assert np.array_equal(y2.cpu().numpy(), ref)
    assert np.array_equal(eng.forward(fxa).numpy(), ref)
    # and the all-generic engine agrees as well
    gen = build_regression_model(md, qc, dims["n_layers"], engine_flags=_lib.MODEL_FORCE_GENERIC)
    assert _lib.lib.s5fxp_model_is_fast(gen.engine()._h) == 0
    assert np.array_equal(gen(FxpArray(fx.data, fx.bits, fx.exp)).numpy(), ref)


def test_unclipped_input_is_rerun_on_the_generic_kernels():
    """An FxpArray may hold data beyond its nominal bits (the reference never checks): the MFMA encoder
    flags it and the model re-runs on the 32-bit kernels."""
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5))
    model = build_regression_model(md, qc, dims["n_layers"])
    fx = _input(qc, dims, 1, 64, seed=2)
    data = fx.data.copy()
    data[0, 5, 7] = 70000
    data[0, 40, 200] = -(1 << 25)
    ref, _, _, _ = cref.CModel(model.export()).forward(data, fx.bits, fx.exp)
    y = model(FxpArray(data, fx.bits, fx.exp))
    assert np.array_equal(y.numpy(), ref)


def test_exponent_hook_is_called_per_compute_best_op():
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5))
    model = build_regression_model(md, qc, dims["n_layers"])
    fx = _input(qc, dims, 2, 64, seed=3)
    ref = model(FxpArray(fx.data, fx.bits, fx.exp)).numpy()
    calls = []

    def hook(t):
        assert t.dtype.is_floating_point and t.is_cuda
        calls.append(int(t.numel()))

    y = model.engine().forward(FxpArray(fx.data, fx.bits, fx.exp), allreduce=hook)
    assert np.array_equal(y.numpy(), ref)
    # per layer: the per-channel extremes the BatchNorm exponents are derived from (2H floats), then the
    # three maxima of the residual add
    assert calls == [2 * dims["H"], 3] * dims["n_layers"]


def test_inflight_runner_matches_oracle_per_batch():
    """Several different batches kept in flight on separate streams / lanes of one engine: every output must be
    the oracle's for ITS batch (no cross-talk between lanes), including a batch that needs the exact re-run."""
    import torch
    from sparsernns_amd.engine import InflightRunner
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5))
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    cm = cref.CModel(model.export())
    B, L = 2, 256
    runner = InflightRunner(eng, depth=3)
    jobs = []
    for i in range(7):
        fx = _input(qc, dims, B, L, seed=40 + i, scale=6.0 if i == 4 else 1.0)  # batch 4 overflows the fast range
        x = torch.from_numpy(fx.data).cuda()
        y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        runner.submit(x, fx.bits, fx.exp, y, B, L)
        jobs.append((fx, y))
    runner.drain()
    for i, (fx, y) in enumerate(jobs):
        ref, _, _, _ = cm.forward(fx.data, fx.bits, fx.exp)
        assert np.array_equal(y.cpu().numpy(), ref), f"batch {i}"


def test_fxprun_cli_validate_verify_export_reload(tmp_path):
    """The command line end to end: synthetic model, verification (op-by-op == fused), export, reload of the
    exported integer model, same outputs."""
    from sparsernns_amd import fxprun

    pre, o1, o2 = str(tmp_path / "m"), str(tmp_path / "y1.npy"), str(tmp_path / "y2.npy")
    common = ["--seq_len", "128", "--bsz", "2", "--seed", "5"]
    assert fxprun.main(["--synthetic", "--verify", "--export", pre, "--outputs", o1, "--steps", "3", "--inflight", "2"] + common) == 0
    assert fxprun.main(["--model", pre + ".npz", "--meta", pre + ".json", "--outputs", o2, "--steps", "1"] + common) == 0
    assert np.array_equal(np.load(o1), np.load(o2))


def test_denoise_pipeline_on_device_uses_the_exact_model():
    """fxprun.py:63-78 on the device: STFT -> fixed-point model -> mask -> iSTFT.  The model's part must be the
    oracle's output for the integer input the pipeline built; the rest is float tensor code checked against scipy in
    the CPU suite."""
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5))
    model = build_regression_model(md, qc, dims["n_layers"])
    g = torch.Generator().manual_seed(5)
    noisy = (0.02 * torch.randn(2, 128 * 63, generator=g)).cuda()  # 64 STFT frames
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    cleaned, cleaned_mag, mag = audio.denoise(model, ib, ie, noisy)
    assert cleaned.shape == noisy.shape and torch.isfinite(cleaned).all()
    x = (mag - audio.STFT_MAG_MEAN).transpose(-1, -2).contiguous().cpu().numpy()
    fx = O.from_fp(x, ib, ie, True, O.FLOOR)
    ref, rb, re_, _ = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp)
    mask = torch.from_numpy(ref.astype(np.float32) / (1 << re_)).transpose(-1, -2).cuda()
    assert torch.equal(cleaned_mag, mag * (1.0 + mask))
    assert torch.isfinite(audio.si_snr(noisy, cleaned)).all()


def test_csr_dense_is_bit_identical_to_the_dense_op():
    """s5fxp_dense_csr on pruned kernels (90 % zeros, an all-zero channel, 32-bit products that wrap) against
    s5fxp_dense on the zero-filled kernel and against the NumPy oracle."""
    import torch
    from sparsernns_amd.fxparray import CsrWeight, FxpArray, fxp_matmul, fxp_matmul_csr

    rng = np.random.default_rng(17)
    for (N, K, M, wmax, xmax) in ((130, 257, 96, 127, 32767), (64, 96, 257, 127, 32767), (70, 33, 5, 2 ** 20, 2 ** 20)):
        w = rng.integers(-wmax, wmax + 1, size=(K, M)).astype(np.int32)
        w[rng.random((K, M)) < 0.9] = 0
        w[:, M // 2] = 0
        x = rng.integers(-xmax, xmax + 1, size=(N, K)).astype(np.int32)
        fx = FxpArray(torch.from_numpy(x).cuda(), 32, 10)
        dense = fxp_matmul(fx, FxpArray(torch.from_numpy(w).cuda(), 32, 7), result_bits=16, result_exp=9)
        csr = CsrWeight(w, 32, 7)
        assert csr.density < 0.15
        sparse = fxp_matmul_csr(fx, csr, result_bits=16, result_exp=9)
        assert (sparse.bits, sparse.exp) == (dense.bits, dense.exp)
        assert torch.equal(sparse.data, dense.data)
        want = O.matmul(O.Fx(x, 32, 10), O.Fx(w, 32, 7), 16, 9)
        assert np.array_equal(sparse.numpy(), want.data)


def test_pruned_model_op_by_op_goes_through_csr_and_force_csr_is_refused():
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5, sparsity=0.9))
    fx = _input(qc, dims, 2, 64, seed=2)
    eager = build_regression_model(md, qc, dims["n_layers"], store_intermediates=True)
    y = eager(FxpArray(fx.data, fx.bits, fx.exp))
    assert eager.decoder._csr is not None and eager.encoder.encoder._csr is not None  # the CSR op really ran
    ref, _, _, _ = cref.CModel(eager.export()).forward(fx.data, fx.bits, fx.exp)
    assert np.array_equal(y.numpy(), ref)
    with pytest.raises(NotImplementedError):
        build_regression_model(md, qc, dims["n_layers"], engine_flags=_lib.MODEL_FORCE_CSR).engine()


def test_smoke_entry_point_in_a_fresh_interpreter():
    """The driver calls __graft_entry__.smoke() in its own process, where nothing has imported torch yet: the HIP
    library must still end up on torch's HIP runtime (sparsernns_amd/_lib.py imports torch before loading it)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=root, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "[smoke] ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_four_reduction_batchnorm_path_still_exact():
    """The extremes method needs every BatchNorm operand within 16 bits and exponents in [0,15]; outside that the fast
    path falls back to four tensor-wide reductions per layer (k_bn_reduce16 / k_bn_finalize / k_res_finalize /
    k_resid16).  S5FXP_NO_BN_EXT=1 forces that path (read once per process: fresh interpreter)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import numpy as np, torch\n"
        "from oracle import cref, fxp_oracle as O\n"
        "from sparsernns_amd import synth\n"
        "from sparsernns_amd.fxparray import FxpArray\n"
        "from sparsernns_amd.fxpmodel import build_regression_model\n"
        "md, qc, dims = synth.make_model(0.5, bn_scale_bias=True)\n"
        "model = build_regression_model(md, qc, dims['n_layers'])\n"
        "x = synth.make_input(2, 200, dims['d_in'], seed=4)\n"
        "fx = O.from_fp(x, qc['encoder']['inp_bits'], qc['encoder']['inp_exp'], True, O.FLOOR)\n"
        "y = model.engine().forward(FxpArray(fx.data, fx.bits, fx.exp))\n"
        "ref, _, _, _ = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp)\n"
        "assert np.array_equal(y.numpy(), ref)\n"
        "y2 = model.engine().forward(FxpArray(fx.data, fx.bits, fx.exp), check_status=False)\n"
        "assert np.array_equal(y2.numpy(), ref)\n"
        "print('four-reduction path ok')\n")
    env = dict(os.environ, S5FXP_NO_BN_EXT="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "four-reduction path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_forward_is_capturable_in_a_hip_graph():
    """One forward is a fixed sequence of launches on the caller's stream (no allocation, no host round trip, no
    memset in the optimistic mode): it can be captured once and replayed."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5, calib_L=256, state_headroom_bits=1))
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    B, L = 3, 320
    fx = _input(qc, dims, B, L, seed=31)
    xd = torch.from_numpy(fx.data).cuda()
    y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.enqueue(xd, fx.bits, fx.exp, y, B, L, flags=_lib.FWD_DEFER_REDO)  # allocates the workspace, sets attributes
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            eng.enqueue(xd, fx.bits, fx.exp, y, B, L, flags=_lib.FWD_DEFER_REDO)
    ref, _, _, _ = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy(), ref)
        assert not int(eng.status[0].item()) & _lib.ST_REDO


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b_bnscale", "ndns05_short"])
def test_fxprun_cli_golden_check(name):
    """--check-golden on the committed fixtures (the same format tools/reference_pickles_to_npz.py writes from the
    reference's own --export files)."""
    import os
    from sparsernns_amd import fxprun

    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert fxprun.main(["--model", os.path.join(g, name + ".npz"), "--meta", os.path.join(g, name + ".json"),
                        "--check-golden"]) == 0


# ------------------------------------------------------------------------------------------
# BASELINE.json configs at their own shapes (the C oracle finishes these in a few seconds on the box's host cores)
# ------------------------------------------------------------------------------------------
FULL_CONFIGS = {
    # configs[1]: the headline workload, exactly as bench.py builds it (three resident batches, seeds 1000 + lane)
    "configs1_dim05_dense_B32_L4096": (dict(dim_scale=0.5, calib_L=1024, state_headroom_bits=1), 32, 4096, 1.0, 3),
    # configs[2]: 90 % magnitude-pruned weights (zeros stored densely, as the reference keeps them)
    "configs2_dim05_sparse_B32_L4096": (dict(dim_scale=0.5, sparsity=0.9, calib_L=1024, state_headroom_bits=2), 32, 4096, 1.0, 1),
    # configs[3]: one GPU's share of the 512-sequence batch (512 / 8 ranks)
    "configs3_dim10_sparse_B64_L4096": (dict(dim_scale=1.0, sparsity=0.9, calib_L=1024, state_headroom_bits=2), 64, 4096, 1.0, 1),
    # configs[4]: 4-bit weights, 8-bit activations, calibrated BatchNorm statistics
    "configs4_dim10_w4a8_B32_L4096": (dict(dim_scale=1.0, quantization="w4a8", input_scale=300.0, calib_L=256), 32, 4096, 300.0, 1),
}


@pytest.mark.parametrize("name", list(FULL_CONFIGS))
def test_baseline_configs_at_full_size_match_oracle(name):
    """Every batch a bench lane would hold, through the in-flight runner (bench.py's mode) and through Engine.forward,
    against the C oracle's run of the same batch.  Includes the ring wrap of the recurrence kernel (TB = 1024 blocks)
    and whichever of the optimistic / exact kernels the model's state range selects."""
    import torch
    from sparsernns_amd.engine import InflightRunner
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    cfg, B, L, scale, lanes = FULL_CONFIGS[name]
    md, qc, dims = _make(cfg)
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    cm = cref.CModel(model.export())
    runner = InflightRunner(eng, depth=lanes)
    jobs = []
    for lane in range(lanes):
        fx = _input(qc, dims, B, L, seed=1000 + lane, scale=scale)
        x = torch.from_numpy(fx.data).cuda()
        y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        runner.submit(x, fx.bits, fx.exp, y, B, L)
        jobs.append((fx, x, y))
    runner.drain()
    for lane, (fx, x, y) in enumerate(jobs):
        ref, rb, re_, _ = cm.forward(fx.data, fx.bits, fx.exp)
        got = y.cpu().numpy()
        assert np.array_equal(got, ref), f"lane {lane}: {np.count_nonzero(got != ref)} of {ref.size} outputs differ"
    fx, x, _ = jobs[0]
    y1 = eng.forward(FxpArray(x, fx.bits, fx.exp))
    assert (y1.bits, y1.exp) == (rb, re_) and np.array_equal(y1.numpy(), cm.forward(fx.data, fx.bits, fx.exp)[0])


def test_grouped_launch_sets_at_full_size_match_oracle():
    """bench.py's default mode: launch sets of several reference batches (here 4 x 32 x 4096 per set, two sets in flight),
    every batch compared with the C oracle's run of that batch alone."""
    import torch
    from sparsernns_amd.engine import InflightRunner
    from sparsernns_amd.fxpmodel import build_regression_model

    cfg, B, L, scale, _ = FULL_CONFIGS["configs1_dim05_dense_B32_L4096"]
    md, qc, dims = _make(cfg)
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    cm = cref.CModel(model.export())
    G, sets = 4, 2
    runner = InflightRunner(eng, depth=sets)
    jobs = []
    for k in range(sets):
        parts = [_input(qc, dims, B, L, seed=2000 + 10 * k + g, scale=scale) for g in range(G)]
        x = torch.from_numpy(np.concatenate([p.data for p in parts])).cuda()
        y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        runner.submit(x, parts[0].bits, parts[0].exp, y, B, L, groups=G)
        jobs.append((parts, y))
    runner.drain()
    for k, (parts, y) in enumerate(jobs):
        got = y.cpu().numpy()
        for g, p in enumerate(parts):
            ref, _, _, _ = cm.forward(p.data, p.bits, p.exp)
            assert np.array_equal(got[g * B:(g + 1) * B], ref), f"set {k} group {g}"


@pytest.mark.parametrize("B,L", [(1, 16388), (3, 8196), (5, 132)])
def test_long_and_ragged_sequences_on_every_rung(B, L):
    """Sequence lengths that are not multiples of the recurrence kernels' 128-step buffers or 32-block rings (the streams
    are padded, the tail blocks must not leak into real frames), four times the bench length, odd batch sizes -- on the
    pair rung, on the quad16 rung (S5FXP_FWD_NO_PAIR) and on the exact kernels."""
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5, calib_L=256, state_headroom_bits=1))
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    cm = cref.CModel(model.export())
    fx = _input(qc, dims, B, L, seed=77)
    ref = cm.forward(fx.data, fx.bits, fx.exp)[0]
    import torch
    x = torch.from_numpy(fx.data).cuda()
    for flags in (_lib.FWD_DEFER_REDO, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, _lib.FWD_EXACT, 0):
        y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        eng.enqueue(x, fx.bits, fx.exp, y, B, L, flags=flags)
        torch.cuda.synchronize()
        assert not (int(eng.status[0].item()) & _lib.ST_REDO), f"flags {flags}: the calibrated model should stay in range"
        assert np.array_equal(y.cpu().numpy(), ref), f"flags {flags}"


def test_w4a8_tracks_w8a16_within_the_stated_tolerance():
    """BASELINE configs[4]: "tolerance-checked vs w8a16".  The same float model and input, quantised with both recipes,
    both run on the GPU (each bit-exact against its own oracle run: the test above and this one), outputs decoded to
    float.  The bound is loose because the model is random-init and un-trained for 4-bit weights (no QAT): what it pins
    is that the narrow path computes the same function at its own precision -- correlated, same scale -- not an accuracy
    claim.  DESIGN.md section 6 states the same numbers."""
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    outs, enc = {}, {}
    for q in ("w8a16", "w4a8"):
        md, qc, dims = _make(dict(dim_scale=1.0, quantization=q, input_scale=300.0, calib_L=256))
        model = build_regression_model(md, qc, dims["n_layers"])
        fx = _input(qc, dims, 4, 512, seed=11, scale=300.0)
        y = model(FxpArray(fx.data, fx.bits, fx.exp))
        ref, _, re_, _ = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp)
        assert np.array_equal(y.numpy(), ref), q
        outs[q] = ref.astype(np.float64) / (1 << re_)
        inter = {}
        O.RegressionModel(md, qc, dims["n_layers"])(fx, inter)
        e = O.flatten_intermediates(inter)["encoder_output"]
        enc[q] = (e.data.astype(np.float64) / 2.0 ** e.exp, qc["encoder"], np.asarray(md["encoder"]["encoder"]["kernel"], dtype=np.float64))
    d = outs["w4a8"] - outs["w8a16"]
    rel = np.linalg.norm(d) / np.linalg.norm(outs["w8a16"])
    corr = np.corrcoef(outs["w4a8"].ravel(), outs["w8a16"].ravel())[0, 1]
    assert rel < W4A8_REL_L2_BOUND and corr > W4A8_CORR_BOUND, (rel, corr)
    # Where the tolerance CAN be derived -- one dense layer, no accumulated nonlinearity -- it is: rounding a weight to a step of
    # 2^-w_exp adds uniform noise of variance step^2 / 12, so the encoder outputs of the two recipes must differ by a relative L2
    # error of (2^-w_exp / sqrt 12) / rms(kernel), plus the (small) input and output steps.  A wrong exponent, a dropped byte
    # plane or a saturating weight would land far outside [0.5, 1.5] x that figure (measured 0.161 against 0.147).
    a4, q4, kern = enc["w4a8"]
    a8 = enc["w8a16"][0]
    x_rms = float(np.sqrt(np.mean((fx.data.astype(np.float64) / 2.0 ** fx.exp) ** 2)))
    pred = np.sqrt((2.0 ** -q4["w_exp"] / np.sqrt(12) / np.sqrt(np.mean(kern ** 2))) ** 2 +
                   (2.0 ** -q4["out_exp"] / np.sqrt(12) / np.sqrt(np.mean(a8 ** 2))) ** 2 + (2.0 ** -q4["inp_exp"] / np.sqrt(12) / x_rms) ** 2)
    rel_enc = np.linalg.norm(a4 - a8) / np.linalg.norm(a8)
    assert 0.5 * pred < rel_enc < 1.5 * pred, (rel_enc, pred)


# measured (deterministic: both outputs are bit-exact with the oracle): rel L2 0.649, correlation 0.797
W4A8_REL_L2_BOUND, W4A8_CORR_BOUND = 0.8, 0.7


# ------------------------------------------------------------------------------------------
# mode A for real: two ranks of the ENGINE, global exponents, against ONE oracle run over the whole batch
# ------------------------------------------------------------------------------------------
MODE_A_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from oracle import cref, fxp_oracle as O
from sparsernns_amd import _lib, synth
from sparsernns_amd.dist import shard_bounds, make_exponent_allreduce
from sparsernns_amd.fxparray import FxpArray
from sparsernns_amd.fxpmodel import build_regression_model
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)                                   # both ranks share the one GPU of the box
dist.init_process_group("gloo", rank=rank, world_size=world)
md, qc, dims = synth.make_model(0.5, calib_L=256)
model = build_regression_model(md, qc, dims["n_layers"])
cm = cref.CModel(model.export())
hook = make_exponent_allreduce(via_host=True)              # gloo: stage the device maxima through the host
B, L = 4, 512
ok = True
for case, scales in (("plain", [1.0] * B), ("one_rank_overflows", [1.0, 1.0, 6.0, 1.0])):
    x = np.concatenate([synth.make_input(1, L, dims["d_in"], seed=70 + i, scale=s) for i, s in enumerate(scales)])
    fx = O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    full, fb, fe, tr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)   # ONE oracle run over the concatenated batch
    lo, hi = shard_bounds(B, world, rank)
    eng = model.engine()
    calls = []
    def counted(t):
        calls.append(int(t.numel()))
        hook(t)
    y = eng.forward(FxpArray(fx.data[lo:hi], fx.bits, fx.exp), allreduce=counted)
    st = int(eng.status[0].item())
    mine_overflows = bool(max(int(np.abs(t["xs_re"][lo:hi]).max()) for t in tr) > 32767)
    parts = [torch.empty((hi - lo, L, dims["d_out"]), dtype=torch.int32) for _ in range(world)]
    dist.all_gather(parts, y.data.cpu())
    got = torch.cat(parts).numpy()
    same = bool(np.array_equal(got, full)) and (y.bits, y.exp) == (fb, fe)
    local_only = cm.forward(fx.data[lo:hi], fx.bits, fx.exp)[0]          # mode B on the same shard
    coupled = bool(not np.array_equal(local_only, full[lo:hi]))
    wide = bool(st & _lib.ST_WIDE_STATE)
    print(f"RANK{rank} {case}: modeA={same} exchanges={len(calls)} wide={wide} expect_wide={mine_overflows} coupled={coupled}", flush=True)
    ok = ok and same and wide == mine_overflows and calls == [2 * dims["H"], 3] * dims["n_layers"]
print(f"RANK{rank} ALL_OK={ok}", flush=True)
dist.destroy_process_group()
'''


def _free_port() -> int:
    """A rendezvous port nobody holds right now (a fixed one collides when two test runs share a host)."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_engine_ranks_with_global_exponents_equal_one_oracle_run(tmp_path):
    """SURVEY.md 8(e) mode A on the product: two fresh processes (gloo, both on GPU 0), each running Engine.forward
    on its half of the batch with the exponent all-reduce hook; the gathered output must equal ONE oracle run over the
    concatenated batch.  Second case: only rank 1 holds a sequence whose states leave the 16-bit range, so only that
    rank's layers take the exact re-run (LayerDyn::redo, k_select_maxima) while both must still agree on every
    exponent."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "mode_a_worker.py"
    script.write_text(MODE_A_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2", OMP_NUM_THREADS="8")
    procs = [subprocess.Popen([sys.executable, str(script), root], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=900)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o[-4000:]
        assert f"RANK{r} ALL_OK=True" in o, o[-4000:]
    # the second case must really be asymmetric: rank 1 re-ran, rank 0 did not
    assert "RANK0 one_rank_overflows: modeA=True" in outs[0] and "wide=False" in outs[0].split("one_rank_overflows")[1].splitlines()[0]
    assert "wide=True" in outs[1].split("one_rank_overflows")[1].splitlines()[0]


def test_bench_starts_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher: the parent starts two fresh ranks before it touches the GPU and relays
    rank 0's JSON line (here both ranks share the box's one GPU over gloo -- S5FXP_BENCH_BACKEND, a rehearsal aid; the
    driver's runs use RCCL).  Also the sharded configs[3] form with global exponents, and the WORLD_SIZE / --gpus check."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["S5FXP_BENCH_BACKEND"] = "gloo"
    small = ["--seq-len", "256", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-scan-sweep"]
    # two ranks, then four (the launch path of the driver's 8-rank run beyond N = 2: shard_bounds with a remainder-free
    # split, the gather of four shards, every rank's own clock in the line); config 3 = ONE batch sharded, mode A
    for n, extra, n_bl in ((2, ["--batch", "2"], 2 * 2 * 256), (2, ["--config", "3", "--batch", "4", "--global-exponents"], 4 * 256),
                           (4, ["--batch", "2"], 4 * 2 * 256), (4, ["--config", "3", "--batch", "8", "--global-exponents"], 8 * 256)):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n)] + small + extra, cwd=root, env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["n_gpus"] == n and out["steps"] == 2 and out["output_gather_ms"] is not None
        assert abs(out["value"] * out["ms_per_step"] * 1e-3 - n_bl) < 1e-3 * n_bl  # value = all ranks' frames / time
        assert out["roofline"]["frac"] > 0 and out["scaling"] == ("strong" if "--config" in extra else "weak")
        rv = out["rank_values"]
        assert len(rv["per_rank"]) == n and rv["min"] <= rv["max"] and abs(rv["min"] * n - out["value"]) < 1e-6 * out["value"]
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"] + small, cwd=root,
                         env=dict(env, WORLD_SIZE="3", RANK="0"), capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "WORLD_SIZE=3" in (bad.stdout + bad.stderr)


def test_bench_dump_outputs_is_the_last_timed_step(tmp_path):
    """`bench.py --dump-outputs DIR` writes the output of the last timed step, as floats, equal to the C oracle's run of
    that step's batch: step K - 1 is group (K - 1) % G of the last launch set, on lane (sets - 1) % inflight, whose
    batches are pool[(lane + g) % max(G, inflight)] of the seeded inputs.  The small case dumps the whole output; the
    larger one exceeds the size cap and dumps a fixed, seeded sample of frames."""
    import json
    import os
    import subprocess
    import sys

    from sparsernns_amd.fxparray import RoundingMode, fxp_from_fp
    from sparsernns_amd.fxpmodel import build_regression_model

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    md, qc, dims = _make(dict(dim_scale=0.5, quantization="w8a16", sparsity=0.0, calib_L=1024, state_headroom_bits=1,
                              input_scale=1.0))   # bench.py's configs[1] model
    cm = cref.CModel(build_regression_model(md, qc, dims["n_layers"]).export())
    for B, L, steps, G, depth in ((2, 256, 5, 2, 3), (32, 1024, 11, 8, 3)):
        out = tmp_path / f"dump_{B}x{L}"
        args = ["--batch", str(B), "--seq-len", str(L), "--steps", str(steps), "--warmup", "1", "--groups", str(G),
                "--inflight", str(depth), "--no-cpu-baseline", "--no-scan-sweep", "--dump-outputs", str(out)]
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, cwd=root, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        sets = (steps + G - 1) // G
        lane, g = (sets - 1) % depth, (steps - 1) % G
        x = synth.make_input(B, L, dims["d_in"], seed=1000 + 4096 * ((lane + g) % max(G, depth)), scale=1.0)
        fx = fxp_from_fp(x, bits=qc["encoder"]["inp_bits"], exp=qc["encoder"]["inp_exp"], signed=True, round_mode=RoundingMode.FLOOR)
        ref, _, re_, _ = cm.forward(fx.numpy(), fx.bits, fx.exp)
        want = ref.reshape(B * L, -1).astype(np.float64) / 2.0 ** re_
        files = os.listdir(out)
        assert files == ["y.npy"] and os.path.getsize(out / "y.npy") <= 64 << 20
        got = np.load(out / "y.npy")
        assert got.dtype == np.float64
        if want.nbytes > 48 << 20:
            keep = np.sort(np.random.default_rng(0).choice(B * L, (48 << 20) // want[0].nbytes, replace=False))
            want = want[keep]
        assert got.shape == want.shape and np.array_equal(got, want)


def test_pair_recurrence_kernel_is_selected_and_guarded():
    """The optimistic forward of the NDNS models runs the pair kernel (two lanes per state, Bu folded into the multiply's
    addend: csrc/scan_quad.hpp).  Its exactness bound on |state| is tighter than the quad kernel's; inputs scaled so that
    the states pass it must come back through the exact kernels with the oracle's result, and with S5FXP_NO_PAIR=1 the
    quad kernels must still give the same outputs."""
    import os
    import subprocess
    import sys
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    for ds in (0.5, 1.0):
        md, qc, dims = _make(dict(dim_scale=ds, calib_L=256, state_headroom_bits=1))
        model = build_regression_model(md, qc, dims["n_layers"])
        eng = model.engine()
        assert [_lib.lib.s5fxp_model_recurrence_kernel(eng._h, i) for i in range(3)] == [4, 4, 4]
        cm = cref.CModel(model.export())
        seen = set()
        for scale in (1.0, 2.0, 2.6, 3.2, 4.0):   # from well inside the bound to beyond 16 bits
            fx = _input(qc, dims, 2, 640, seed=int(10 * scale), scale=scale)
            ref, _, _, tr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
            top = max(max(int(np.abs(t["xs_re"]).max()), int(np.abs(t["xs_im"]).max())) for t in tr)
            y = eng.forward(FxpArray(fx.data, fx.bits, fx.exp))
            assert np.array_equal(y.numpy(), ref), (ds, scale, top)
            seen.add(top > 32767)
        assert seen == {False, True}, "the sweep must cover states inside and outside 16 bits"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import numpy as np\n"
            "from oracle import cref, fxp_oracle as O\n"
            "from sparsernns_amd import _lib, synth\n"
            "from sparsernns_amd.fxparray import FxpArray\n"
            "from sparsernns_amd.fxpmodel import build_regression_model\n"
            "md, qc, dims = synth.make_model(0.5, calib_L=256, state_headroom_bits=1)\n"
            "model = build_regression_model(md, qc, dims['n_layers'])\n"
            "eng = model.engine()\n"
            "assert _lib.lib.s5fxp_model_recurrence_kernel(eng._h, 0) == 2\n"
            "x = synth.make_input(2, 640, dims['d_in'], seed=4)\n"
            "fx = O.from_fp(x, qc['encoder']['inp_bits'], qc['encoder']['inp_exp'], True, O.FLOOR)\n"
            "y = eng.forward(FxpArray(fx.data, fx.bits, fx.exp))\n"
            "assert np.array_equal(y.numpy(), cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp)[0])\n"
            "print('quad16 path ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, S5FXP_NO_PAIR="1"))
    assert r.returncode == 0 and "quad16 path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    # the pair kernel's other feeds: the int32 K stream in global memory, and the LDS-fed kernel with 16-block buffers
    code2 = code.replace("== 2", "in (3, 4)").replace("quad16 path ok", "pair variant ok")
    for var, val in (("S5FXP_PAIR_GLOBAL", "1"), ("S5FXP_PAIRL_BLOCKS", "16")):
        r = subprocess.run([sys.executable, "-c", code2], cwd=root, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, **{var: val}))
        assert r.returncode == 0 and "pair variant ok" in r.stdout, var + r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("engine_flags", [0, "generic"])
def test_streaming_chunks_carry_the_state_like_the_oracle(engine_flags):
    """SURVEY.md 8(f)4 / fxpmodel.py:147-172: a sequence fed chunk by chunk with the SSM states carried between calls.
    Per chunk the GPU must give what the oracle gives for that chunk started from the same carry (both oracle halves
    agree on that in the CPU suite), the carry itself must match after every chunk, chunk lengths are ragged, one chunk
    overflows the fast recurrence's range (exact repeat from the untouched carry), and a carry of zeros is the plain
    forward."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5, calib_L=256))
    flags = _lib.MODEL_FORCE_GENERIC if engine_flags == "generic" else 0
    model = build_regression_model(md, qc, dims["n_layers"], engine_flags=flags)
    eng = model.engine()
    cm = cref.CModel(model.export())
    B = 2
    sess = eng.stream(B)
    ref_state = np.zeros((dims["n_layers"], 2, B, dims["P"]), dtype=np.int32)
    # both paths take any chunk length; the fused one down to single frames (real-time use)
    lens = (64, 128, 36, 4, 200, 1, 3, 2, 37, 1) if engine_flags == 0 else (64, 37, 5)
    for i, L in enumerate(lens):
        fx = _input(qc, dims, B, L, seed=300 + i, scale=6.0 if i == 2 else 1.0)
        ref, rb, re_, _ = cm.forward(fx.data, fx.bits, fx.exp, state=ref_state)   # updates ref_state in place
        y = sess.push(FxpArray(fx.data, fx.bits, fx.exp))
        assert (y.bits, y.exp) == (rb, re_)
        assert np.array_equal(y.numpy(), ref), f"chunk {i} (L={L})"
        assert np.array_equal(sess.state.cpu().numpy(), ref_state), f"carry after chunk {i}"
        if engine_flags == 0:
            _ran_fused(eng, dims["n_layers"])
    assert sess.frames == sum(lens) and np.abs(ref_state).max() > 0
    # zero carry == the stateless forward
    fx = _input(qc, dims, B, 64, seed=9)
    y0, st = eng.forward_chunk(FxpArray(fx.data, fx.bits, fx.exp), None)
    assert np.array_equal(y0.numpy(), eng.forward(FxpArray(fx.data, fx.bits, fx.exp)).numpy())
    with pytest.raises(ValueError):
        eng.forward_chunk(FxpArray(fx.data, fx.bits, fx.exp), torch.zeros((1, 2, B, dims["P"]), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("ds", [0.5, 1.0])
def test_layers_run_on_their_live_states_only(ds, monkeypatch):
    """A state whose rows of the 8-bit B_bar are all zero never leaves (0, 0) (include/s5fxp.h s5fxp_model_live_states): when at
    most half of a layer's states are live the fused kernels run the layer on the fewest groups of 32 state slots that hold them.  The status words must say
    so, the output must be the oracle's on every rung, an engine created with S5FXP_NO_COMPACT must give the same bits on
    all P slots, and a forward that carries the states in or out must not compact."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=ds, calib_L=256, state_headroom_bits=1))
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    P, nl = dims["P"], dims["n_layers"]
    ex = model.export()["params"]["encoder"]
    live = [int(((np.asarray(ex[f"layers_{i}"]["mixer"]["B_real"]) != 0).any(axis=1) |
                 (np.asarray(ex[f"layers_{i}"]["mixer"]["B_imag"]) != 0).any(axis=1)).sum()) for i in range(nl)]
    assert [_lib.lib.s5fxp_model_live_states(eng._h, i) for i in range(nl)] == live
    assert all(n <= P // 2 for n in live), live          # the N-DNS recipe: two thirds of the states are dead
    want = [max(32, (n + 31) // 32 * 32) for n in live]  # the fewest groups of 32 slots that hold the live states
    cm = cref.CModel(model.export())
    B, L = 3, 333
    fx = _input(qc, dims, B, L, seed=21)
    ref, _, _, rtr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
    tops = [max(int(np.abs(t["xs_re"]).max()), int(np.abs(t["xs_im"]).max())) for t in rtr]
    bounds = [_lib.lib.s5fxp_model_recurrence_xmax(eng._h, i) for i in range(nl)]   # of the top rung, over the live states
    x = torch.from_numpy(fx.data).cuda()
    slots = lambda e: [int(v) for v in e.lane_status(0).cpu().numpy()[8 + 6:8 + 8 * nl:8]]
    for flags in (_lib.FWD_DEFER_REDO, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, 0, _lib.FWD_EXACT):
        y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        eng.enqueue(x, fx.bits, fx.exp, y, B, L, flags=flags)
        redo = bool(int(eng.check_status()[0]) & _lib.ST_REDO)
        assert slots(eng) == want, (flags, slots(eng), live)
        # the two int16 rungs keep only the live slots (whole state pairs) in their recurrence streams: status word [8 + 8l + 7]
        stream = [int(v) for v in eng.lane_status(0).cpu().numpy()[8 + 7:8 + 8 * nl:8]]
        int16_rung = bool(flags & _lib.FWD_DEFER_REDO)
        assert stream == [min(w, max(2, 2 * ((n + 1) // 2))) if int16_rung else w for n, w in zip(live, want)], (flags, stream)
        if flags == _lib.FWD_DEFER_REDO:   # the top rung asks for a repeat exactly when a live state passes its bound
            assert redo == any(t > b for t, b in zip(tops, bounds)), (tops, bounds)
        else:
            assert not redo, flags
        if not redo:
            assert np.array_equal(y.cpu().numpy(), ref), flags
    # with the carry in play every state slot is live as far as the kernels know
    y, st = eng.forward_chunk(FxpArray(fx.data, fx.bits, fx.exp), None)
    assert slots(eng) == [P] * nl and np.array_equal(y.numpy(), ref)
    # the same model without the compaction
    monkeypatch.setenv("S5FXP_NO_COMPACT", "1")
    eng2 = build_regression_model(md, qc, dims["n_layers"]).engine()
    monkeypatch.delenv("S5FXP_NO_COMPACT")
    y2 = eng2.forward(FxpArray(fx.data, fx.bits, fx.exp))
    assert slots(eng2) == [P] * nl and np.array_equal(y2.numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("ds,B,L", [(0.5, 3, 333), (0.5, 2, 64), (1.0, 2, 129), (0.5, 33, 1)])
def test_decoder_carries_the_last_residual_pass(ds, B, L, monkeypatch):
    """The fused path's decoder forms the last layer's h = relu(z + skip) itself (proj_p.hpp k_dec_p<.., RESID>) and derives
    the residual exponent in its own prologue: the output and the reported ``residadd`` exponents must be the oracle's, on full
    tiles, a ragged last tile (N % 64 != 0) and a single frame, and an engine created with S5FXP_NO_DEC_RESID (the residual
    pass as its own launch) must give the same bits."""
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=ds, calib_L=256, state_headroom_bits=1))
    model = build_regression_model(md, qc, dims["n_layers"])
    cm = cref.CModel(model.export())
    fx = _input(qc, dims, B, L, seed=5)
    ref, rb, re_, rtr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
    eng = model.engine()
    y = eng.forward(FxpArray(fx.data, fx.bits, fx.exp))
    _ran_fused(eng, dims["n_layers"])
    assert (y.bits, y.exp) == (rb, re_) and np.array_equal(y.numpy(), ref)
    got = [e["residadd"] for e in eng.layer_exponents()]
    assert got == [t["residadd_exp"] for t in rtr]
    monkeypatch.setenv("S5FXP_NO_DEC_RESID", "1")
    eng2 = build_regression_model(md, qc, dims["n_layers"]).engine()
    monkeypatch.delenv("S5FXP_NO_DEC_RESID")
    y2 = eng2.forward(FxpArray(fx.data, fx.bits, fx.exp))
    assert np.array_equal(y2.numpy(), ref)
    assert got == [e["residadd"] for e in eng2.layer_exponents()]


@pytest.mark.parametrize("case", ["tiny_bnsb", "ndns05"])
def test_layer_forward_entry_point_matches_the_oracle_layer_by_layer(case):
    """s5fxp_layer_forward (FxpSequenceLayer.forward, fxpmodel.py:1110-1161): feeding the oracle's
    ``layer_{i-1}_output`` into layer i must reproduce the oracle's residadd / output of that layer and its data-dependent
    exponent, for every layer, with the traced stages equal too."""
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    cfg, B, L, scale = CASES[case]
    md, qc, dims = _make(cfg)
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    fx = _input(qc, dims, B, L, seed=11, scale=scale)
    om = O.RegressionModel(md, qc, dims["n_layers"])
    inter = {}
    om(fx, inter)
    fl = O.flatten_intermediates(inter)
    _, _, _, rtr = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp, trace=True)
    h = fl["encoder_output_relu"]
    for i in range(dims["n_layers"]):
        want = fl[f"layers_{i}.output"]
        got, tr = eng.layer_forward(i, FxpArray(h.data, h.bits, h.exp), traces=True)
        assert (got.bits, got.exp) == (want.bits, want.exp), (i, got.bits, got.exp, want.bits, want.exp)
        assert np.array_equal(got.numpy(), want.data), i
        for k, ck in TRACE_MAP.items():
            assert np.array_equal(tr[k].cpu().numpy(), rtr[i][ck]), (i, k)
        h = want


def test_fxprun_verify_reports_every_stage_against_float_activations(tmp_path, capsys):
    """run_verification's report (sparseRNNs/fxprun.py:553-731, fxpreporter.py) -- every stage the reference
    looks at, fixed point against FLOAT activations, not the repository against itself.  The float side is this package's
    float forward of the same parameters (what the reference's activations_fp.pkl holds), once computed in the run and once
    read back from the npz tree the converter writes."""
    import json
    from sparsernns_amd import fxprun

    common = ["--synthetic", "--seq_len", "256", "--bsz", "2", "--steps", "0", "--verify"]
    assert fxprun.main(common + ["--report", str(tmp_path / "r1"), "--write-activations", str(tmp_path / "a.npz")]) == 0
    out = capsys.readouterr().out
    assert "op-by-op forward == fused forward: True" in out and "verification report: 41 stages" in out
    res = json.load(open(tmp_path / "r1" / "results.json"))["results"]
    names = [r["name"] for r in res]
    assert names[0] == "inputs" and names[-1] == "decoder" and "encoder.layers_1.mixer.xt (imag)" in names
    assert "encoder.encoder (post-relu)" in names and "encoder.layers_2.mixer.residadd" in names
    by = {r["name"]: r for r in res}
    assert by["inputs"]["abs_error_max"] <= 2.0 ** -15          # FLOOR to 16 bits at exponent 15 (fxprun.py:69-75)
    for r in res:
        assert all(np.isfinite(r[k]) for k in ("abs_error_mean", "abs_error_max", "rel_error_med", "xhat_absmax")), r
    # what 16-bit activations and 8-bit weights leave of the float model where nothing else interferes: the encoder and the
    # LUT sigmoid track it to a percent.  (Deeper stages of this random-init model do not -- the report's job is to show
    # where: 8-bit B_bar with one shared exponent rounds most of its rows to zero, profiles/r03_verify_report.md.)
    assert by["encoder.encoder (post-relu)"]["rel_error_med"] < 0.02 and by["encoder.layers_0.mixer.out2_sigmoid"]["rel_error_med"] < 0.05
    assert by["encoder.layers_1.input"]["abs_error_mean"] == by["encoder.layers_0.mixer.output"]["abs_error_mean"]
    assert (tmp_path / "r1" / "report.md").read_text().count("\n| ") >= 41
    # the same report from the activations file
    assert fxprun.main(common + ["--activations_fname", str(tmp_path / "a.npz"), "--report", str(tmp_path / "r2")]) == 0
    res2 = json.load(open(tmp_path / "r2" / "results.json"))["results"]
    assert [r["abs_error_mean"] for r in res2] == [r["abs_error_mean"] for r in res]


def test_fxprun_cli_from_calibration_trees(tmp_path):
    """--params / --stats: the reference's calibration output as npz trees -> fxputils.derive -> model -> forward.  The
    outputs must be those of the model built directly from the same float parameters and statistics, shared and
    per-layer exponents."""
    from sparsernns_amd import fxprun, fxputils
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    dims = synth.ndns_dims(0.5)
    md = synth.make_float_params(dims, 1919)
    stats = {}
    synth.float_forward(md, synth.make_input(2, 256, dims["d_in"], seed=1920), dims["n_layers"], calibrate_bn=True, stats=stats)
    qc = synth.derive_qconfig(md, stats, dims["n_layers"])
    params, st = synth.reference_trees(md, stats, dims["n_layers"])
    fxputils.save_tree_npz(tmp_path / "p.npz", params)
    fxputils.save_tree_npz(tmp_path / "s.npz", st)
    x = synth.make_input(2, 128, dims["d_in"], seed=8)
    np.save(tmp_path / "x.npy", x)
    common = ["--params", str(tmp_path / "p.npz"), "--stats", str(tmp_path / "s.npz"), "--inputs", str(tmp_path / "x.npy"), "--steps", "0"]
    assert fxprun.main(common + ["--outputs", str(tmp_path / "y.npy")]) == 0
    fx = O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    want = build_regression_model(md, qc, dims["n_layers"])(FxpArray(fx.data, fx.bits, fx.exp))
    assert np.array_equal(np.load(tmp_path / "y.npy"), want.to_float().cpu().numpy())
    assert fxprun.main(common + ["--separate_exponents", "--outputs", str(tmp_path / "y2.npy")]) == 0
    md2, qc2 = fxputils.derive(params, st, "w8a16", separate_exponents=True)
    ref = cref.CModel(build_regression_model(md2, qc2, dims["n_layers"]).export()).forward(fx.data, fx.bits, fx.exp)
    assert np.array_equal(np.load(tmp_path / "y2.npy"), ref[0].astype(np.float32) / (1 << ref[2]))


def test_recurrence_ladder_pair_quad_exact():
    """Optimistic forwards climb a ladder when the range check fires: pair kernel (bound tightened by the folded Bu) ->
    quad kernel with int16 streams (the full 16 bits) -> exact 32-bit kernels.  A pruned model whose states sit between the
    first two bounds must be served by the middle rung (no exact kernels), with the oracle's output, and after two such
    forwards the engine starts there."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import InflightRunner
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = _make(dict(dim_scale=0.5, sparsity=0.9, calib_L=1024, state_headroom_bits=2))
    model = build_regression_model(md, qc, dims["n_layers"])
    eng = model.engine()
    cm = cref.CModel(model.export())
    bounds = [_lib.lib.s5fxp_model_recurrence_xmax(eng._h, i) for i in range(3)]
    assert all(16384 <= b < 32766 for b in bounds)  # this model's |Im lambda| is close to one: the folded Bu costs the pair kernel range
    for scale in (1.5, 1.7, 1.9, 2.1, 2.3, 2.6, 3.0):   # a sequence with a layer whose largest state lies between the two rungs' bounds
        fx = _input(qc, dims, 2, 2048, seed=1000, scale=scale)
        ref, _, _, tr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
        tops = [max(int(np.abs(t["xs_re"]).max()), int(np.abs(t["xs_im"]).max())) for t in tr]
        top = max(tops)
        if top <= 32766 and any(t > b for t, b in zip(tops, bounds)):
            break
    x = torch.from_numpy(fx.data).cuda()
    y = torch.empty((2, 2048, dims["d_out"]), dtype=torch.int32, device="cuda")
    eng.enqueue(x, fx.bits, fx.exp, y, 2, 2048, flags=_lib.FWD_DEFER_REDO)
    pair_redo = bool(int(eng.status[0].item()) & _lib.ST_REDO)
    eng.enqueue(x, fx.bits, fx.exp, y, 2, 2048, flags=_lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR)
    quad_redo = bool(int(eng.status[0].item()) & _lib.ST_REDO)
    assert top <= 32766 and pair_redo and not quad_redo, (top, pair_redo, quad_redo)  # the case sits between the two bounds
    assert np.array_equal(y.cpu().numpy(), ref)
    for k in range(2):
        assert eng.level == 0
        assert np.array_equal(eng.forward(FxpArray(x, fx.bits, fx.exp)).numpy(), ref)
    assert eng.level == 1  # two failures of the first rung: start on the second from now on
    runner = InflightRunner(eng, depth=2)
    ys = [torch.empty_like(y) for _ in range(3)]
    for yy in ys:
        runner.submit(x, fx.bits, fx.exp, yy, 2, 2048)
    runner.drain()
    assert all(np.array_equal(yy.cpu().numpy(), ref) for yy in ys)
