"""The HIP kernels against what the REFERENCE's own integer code recorded (tests/golden/ref_*, written by
tests/golden/make_reference_golden.py from the reference run under oracle/jaxlike.py).  Bit-exact throughout.  Reads the
fixtures only: no reference checkout, and no expected value comes from the CPU oracle.

The stream step is not compared: each chunk is its own compute_best batch there, a mode the reference does not have.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import reference_fixtures as RF

# Engine.forward's trace planes (sparsernns_amd/_lib.py TRACE_FIELDS) under the reference's sow keys
ENGINE_TRACE = {"pre_s5": "pre_s5", "Bu_re": "mixer.Bu_elements.real", "Bu_im": "mixer.Bu_elements.imag", "xs_re": "mixer.xs.real",
                "xs_im": "mixer.xs.imag", "ys": "mixer.ys", "out2": "out2.__call__", "out2_sigmoid": "out2_sigmoid",
                "post_GLU": "post_GLU", "residadd": "residadd"}


# ---------------------------------------------------------------------------------------------------------------------
# op kernels through the C ABI (sparsernns_amd.fxparray / fxpmodel are thin ctypes callers of s5fxp_*)
# ---------------------------------------------------------------------------------------------------------------------
def run_gpu(cfg, ins):
    """One ref_ops case on the device.  None for a case the C ABI has no entry for: a rounding mode other than FLOOR
    outside s5fxp_from_fp, and the complex add / mul, which the model never calls."""
    import torch
    from sparsernns_amd import fxparray as G
    from sparsernns_amd._lib import check, lib
    from sparsernns_amd.fxpmodel import FxpSigmoid, fxp_relu

    op = cfg["op"]
    if op in ("complex_add", "complex_mul") or (op != "from_fp" and cfg.get("mode", "FLOOR") != "FLOOR"):
        return None
    fx = lambda k, c: G.FxpArray(np.ascontiguousarray(ins[k], dtype=np.int32), c[0], c[1])
    one = lambda r: (dict(out=r.numpy()), [[r.bits, r.exp]])
    if op == "from_fp":
        return one(G.fxp_from_fp(ins["x"], cfg["bits"], cfg["exp"], True, G.RoundingMode[cfg["mode"]]))
    if op == "to_float":
        return dict(out=fx("a", cfg["a_cfg"]).to_float().cpu().numpy()), []
    if op == "change_exp":
        return one(G.fxp_change_exp(fx("a", cfg["a_cfg"]), cfg["new_exp"]))
    if op == "change_cfg":
        return one(G.fxp_change_cfg(fx("a", cfg["a_cfg"]), cfg["new_bits"], cfg["new_exp"], True))
    if op in ("add", "sub", "mul"):
        f = dict(add=G.fxp_add, sub=G.fxp_sub, mul=G.fxp_mul)[op]
        return one(f(fx("a", cfg["a_cfg"]), fx("b", cfg["b_cfg"]), result_bits=cfg["result_bits"], result_exp=cfg["result_exp"]))
    if op == "matmul":
        a, b = fx("a", cfg["a_cfg"]), fx("b", cfg["b_cfg"])
        dense = G.fxp_matmul(a, b, result_bits=cfg["result_bits"], result_exp=cfg["result_exp"])
        csr = G.fxp_matmul_csr(a, G.CsrWeight(ins["b"], *cfg["b_cfg"]), result_bits=cfg["result_bits"], result_exp=cfg["result_exp"])
        assert (csr.bits, csr.exp) == (dense.bits, dense.exp) and torch.equal(csr.data, dense.data), "s5fxp_dense_csr != s5fxp_dense"
        return one(dense)
    if op == "clip":
        return one(G.fxp_clip(fx("a", cfg["a_cfg"])))
    if op == "relu":
        return one(fxp_relu(fx("a", cfg["a_cfg"])))
    if op == "relu_complex":
        r = fxp_relu(G.ComplexFxpArray(fx("ar", cfg["a_cfg"]), fx("ai", cfg["a_cfg"])))
        return dict(out_re=r.real.numpy(), out_im=r.imag.numpy()), [[r.real.bits, r.real.exp], [r.imag.bits, r.imag.exp]]
    if op == "sigmoid":
        s = FxpSigmoid(x_exp=cfg["x_exp"], y_exp=cfg["y_exp"])
        outs, c = one(s.apply(fx("a", cfg["a_cfg"])))
        outs["lut"] = np.asarray(s.lut)
        return outs, c
    if op == "scan":
        t = lambda k: torch.as_tensor(np.ascontiguousarray(ins[k], dtype=np.int32)).cuda()
        bre, bim, ar, ai = t("bu_re"), t("bu_im"), t("a_re"), t("a_im")
        B, (L, P) = (bre.shape[0] if bre.ndim == 3 else 1), bre.shape[-2:]
        xr, xi = torch.empty_like(bre), torch.empty_like(bim)
        check(lib.s5fxp_scan(bre.data_ptr(), bim.data_ptr(), ar.data_ptr(), ai.data_ptr(), xr.data_ptr(), xi.data_ptr(), B, L, P,
                             cfg["a_exp"], cfg["a_exp"], cfg["bu_exp"], cfg["bu_exp"], cfg["x_exp"], cfg["x_exp"], 0,
                             torch.cuda.current_stream().cuda_stream), "s5fxp_scan")
        return dict(out_re=xr.cpu().numpy(), out_im=xi.cpu().numpy()), []
    raise KeyError(op)


def test_op_kernels_reproduce_the_reference_op_table():
    ran, skipped = {}, 0
    for i, cfg, ins, want in RF.op_cases():
        res = run_gpu(cfg, ins)
        if res is None:
            skipped += 1
            continue
        RF.assert_case_equal(f"ref_ops case {i} {cfg}", res[0], res[1], want, cfg["out_cfg"])
        ran[cfg["op"]] = ran.get(cfg["op"], 0) + 1
    # every entry of the C ABI the table reaches really ran: s5fxp_from_fp / to_float / change_cfg / add / mul / add_cb /
    # mul_cb / dense / dense_csr / relu / sigmoid / scan
    assert set(ran) == {"from_fp", "to_float", "change_exp", "change_cfg", "add", "sub", "mul", "matmul", "clip", "relu",
                        "relu_complex", "sigmoid", "scan"}, ran
    assert ran["from_fp"] >= 12 and ran["sigmoid"] == 4 and ran["scan"] == 3 and ran["matmul"] >= 3
    best = [c for _, c, _, _ in RF.op_cases() if c.get("result_exp") == "compute_best"]
    assert {c["op"] for c in best} >= {"add", "mul"}
    print(f"\n[reference gpu] {sum(ran.values())} op cases bit-exact, {skipped} without a C ABI entry (non-FLOOR modes, complex add / mul)")


# ---------------------------------------------------------------------------------------------------------------------
# model kernels
# ---------------------------------------------------------------------------------------------------------------------
def _dummy_modeldict(export):
    """Float parameters of the right shapes for a fixture that records none; every integer they produce is replaced."""
    P = export["params"]
    z = lambda *s: np.zeros(s, dtype=np.float32)

    def dense(p):
        return dict(kernel=z(*p["weight"].shape), bias=z(*p["bias"].shape))

    enc = dict(encoder=dense(P["encoder"]["encoder"]))
    for k, lp in P["encoder"].items():
        if not k.startswith("layers_"):
            continue
        Pn, H = lp["mixer"]["B_real"].shape
        norm = dict(mean=z(H), var=np.ones(H, dtype=np.float32))
        norm.update({n: z(H) for n in ("scale", "bias") if n in lp["norm"]})
        enc[k] = dict(norm=norm, out2=dense(lp["out2"]),
                      mixer=dict(B=z(Pn, H, 2), C=z(H, Pn, 2), D=z(H), Lambda_re=-np.ones(Pn, dtype=np.float32), Lambda_im=z(Pn),
                                 log_step=z(Pn, 1)))
    return dict(encoder=enc, decoder=dense(P["decoder"]))


def _install_integers(model, export):
    """Puts the recorded integer parameters into an eager (op-by-op) model."""
    from sparsernns_amd.fxpmodel import HostComplexFxp, HostFxp

    P, Q = export["params"], export["qconfig"]
    h = lambda a, bits, exp: HostFxp(np.ascontiguousarray(np.asarray(a, dtype=np.int32)), int(bits), int(exp))

    def dense(d, p, q):
        d.weight, d.bias, d._csr = h(p["weight"], q["weight_bits"], q["weight_exp"]), h(p["bias"], q["bias_bits"], q["bias_exp"]), None

    dense(model.encoder.encoder, P["encoder"]["encoder"], Q["encoder"]["encoder"])
    dense(model.decoder, P["decoder"], Q["decoder"])
    for i, layer in enumerate(model.encoder.seq_layers):
        lp, lq = P["encoder"][f"layers_{i}"], Q["encoder"][f"layers_{i}"]
        dense(layer.out2, lp["out2"], lq["out2"])
        m, mq = lp["mixer"], lq["mixer"]
        part = lambda k: h(m[k], mq[f"{k}_bits"], mq[f"{k}_exp"])
        layer.mixer.Lambda_bar = HostComplexFxp(part("A_real"), part("A_imag"))
        layer.mixer.B_bar = HostComplexFxp(part("B_real"), part("B_imag"))
        layer.mixer.C_tilde = HostComplexFxp(part("C_real"), part("C_imag"))
        layer.mixer.D = part("D")
        n, nq = lp["norm"], lq["norm"]
        layer.norm.minus_mean = h(-np.asarray(n["mean"], dtype=np.int64), nq["mean_bits"], nq["mean_exp"])
        layer.norm.invsq_var = h(n["invsq_var"], nq["invsq_var_bits"], nq["invsq_var_exp"])
        layer.norm.scale = h(n["scale"], nq["scale_bits"], nq["scale_exp"]) if "scale" in n else None
        layer.norm.bias = h(n["bias"], nq["bias_bits"], nq["bias_exp"]) if "bias" in n else None


_LOADED = {}
B1_FIXTURES = tuple(n for n in RF.MODEL_FIXTURES if RF.load_json(n)["B"] == 1)   # a clip is its own compute_best batch


@pytest.fixture
def fixture(name):
    """The fixture `name` with one Engine built from its recorded integer export, shared by the tests of this module."""
    from sparsernns_amd.engine import Engine

    if name not in _LOADED:
        meta, export, x, y, inter, md = RF.load_model_fixture(name)
        _LOADED[name] = dict(name=name, meta=meta, export=export, x=x, y=y, inter=inter, md=md, engine=Engine(export))
    return _LOADED[name]


all_fixtures = pytest.mark.parametrize("name", RF.MODEL_FIXTURES)


@all_fixtures
def test_engine_forward_reproduces_the_reference(fixture):
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray

    f, meta, eng = fixture, fixture["meta"], fixture["engine"]
    if f["name"] in RF.RECIPE_FIXTURES:
        assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    fx = FxpArray(f["x"], meta["x_bits"], meta["x_exp"])
    got = eng.forward(fx)                                        # the production path
    assert (got.bits, got.exp) == (meta["y_bits"], meta["y_exp"])
    assert np.array_equal(got.numpy(), f["y"]), f"{np.count_nonzero(got.numpy() != f['y'])} of {f['y'].size} outputs differ"
    if f["name"] in RF.RECIPE_FIXTURES:
        assert eng.lane_status(0).cpu().numpy()[2] == _lib.PATH_FUSED
    got, tr = eng.forward(fx, traces=True)                       # and with its trace planes, by the reference's names
    assert np.array_equal(got.numpy(), f["y"])
    exps, checked = eng.layer_exponents(), 0
    for i in range(eng.n_layers):
        assert exps[i]["residadd"] == meta["inter"][f"encoder.layers_{i}.residadd"][1], i
        for gk, rk in ENGINE_TRACE.items():
            key = f"encoder.layers_{i}.{rk}"
            if key in f["inter"]:
                assert np.array_equal(tr[i][gk].cpu().numpy(), f["inter"][key]), key
                checked += 1
    assert checked >= 2


@all_fixtures
def test_eager_path_reproduces_every_intermediate_by_name(fixture):
    """The op-by-op model (one C ABI call per reference op; a pruned kernel goes through s5fxp_dense_csr): the same names
    as the reference's export()["intermediates"], every (bits, exp), every recorded array."""
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    f, meta = fixture, fixture["meta"]
    md = f["md"] if f["md"] is not None else _dummy_modeldict(f["export"])
    eager = build_regression_model(md, meta["qconfig"], meta["dims"]["n_layers"], store_intermediates=True)
    if f["md"] is None:
        _install_integers(eager, f["export"])
    y = eager(FxpArray(f["x"], meta["x_bits"], meta["x_exp"]))
    assert (y.bits, y.exp) == (meta["y_bits"], meta["y_exp"]) and np.array_equal(y.numpy(), f["y"])
    flat = RF.flat_intermediates(eager.export()["intermediates"])
    assert set(flat) == set(meta["inter"]), sorted(set(flat) ^ set(meta["inter"]))
    for k, (bits, exp) in meta["inter"].items():
        assert (flat[k].bits, flat[k].exp) == (bits, exp), k
    for k, v in f["inter"].items():
        got = flat[k].numpy()
        assert np.array_equal(got, v), f"{k}: {np.count_nonzero(got != v)} of {v.size} values differ"
    if f["name"] == "ref_ndns05_pruned":
        assert eager.decoder._csr is not None and eager.encoder.encoder._csr is not None   # the CSR op really ran


@all_fixtures
def test_layer_forward_reproduces_the_recorded_layer_outputs(fixture):
    from sparsernns_amd.fxparray import FxpArray

    f, meta, eng = fixture, fixture["meta"], fixture["engine"]
    for i in range(eng.n_layers):
        bits, exp = meta["inter"][f"encoder.layers_{i}.ssm_input"]
        out = eng.layer_forward(i, FxpArray(RF.layer_input(f["inter"], i), bits, exp))
        want_key = f"encoder.layers_{i}.output"
        assert (out.bits, out.exp) == tuple(meta["inter"][want_key]), i
        assert np.array_equal(out.numpy(), f["inter"][want_key]), f"layer {i}"


@pytest.mark.parametrize("name", B1_FIXTURES)
def test_clip_kernel_reproduces_a_single_sequence(fixture):
    from sparsernns_amd.fxparray import FxpArray

    f, meta, eng = fixture, fixture["meta"], fixture["engine"]
    assert f["x"].shape[0] == 1
    clip = FxpArray(f["x"][0], meta["x_bits"], meta["x_exp"])
    if f["name"] not in RF.RECIPE_FIXTURES:
        with pytest.raises(NotImplementedError):   # the clip kernel serves the fused path only, and says so
            eng.forward_clips([clip])
        return
    (got,) = eng.forward_clips([clip])
    assert (got.bits, got.exp) == (meta["y_bits"], meta["y_exp"]) and np.array_equal(got.numpy(), f["y"][0])


@all_fixtures
def test_float_and_int16_boundaries_reproduce_the_reference(fixture):
    """s5fxp_model_forward_f32 / _i16.  The float input is the recorded integer input through to_float: exact, and
    fxp_from_fp(FLOOR) at the same (bits, exp) gives the recorded integers back, so the recorded output applies."""
    import torch

    f, meta, eng = fixture, fixture["meta"], fixture["engine"]
    assert int(np.abs(f["x"]).max()) < 2 ** 15 and meta["x_bits"] <= 16 and meta["y_bits"] <= 16
    xf = torch.from_numpy((f["x"].astype(np.float32) / np.float32(1 << meta["x_exp"])).astype(np.float32))
    yf = eng.forward_float(xf, meta["x_bits"], meta["x_exp"]).cpu().numpy()
    want = (f["y"].astype(np.float32) / np.float32(1 << meta["y_exp"])).astype(np.float32)
    assert yf.dtype == np.float32 and np.array_equal(yf.view(np.int32), want.view(np.int32))
    yi = eng.forward_int16(torch.from_numpy(f["x"].astype(np.int16)), meta["x_bits"], meta["x_exp"]).cpu().numpy()
    assert yi.dtype == np.int16 and np.array_equal(yi, f["y"].astype(np.int16))


@all_fixtures
def test_fxprun_check_golden_replays_the_reference_fixtures(name):
    """The ref_* model files keep make_golden.py's layout, so the command line replays them unchanged."""
    import os
    from sparsernns_amd import fxprun

    path = os.path.join(RF.GOLD, name)
    assert fxprun.main(["--model", path + ".npz", "--meta", path + ".json", "--check-golden"]) == 0
