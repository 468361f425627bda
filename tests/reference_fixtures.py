"""Readers of the reference-recorded fixtures tests/golden/ref_* (written by tests/golden/make_reference_golden.py) and
the pieces both tests/test_reference_pin.py and tests/test_reference_gpu.py need: the case runner of the NumPy oracle,
the name map between the reference's ``sow`` keys and the oracle's, and an oracle model built from an integer export.
Nothing here touches a reference checkout."""
import json
import os
import re

import numpy as np

from oracle import fxp_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_FIXTURES = ("ref_tiny_a", "ref_tiny_b_bnscale", "ref_ndns05_b2", "ref_ndns025", "ref_ndns05_pruned", "ref_tiny_w4a8",
                  "ref_tiny_sepexp")
RECIPE_FIXTURES = ("ref_ndns05_b2", "ref_ndns025", "ref_ndns05_pruned")   # the N-DNS recipe: the fused MFMA path must serve them
MODE = dict(FLOOR=O.FLOOR, CEIL=O.CEIL, ROUND=O.ROUND)


def unflatten(flat, sep="/"):
    tree = {}
    for k, v in flat.items():
        node = tree
        parts = k.split(sep)
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = v
    return tree


def load_json(name):
    with open(os.path.join(GOLD, name + ".json")) as f:
        return json.load(f)


def load_packed(name):
    """ref_ops / ref_qconfig: ({array name: ndarray}, json)."""
    meta = load_json(name)
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    flat = {d: z[d] for d in z.files}
    arrays = {k: flat[d][off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape) for k, (d, off, shape) in meta["index"].items()}
    return arrays, meta


_OPS = None


def op_cases():
    """[(index, cfg, inputs, recorded outputs)] of ref_ops; integer arrays widened back to int32."""
    global _OPS
    if _OPS is None:
        arrays, meta = load_packed("ref_ops")
        _OPS = []
        for i, cfg in enumerate(meta["cases"]):
            mine = {k.split("/", 1)[1]: (v.astype(np.int32) if v.dtype.kind == "i" else v) for k, v in arrays.items() if k.startswith(f"{i:03d}/")}
            outs = {k: v for k, v in mine.items() if k.startswith("out") or k == "lut"}
            ins = {k: v for k, v in mine.items() if k not in outs}
            if cfg.get("all_inputs"):
                b = cfg["a_cfg"][0]
                ins = dict(a=np.arange(-(1 << (b - 1)), 1 << (b - 1), dtype=np.int32))
            _OPS.append((i, cfg, ins, outs))
    return _OPS


def load_model_fixture(name):
    """(meta, export, x, y, {reference key: ndarray}, float modeldict or None)."""
    meta = load_json(name)
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    params = unflatten({k[7:]: z[k].astype(np.int32) for k in z.files if k.startswith("params/")})
    inter = {k[6:]: z[k].astype(np.int32) for k in z.files if k.startswith("inter/")}
    md = unflatten({k[3:]: z[k] for k in z.files if k.startswith("md/")}) or None
    export = dict(params=params, qconfig=meta["export_qconfig"])
    return meta, export, z["x"].astype(np.int32), z["y"].astype(np.int32), inter, md


# ---------------------------------------------------------------------------------------------------------------------
# one op-table case through the NumPy oracle: the mirror of make_reference_golden.run_reference
# ---------------------------------------------------------------------------------------------------------------------
def run_oracle(cfg, ins):
    fx = lambda k, c: O.Fx(np.asarray(ins[k], dtype=np.int32), c[0], c[1])
    mode = MODE[cfg["mode"]] if "mode" in cfg else O.FLOOR
    one = lambda r: (dict(out=r.data), [[r.bits, r.exp]])
    two = lambda re, im: (dict(out_re=re.data, out_im=im.data), [[re.bits, re.exp], [im.bits, im.exp]])
    op = cfg["op"]
    if op == "from_fp":
        return one(O.from_fp(ins["x"], cfg["bits"], cfg["exp"], True, mode))
    if op == "to_float":
        return dict(out=fx("a", cfg["a_cfg"]).f32()), []
    if op == "change_exp":
        return one(O.change_exp(fx("a", cfg["a_cfg"]), cfg["new_exp"], mode))
    if op == "change_cfg":
        return one(O.change_cfg(fx("a", cfg["a_cfg"]), cfg["new_bits"], cfg["new_exp"], True, mode))
    if op in ("add", "sub", "mul"):
        f = dict(add=O.add, sub=O.sub, mul=O.mul)[op]
        return one(f(fx("a", cfg["a_cfg"]), fx("b", cfg["b_cfg"]), cfg["result_bits"], cfg["result_exp"], mode))
    if op == "matmul":
        return one(O.matmul(fx("a", cfg["a_cfg"]), fx("b", cfg["b_cfg"]), cfg["result_bits"], cfg["result_exp"], mode))
    if op in ("complex_add", "complex_mul"):
        ar, ai, br, bi = fx("ar", cfg["a_cfg"]), fx("ai", cfg["a_cfg"]), fx("br", cfg["b_cfg"]), fx("bi", cfg["b_cfg"])
        (b0, b1), (e0, e1) = cfg["result_bits"], cfg["result_exp"]
        if op == "complex_add":
            return two(O.add(ar, br, b0, e0, mode), O.add(ai, bi, b1, e1, mode))
        # fxparray.py:504-570: four products at the part's own (bits, exp), then a subtraction and an addition there
        arbr, aibi = O.mul(ar, br, b0, e0, mode), O.mul(ai, bi, b0, e0, mode)
        aibr, arbi = O.mul(ai, br, b1, e1, mode), O.mul(ar, bi, b1, e1, mode)
        return two(O.sub(arbr, aibi, b0, e0, mode), O.add(arbi, aibr, b1, e1, mode))
    if op == "clip":
        a = fx("a", cfg["a_cfg"])
        return one(O.Fx(O.sat(a.data, a.bits), a.bits, a.exp))
    if op == "relu":
        return one(O.relu(fx("a", cfg["a_cfg"])))
    if op == "relu_complex":
        return two(*O.complex_relu(fx("ar", cfg["a_cfg"]), fx("ai", cfg["a_cfg"])))
    if op == "sigmoid":
        lut = O.sigmoid_lut(cfg["x_exp"], cfg["y_exp"])
        outs, c = one(O.sigmoid_apply(fx("a", cfg["a_cfg"]), cfg["x_exp"], cfg["y_exp"], lut))
        outs["lut"] = lut
        return outs, c
    if op == "scan":
        e = cfg["bu_exp"]
        xr, xi = O.scan(O.Fx(ins["bu_re"], 32, e), O.Fx(ins["bu_im"], 32, e), O.Fx(ins["a_re"], 16, cfg["a_exp"]),
                        O.Fx(ins["a_im"], 16, cfg["a_exp"]), cfg["x_exp"], cfg["x_exp"])
        return dict(out_re=xr, out_im=xi), []
    raise KeyError(op)


def assert_case_equal(tag, got, got_cfg, want, want_cfg):
    assert [list(c) for c in got_cfg] == [list(c) for c in want_cfg], f"{tag}: (bits, exp) {got_cfg} != recorded {want_cfg}"
    assert set(got) == set(want), f"{tag}: outputs {sorted(got)} != recorded {sorted(want)}"
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, f"{tag} {k}: shape {g.shape} != {w.shape}"
        if w.dtype.kind == "f":
            same = g.astype(np.float32).view(np.int32) == w.astype(np.float32).view(np.int32)
        else:
            same = g.astype(np.int64) == w.astype(np.int64)
        assert same.all(), f"{tag} {k}: {np.count_nonzero(~same)} of {w.size} values differ, first at {np.argwhere(~same)[0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# names: the reference's sow keys (export()["intermediates"], flattened with '.', complex parts as .real / .imag) and
# the oracle's (O.flatten_intermediates)
# ---------------------------------------------------------------------------------------------------------------------
# The reference run names 49 intermediates (a complex pair counted once), the oracle 48 tensors.  Every reference key
# maps to an oracle tensor below, so the oracle lacks NO tensor: the reference's surplus are second names for a tensor
# it already sows (norm.norm_input = ssm_input, pre_C = mixer.xs_relu, encoder.encoder.__call__ = encoder.encoder_output,
# encoder.layer_i_output = layers_i.output, the top-level encoder_output = the last layer's output, decoder.__call__ =
# output); the oracle deliberately keeps one name per tensor and the duplicates are checked against it all the same.
# The other way round the oracle names one tensor the reference never sows, ``mixer.u`` (the SSM input after its
# change_cfg, fxpmodel.py:610-627): ORACLE_ONLY.  It is pinned indirectly, as the operand of Bu_elements and Du.
_LAYER = {
    "ssm_input": "ssm_input", "norm.norm_input": "ssm_input", "norm.norm_input_minus_mean": "norm.norm_input_minus_mean",
    "norm.norm_output_raw": "norm.norm_output_raw", "norm.norm_output_scaled": "norm.norm_output_scaled",
    "norm.norm_output_scaled_bias": "norm.norm_output_scaled_bias", "norm.norm_output": "norm.norm_output", "pre_s5": "pre_s5",
    "mixer.Bu_elements.real": "mixer.Bu_re", "mixer.Bu_elements.imag": "mixer.Bu_im", "mixer.xs.real": "mixer.xs_re",
    "mixer.xs.imag": "mixer.xs_im", "mixer.xs_relu.real": "mixer.xs_relu_re", "mixer.xs_relu.imag": "mixer.xs_relu_im",
    "pre_C.real": "mixer.xs_relu_re", "pre_C.imag": "mixer.xs_relu_im", "mixer.Cxs": "mixer.Cxs", "mixer.2Cxs": "mixer.Cxs2",
    "mixer.Du": "mixer.Du", "mixer.ys": "mixer.ys", "pre_GLU": "pre_GLU", "out2.__call__": "out2", "out2_sigmoid": "out2_sigmoid",
    "post_GLU": "post_GLU", "residadd": "residadd", "output": "output",
}
_TOP = {"encoder.pre_encoder": "pre_encoder", "encoder.encoder.__call__": "encoder_output", "encoder.encoder_output": "encoder_output",
        "encoder.encoder_output_relu": "encoder_output_relu", "decoder.__call__": "output", "output": "output"}
ORACLE_ONLY = ("mixer.u",)


def oracle_name(ref_key: str, n_layers: int) -> str:
    """The oracle's name of a reference intermediate; KeyError for a key the map does not know."""
    if ref_key in _TOP:
        return _TOP[ref_key]
    if ref_key == "encoder_output":
        return f"layers_{n_layers - 1}.output"
    m = re.fullmatch(r"encoder\.layer_(\d+)_output", ref_key)
    if m:
        return f"layers_{m.group(1)}.output"
    m = re.fullmatch(r"encoder\.(layers_\d+)\.(.+)", ref_key)
    if m:
        return f"{m.group(1)}.{_LAYER[m.group(2)]}"
    raise KeyError(ref_key)


# the scalar C half's trace planes (oracle/cref.py TRACE_KEYS) under the reference's keys
CREF_TRACE = {"pre_s5": "pre_s5", "bu_re": "mixer.Bu_elements.real", "bu_im": "mixer.Bu_elements.imag", "xs_re": "mixer.xs.real",
              "xs_im": "mixer.xs.imag", "ys": "mixer.ys", "out2": "out2.__call__", "sigmoid": "out2_sigmoid", "post_glu": "post_GLU",
              "residadd": "residadd"}


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy oracle's model from an INTEGER export (the wide fixtures carry no float parameters)
# ---------------------------------------------------------------------------------------------------------------------
def oracle_from_export(export) -> O.RegressionModel:
    P, Q = export["params"], export["qconfig"]
    fx = lambda a, bits, exp: O.Fx(np.asarray(a, dtype=np.int32), int(bits), int(exp))

    def dense(p, q):
        d = O.Dense.__new__(O.Dense)
        d.qc = {k: int(q[k]) for k in ("inp_bits", "inp_exp", "out_bits", "out_exp")}
        d.weight = fx(p["weight"], q["weight_bits"], q["weight_exp"])
        d.bias = fx(p["bias"], q["bias_bits"], q["bias_exp"])
        return d

    model = O.RegressionModel.__new__(O.RegressionModel)
    model.encoder = dense(P["encoder"]["encoder"], Q["encoder"]["encoder"])
    model.decoder = dense(P["decoder"], Q["decoder"])
    model.layers = []
    for i in range(len([k for k in P["encoder"] if k.startswith("layers_")])):
        lp, lq = P["encoder"][f"layers_{i}"], Q["encoder"][f"layers_{i}"]
        s = O.SSM.__new__(O.SSM)
        m, mq = lp["mixer"], lq["mixer"]
        s.qc = dict(activations={k: dict(bits=int(mq[f"{k}_bits"]), exp=int(mq[f"{k}_exp"])) for k in ("u", "Bu_re", "Bu_im", "x_re", "x_im", "y")})
        for attr, k in (("A_re", "A_real"), ("A_im", "A_imag"), ("B_re", "B_real"), ("B_im", "B_imag"), ("C_re", "C_real"),
                        ("C_im", "C_imag"), ("D", "D")):
            setattr(s, attr, fx(m[k], mq[f"{k}_bits"], mq[f"{k}_exp"]))
        n, nq = lp["norm"], lq["norm"]
        bn = O.BatchNorm.__new__(O.BatchNorm)
        bn.minus_mean = fx(O.mul32(np.asarray(n["mean"], dtype=np.int32), np.asarray(-1, dtype=np.int32)), nq["mean_bits"], nq["mean_exp"])
        bn.invsq_var = fx(n["invsq_var"], nq["invsq_var_bits"], nq["invsq_var_exp"])
        bn.scale = fx(n["scale"], nq["scale_bits"], nq["scale_exp"]) if "scale" in n else None
        bn.bias = fx(n["bias"], nq["bias_bits"], nq["bias_exp"]) if "bias" in n else None
        layer = O.SequenceLayer.__new__(O.SequenceLayer)
        layer.qc = dict(multgate={k: int(v) for k, v in lq["multgate"].items()})
        layer.norm, layer.mixer, layer.out2 = bn, s, dense(lp["out2"], lq["out2"])
        layer.sig_x_exp, layer.sig_y_exp = int(lq["sigmoid"]["x_exp"]), int(lq["sigmoid"]["y_exp"])
        layer.lut = O.sigmoid_lut(layer.sig_x_exp, layer.sig_y_exp)
        model.layers.append(layer)
    return model


def tree_assert_equal(a, b, path=""):
    """Key for key, both ways; numbers by value, arrays element by element."""
    if isinstance(a, dict) or isinstance(b, dict):
        assert isinstance(a, dict) and isinstance(b, dict), f"{path}: {type(a).__name__} vs {type(b).__name__}"
        assert set(map(str, a)) == set(map(str, b)), f"{path}: keys {sorted(set(map(str, a)) ^ set(map(str, b)))} on one side only"
        for k in a:
            tree_assert_equal(a[k], b[k] if k in b else b[str(k)], f"{path}/{k}")
        return
    x, y = np.asarray(a), np.asarray(b)
    assert x.shape == y.shape and np.array_equal(x, y), f"{path}: {a!r} != {b!r}"


def flat_intermediates(tree, prefix=""):
    """export()["intermediates"] of the reference's layout (the product's eager model keeps the same one), flattened with
    '.'; a complex pair as <key>.real / <key>.imag."""
    out = {}
    for k, v in tree.items():
        if isinstance(v, dict):
            out.update(flat_intermediates(v, f"{prefix}{k}."))
        elif v is None:
            continue
        elif hasattr(v, "real") and hasattr(v, "imag") and not hasattr(v, "data"):
            out[f"{prefix}{k}.real"], out[f"{prefix}{k}.imag"] = v.real, v.imag
        else:
            out[f"{prefix}{k}"] = v
    return out


def layer_input(inter, i):
    """The recorded input of layer i: its ssm_input, or the same tensor under the name its producer sowed it."""
    for key in (f"encoder.layers_{i}.ssm_input", "encoder.encoder_output_relu" if i == 0 else f"encoder.layers_{i - 1}.output",
                f"encoder.layer_{i - 1}_output"):
        if key in inter:
            return inter[key]
    raise KeyError(f"no recorded input for layer {i}")
