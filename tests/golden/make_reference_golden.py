#!/usr/bin/env python3
"""Records what the REFERENCE's own integer code computes, as fixtures tests/golden/ref_*.npz + .json.

Needs a reference checkout (oracle/refload.py: environment variable SPARSERNNS_REFERENCE).  The reference's
``fxparray.py`` / ``fxputils.py`` / ``fxpmodel.py`` are executed in place under the NumPy stand-in oracle/jaxlike.py;
nothing here calls oracle/fxp_oracle.py to produce a recorded value (the one shared piece is the float ZOH
discretisation, see oracle/refload.py).  So the files pin the reference's program logic -- exponents, order of shift /
clip / wrap, LUT construction, wiring, compute_best scope, qconfig derivation -- under the stand-in's stated arithmetic;
they do not pin XLA.  tests/test_reference_pin.py regenerates every file from the checkout and compares byte for byte
(json text, and name + bytes of every npz member), so a fixture can neither go stale nor be written from the oracle.

Usage: ``make_reference_golden.py [--fresh] [fixture names]``.  Without --fresh a fixture's float calibration inputs are
read back from the committed file (load_prior), so the same bytes come out on any machine; use --fresh after changing a
recipe in MODELS / QCONFIG_CASES.

Files hold arrays, settings and names only (``allow_pickle=False``).  Model fixtures use make_golden.py's layout
(``params/...``, ``x``, ``y``, ``inter/...`` in the npz; ``export_qconfig``, ``x_bits`` ... in the json), so
``fxprun --model F.npz --meta F.json --check-golden`` replays them.  Intermediates are stored under the reference's own
``sow`` keys; a complex one as ``<key>.real`` / ``<key>.imag``.
"""
import contextlib
import io
import json
import os
import pickle
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import jaxlike, refload  # noqa: E402
from sparsernns_amd import fxputils, synth  # noqa: E402

MODES = ("FLOOR", "CEIL", "ROUND")
F32 = np.float32

_TINY_B = dict(H=12, P=6, d_in=7, d_out=9, n_layers=2)
MODELS = {
    "ref_tiny_a": dict(make=dict(dims=synth.tiny_dims(), seed=7), B=2, L=24, scale=1.0),
    "ref_tiny_b_bnscale": dict(make=dict(dims=synth.tiny_dims(**_TINY_B), bn_scale_bias=True, input_scale=30.0, seed=11),
                               B=2, L=20, scale=30.0),
    # one frame past a 32-frame tile, batched: the compute_best maxima span both sequences
    "ref_ndns05_b2": dict(make=dict(dim_scale=0.5, seed=1919), B=2, L=33, scale=1.0),
    "ref_ndns025": dict(make=dict(dim_scale=0.25, seed=1919), B=1, L=16, scale=1.0),
    "ref_ndns05_pruned": dict(make=dict(dim_scale=0.5, sparsity=0.9, seed=1919), B=1, L=16, scale=1.0),
    "ref_tiny_w4a8": dict(make=dict(dims=synth.tiny_dims(**_TINY_B), quantization="w4a8", bn_stats="random",
                                    input_scale=300.0, seed=5), B=2, L=20, scale=300.0),
    # fxprun's --separate_exponents layout: per-layer blocks, derived by fxputils from the calibration trees
    "ref_tiny_sepexp": dict(make=dict(dims=synth.tiny_dims(**_TINY_B), bn_scale_bias=True, seed=13), B=1, L=16, scale=1.0,
                            separate_exponents=True),
}
# the wide models keep a subset of the intermediate ARRAYS (every intermediate's (bits, exp) is kept in the json): what
# s5fxp_layer_forward needs -- each layer's input and output -- and one tensor from each side of the recurrence
WIDE_KEEP = ("encoder.encoder_output_relu", ".output", "mixer.ys", "residadd", "mixer.xs.real", "mixer.Bu_elements.imag",
             "norm.norm_output", "out2_sigmoid")
KEEP = {"ref_ndns05_b2": ("encoder.encoder_output_relu", "layers_0.output", "layers_1.output", "layers_2.output",
                          "layers_1.mixer.xs.real", "layers_2.mixer.ys")}


def narrow(a: np.ndarray) -> np.ndarray:
    """The narrowest signed integer dtype that holds an integer array (floats and bools pass through)."""
    a = np.asarray(a)
    if a.dtype.kind != "i":
        return a
    m = max(int(a.max(initial=0)), -int(a.min(initial=0)) - 1)
    return a.astype(np.int8 if m < 128 else np.int16 if m < 32768 else np.int32)


def flatten(tree, prefix="", sep="/"):
    out = {}
    for k, v in tree.items():
        if isinstance(v, dict):
            out.update(flatten(v, f"{prefix}{k}{sep}", sep))
        else:
            out[f"{prefix}{k}"] = v
    return out


def plain(tree):
    """A tree with NumPy / stand-in scalars as Python numbers (for json)."""
    if isinstance(tree, dict):
        return {str(k): plain(v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return [plain(v) for v in tree]
    if isinstance(tree, (np.ndarray, np.generic)):
        a = jaxlike.to_numpy(tree)
        return a.item() if a.ndim == 0 else a.tolist()
    return tree


# ---------------------------------------------------------------------------------------------------------------------
# op table
# ---------------------------------------------------------------------------------------------------------------------
def rnd(rng, bits, shape, extremes=True):
    """Integers that fit `bits` signed bits -- the contract of an FxpArray operand -- both ends of the range included."""
    a = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=shape, dtype=np.int64).astype(np.int32)
    if extremes and a.size >= 2:
        a.flat[0], a.flat[1] = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return a


def random_arith_case(rng):
    """One random add / sub / mul / change_exp / change_cfg / matmul / from_fp configuration, generated INSIDE each op's
    contract (values fit their declared width; mul and matmul shifts >= 0, >= 1 under ROUND whose half-ulp term is
    1 << (shift - 1)); nothing is filtered after generation."""
    op = str(rng.choice(["add", "sub", "mul", "add", "mul", "change_exp", "change_cfg", "matmul", "from_fp"]))
    mode = str(rng.choice(MODES))
    ba, bb = int(rng.choice([8, 16])), int(rng.choice([8, 16]))
    ea, eb = int(rng.integers(2, 15)), int(rng.integers(2, 15))
    rb = int(rng.choice([8, 16, 24]))
    a = rnd(rng, ba, (6, 37))
    b = rnd(rng, bb, (6, 37) if rng.random() < 0.5 else (37,))
    if op in ("add", "sub", "mul"):
        best = rng.random() < 0.4
        if best and op == "mul":
            # the chosen exponent is at most max(ba, bb) - 1: exponents from 8 up keep the product's shift >= 0
            ea, eb = int(rng.integers(8, 15)), int(rng.integers(8, 15))
            cfg = dict(result_bits=None, result_exp="compute_best", mode="FLOOR")
        elif best:
            cfg = dict(result_bits=[None, 16, 24][int(rng.integers(0, 3))], result_exp="compute_best", mode="FLOOR")
        else:
            top = min(15, ea + eb - (1 if mode == "ROUND" else 0)) if op == "mul" else 15
            cfg = dict(result_bits=rb, result_exp=int(rng.integers(0, top + 1)), mode=mode)
        return dict(op=op, a_cfg=[ba, ea], b_cfg=[bb, eb], **cfg), dict(a=a, b=b)
    if op == "change_exp":
        return dict(op=op, a_cfg=[ba, ea], new_exp=int(rng.integers(0, 16)), mode=mode), dict(a=a)
    if op == "change_cfg":
        return dict(op=op, a_cfg=[ba, ea], new_bits=rb, new_exp=int(rng.integers(0, 16)), mode=mode), dict(a=a)
    if op == "matmul":
        w = rnd(rng, bb, (37, 5))
        top = min(15, ea + eb - (1 if mode == "ROUND" else 0))
        return dict(op=op, a_cfg=[ba, ea], b_cfg=[bb, eb], result_bits=rb, result_exp=int(rng.integers(0, top + 1)),
                    mode=mode), dict(a=a, b=w)
    x = (rng.standard_normal(120) * 10.0 ** int(rng.integers(-3, 8))).astype(F32)
    return dict(op="from_fp", bits=rb, exp=int(rng.integers(0, 16)), mode=mode), dict(x=x)


def op_cases():
    """[(cfg, inputs)]: the hand-built edges first, then seeded random configurations."""
    rng = np.random.default_rng(20240)
    cases = []
    add = lambda cfg, **ins: cases.append((cfg, ins))
    # from_fp: ties, clip borders and beyond, values beyond int32, +-0, NaN
    for bits, exp in ((16, 8), (8, 4), (16, 13), (24, 10)):
        top = F32(1 << (bits - 1)) / F32(1 << exp)
        ulp = F32(1.0) / F32(1 << exp)
        x = np.concatenate([
            (rng.standard_normal(150) * float(top) / 3).astype(F32),
            ((np.arange(-40, 40) + 0.5) * ulp).astype(F32),                      # ties
            np.array([top, -top, top - ulp, -top - ulp, top - ulp / 2, -top + ulp / 2, top + ulp, 2 * top, -2 * top], dtype=F32),
            np.array([0.0, -0.0, np.nan, 1e6, -1e6, 3e9, -3e9, 1e20, -1e20, 2.0 ** 31 / (1 << exp), -(2.0 ** 31) / (1 << exp)], dtype=F32)])
        for mode in MODES:
            add(dict(op="from_fp", bits=bits, exp=exp, mode=mode), x=x)
    # to_float: int32 -> float32 rounds to nearest even beyond 24 bits
    wide = np.concatenate([rnd(rng, 32, (200,)), np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 2 ** 25 + 2, 2 ** 25 + 6], dtype=np.int32)])
    for exp in (0, 7, 15):
        add(dict(op="to_float", a_cfg=[32, exp]), a=wide)
    # change_exp / change_cfg: both directions, three modes; a left shift saturates at the OLD width (and wraps int32 first)
    for bits, exp, new_exp in ((16, 12, 8), (16, 12, 3), (16, 8, 12), (16, 8, 15), (8, 4, 7), (24, 5, 15), (16, 9, 9)):
        for mode in MODES:
            add(dict(op="change_exp", a_cfg=[bits, exp], new_exp=new_exp, mode=mode), a=rnd(rng, bits, (6, 37)))
    for bits, exp, nb, ne in ((16, 12, 8, 8), (16, 8, 24, 12), (8, 4, 16, 9), (16, 8, 8, 12), (24, 14, 16, 6), (16, 10, 16, 10),
                              (16, 10, 12, 10), (16, 6, 24, 14)):
        for mode in MODES:
            add(dict(op="change_cfg", a_cfg=[bits, exp], new_bits=nb, new_exp=ne, mode=mode), a=rnd(rng, bits, (6, 37)))
    # compute_best with the maximum either side of a power of two (value / 2**6 next to 2**k)
    for k in (0, 1, 4, 9, 13):
        for delta in (-2, -1, 0, 1, 2):
            v = (1 << k) * 64 + delta
            a = rng.integers(-40, 40, size=(4, 9)).astype(np.int32)
            a[2, 3] = v if (k + delta) % 2 else -v
            z = rng.integers(-1, 2, size=(9,)).astype(np.int32)
            add(dict(op="add", a_cfg=[24, 6], b_cfg=[24, 6], result_bits=None, result_exp="compute_best", mode="FLOOR"), a=a, b=z)
            one = np.full((9,), 1 << 12, dtype=np.int32)
            add(dict(op="mul", a_cfg=[24, 6], b_cfg=[16, 12], result_bits=16, result_exp="compute_best", mode="FLOOR"), a=a, b=one)
    # sub: -1 * data is NOT clipped before the add (the most negative value wraps back to itself); fixed and compute_best
    for mode in MODES:
        add(dict(op="sub", a_cfg=[16, 12], b_cfg=[16, 9], result_bits=16, result_exp=9, mode=mode), a=rnd(rng, 16, (6, 37)), b=rnd(rng, 16, (37,)))
    add(dict(op="sub", a_cfg=[16, 12], b_cfg=[16, 12], result_bits=24, result_exp=14, mode="FLOOR"), a=rnd(rng, 16, (6, 37)), b=rnd(rng, 16, (6, 37)))
    add(dict(op="sub", a_cfg=[16, 10], b_cfg=[8, 5], result_bits=None, result_exp="compute_best", mode="FLOOR"), a=rnd(rng, 16, (6, 37)), b=rnd(rng, 8, (37,)))
    add(dict(op="sub", a_cfg=[32, 4], b_cfg=[32, 4], result_bits=32, result_exp=4, mode="FLOOR"), a=rnd(rng, 32, (6, 37)), b=rnd(rng, 32, (6, 37)))
    # matmul: 16 x 8 bit at the model's shapes' remainders, and full-range operands whose accumulation wraps int32
    add(dict(op="matmul", a_cfg=[16, 12], b_cfg=[8, 7], result_bits=16, result_exp=11, mode="FLOOR"), a=rnd(rng, 16, (2, 9, 40)), b=rnd(rng, 8, (40, 12)))
    add(dict(op="matmul", a_cfg=[32, 10], b_cfg=[32, 5], result_bits=24, result_exp=9, mode="FLOOR"), a=rnd(rng, 32, (7, 33)), b=rnd(rng, 32, (33, 5)))
    add(dict(op="matmul", a_cfg=[16, 3], b_cfg=[16, 2], result_bits=32, result_exp=5, mode="FLOOR"), a=rnd(rng, 16, (5, 65)), b=rnd(rng, 16, (65, 3)))
    # complex add / mul, clip, relu
    for mode in MODES:
        ins = dict(ar=rnd(rng, 16, (5, 21)), ai=rnd(rng, 16, (5, 21)), br=rnd(rng, 16, (21,)), bi=rnd(rng, 16, (21,)))
        add(dict(op="complex_add", a_cfg=[16, 12], b_cfg=[16, 9], result_bits=[16, 24], result_exp=[10, 13], mode=mode), **ins)
        add(dict(op="complex_mul", a_cfg=[16, 12], b_cfg=[16, 9], result_bits=[24, 16], result_exp=[11, 6], mode=mode), **ins)
    add(dict(op="clip", a_cfg=[16, 4]), a=rnd(rng, 32, (300,)))
    add(dict(op="clip", a_cfg=[8, 4]), a=rnd(rng, 12, (300,)))
    add(dict(op="relu", a_cfg=[16, 9]), a=rnd(rng, 16, (6, 37)))
    re = np.concatenate([np.array([5, 0, 0, 0, -3, 2 ** 24 + 1, -(2 ** 24) - 1, 7, 2 ** 31 - 1], dtype=np.int64).astype(np.int32), rnd(rng, 16, (200,)), np.zeros(50, np.int32)])
    im = np.concatenate([np.array([-9, 4, 0, -4, 8, 2 ** 24 + 3, 5, 2 ** 30 + 1, -(2 ** 31)], dtype=np.int64).astype(np.int32), rnd(rng, 16, (200,)), rnd(rng, 16, (50,))])
    add(dict(op="relu_complex", a_cfg=[16, 3]), ar=re, ai=im)
    # FxpSigmoid over every 16-bit input (and every 8-bit one), at the exponents SequenceLayer derives: min(out_exp, 6), bits - 2
    for xe_in, bits in ((12, 16), (6, 16), (4, 16), (9, 8)):
        add(dict(op="sigmoid", a_cfg=[bits, xe_in], x_exp=min(xe_in, 6), y_exp=bits - 2, all_inputs=True))
    # recurrent_loop: 30-bit Bu, so A * x wraps modulo 2**32; unbatched and through vmap
    for shape, sh in (((40, 5), 1), ((3, 33, 7), -2)):
        add(dict(op="scan", bu_exp=15, a_exp=15, x_exp=15 - sh, batched=len(shape) == 3),
            bu_re=rnd(rng, 30, shape), bu_im=rnd(rng, 30, shape), a_re=rnd(rng, 16, shape[-1:]), a_im=rnd(rng, 16, shape[-1:]))
    add(dict(op="scan", bu_exp=12, a_exp=14, x_exp=12, batched=True),
        bu_re=rnd(rng, 16, (2, 50, 6)), bu_im=rnd(rng, 16, (2, 50, 6)), a_re=rnd(rng, 16, (6,)), a_im=rnd(rng, 16, (6,)))
    for _ in range(40):
        cases.append(random_arith_case(rng))
    return cases


def case_inputs(cfg, ins):
    """Adds the implied input of a case that stores none."""
    if cfg.get("all_inputs"):
        b = cfg["a_cfg"][0]
        return dict(a=np.arange(-(1 << (b - 1)), 1 << (b - 1), dtype=np.int32))
    return ins


def run_reference(ref, cfg, ins):
    """One op-table case through the reference.  Returns ({name: ndarray}, [[bits, exp], ...] per output)."""
    R, M, J = ref.fxparray, ref.fxpmodel, jaxlike.numpy
    ins = case_inputs(cfg, ins)
    fx = lambda k, c: R.FxpArray(J.asarray(ins[k]), bits=c[0], exp=c[1], signed=True)
    mode = R.RoundingMode[cfg["mode"]] if "mode" in cfg else None
    one = lambda r: (dict(out=jaxlike.to_numpy(r.data)), [[r.bits, r.exp]])
    two = lambda r: (dict(out_re=jaxlike.to_numpy(r.real.data), out_im=jaxlike.to_numpy(r.imag.data)),
                     [[r.real.bits, r.real.exp], [r.imag.bits, r.imag.exp]])
    op = cfg["op"]
    if op == "from_fp":
        return one(R.fxp_from_fp(J.asarray(ins["x"]), bits=cfg["bits"], exp=cfg["exp"], signed=True, round_mode=mode, warn_on_clip=False))
    if op == "to_float":
        return dict(out=jaxlike.to_numpy(fx("a", cfg["a_cfg"]).to_float())), []
    if op == "change_exp":
        return one(R.fxp_change_exp(fx("a", cfg["a_cfg"]), cfg["new_exp"], mode, warn_on_clip=False))
    if op == "change_cfg":
        return one(R.fxp_change_cfg(fx("a", cfg["a_cfg"]), cfg["new_bits"], cfg["new_exp"], True, mode, warn_on_clip=False))
    if op in ("add", "sub", "mul"):
        a, b = fx("a", cfg["a_cfg"]), fx("b", cfg["b_cfg"])
        kw = dict(result_bits=cfg["result_bits"], result_exp=cfg["result_exp"], round_mode=mode, warn_on_overflow=False)
        return one({"add": R.fxp_add, "sub": R.fxp_sub, "mul": R.fxp_mul}[op](a, b, **kw))
    if op == "matmul":
        with contextlib.redirect_stdout(io.StringIO()):
            return one(R.fxp_matmul(fx("a", cfg["a_cfg"]), fx("b", cfg["b_cfg"]), result_bits=cfg["result_bits"],
                                    result_exp=cfg["result_exp"], round_mode=mode))
    if op in ("complex_add", "complex_mul"):
        a = R.ComplexFxpArray(fx("ar", cfg["a_cfg"]), fx("ai", cfg["a_cfg"]))
        b = R.ComplexFxpArray(fx("br", cfg["b_cfg"]), fx("bi", cfg["b_cfg"]))
        f = R.fxp_complex_add if op == "complex_add" else R.fxp_complex_mul
        return two(f(a, b, result_exp=tuple(cfg["result_exp"]), result_bits=tuple(cfg["result_bits"]), round_mode=mode,
                     warn_on_overflow=False, warn_on_clip=False))
    if op == "clip":
        return one(R.fxp_clip(fx("a", cfg["a_cfg"])))
    if op == "relu":
        return one(M.fxp_relu(fx("a", cfg["a_cfg"])))
    if op == "relu_complex":
        return two(M.fxp_relu(R.ComplexFxpArray(fx("ar", cfg["a_cfg"]), fx("ai", cfg["a_cfg"]))))
    if op == "sigmoid":
        s = M.FxpSigmoid(x_exp=cfg["x_exp"], y_exp=cfg["y_exp"])
        r = s.apply(fx("a", cfg["a_cfg"]))
        outs, c = one(r)
        outs["lut"] = jaxlike.to_numpy(s.lut)
        return outs, c
    if op == "scan":
        zeros = J.zeros(ins["bu_re"].shape[:-2] + ins["bu_re"].shape[-1:], dtype=np.int32)
        loop = jaxlike.vmap(M.recurrent_loop, in_axes=(0, 0, None, None, 0, 0) + (None,) * 6) if cfg["batched"] else M.recurrent_loop
        xs = loop(J.asarray(ins["bu_re"]), J.asarray(ins["bu_im"]), J.asarray(ins["a_re"]), J.asarray(ins["a_im"]), zeros, zeros,
                  cfg["bu_exp"], cfg["bu_exp"], cfg["a_exp"], cfg["a_exp"], cfg["x_exp"], cfg["x_exp"])
        xs = jaxlike.to_numpy(xs)
        return dict(out_re=xs[..., 0], out_im=xs[..., 1]), []
    raise KeyError(op)


def pack(named):
    """Many small arrays as one flat array per dtype (an npz member costs a few hundred bytes each):
    ({dtype name: flat array}, {name: [dtype name, offset, shape]})."""
    flat, index = {}, {}
    for k, v in named.items():
        v = np.asarray(v)
        d = v.dtype.name
        parts = flat.setdefault(d, [])
        index[k] = [d, int(sum(p.size for p in parts)), list(v.shape)]
        parts.append(v.reshape(-1))
    return {d: np.concatenate(p) for d, p in flat.items()}, index


def unpack(z, index):
    return {k: np.asarray(z[d][off:off + int(np.prod(shape, dtype=np.int64))]).reshape(shape) for k, (d, off, shape) in index.items()}


def record_ops(ref):
    named, meta = {}, []
    for i, (cfg, ins) in enumerate(op_cases()):
        outs, out_cfg = run_reference(ref, cfg, ins)
        for k, v in {**ins, **outs}.items():
            named[f"{i:03d}/{k}"] = narrow(v)
        meta.append(dict(cfg, out_cfg=out_cfg))
    arrays, index = pack(named)
    return arrays, dict(cases=meta, index=index)


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
def make_case_model(c):
    """(modeldict, fxp_qconfig, dims) of a MODELS entry."""
    if not c.get("separate_exponents"):
        return synth.make_model(**c["make"])
    mk = dict(c["make"])
    dims = mk.pop("dims")
    seed = mk.pop("seed")
    md = synth.make_float_params(dims, seed, mk.get("bn_scale_bias", False))
    stats = {}
    synth.float_forward(md, synth.make_input(2, 128, dims["d_in"], seed=seed + 1), dims["n_layers"], calibrate_bn=True, stats=stats)
    md2, qc = fxputils.derive(*synth.reference_trees(md, stats, dims["n_layers"]), "w8a16", separate_exponents=True)
    return md2, qc, dims


def flat_intermediates(tree, prefix=""):
    """The reference's export()["intermediates"] as {'encoder.layers_0.mixer.xs.real': FxpArray, ...}."""
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


def load_prior(name):
    """The committed fixture `name` as (npz, json), or None.  A fixture's FLOAT inputs -- BatchNorm statistics and
    observer maxima come out of float32 matrix products, whose last bit depends on the BLAS kernel a CPU selects -- are
    taken from the committed file when there is one, so that regenerating on another machine feeds the reference the
    same numbers; everything the reference computes from them is computed afresh.  --fresh ignores the committed files."""
    path = os.path.join(HERE, name)
    if not (os.path.exists(path + ".npz") and os.path.exists(path + ".json")):
        return None
    with open(path + ".json") as f:
        return np.load(path + ".npz", allow_pickle=False), json.load(f)


def _set_leaf(tree, path, value):
    *head, last = path.split("/")
    for k in head:
        tree = tree[k]
    tree[last] = value


def record_model(ref, name, prior=None):
    c = MODELS[name]
    md, qc, dims = make_case_model(c)
    if prior is not None:
        z, pmeta = prior
        qc = pmeta["qconfig"]
        for k in z.files:
            if k.startswith(("md/", "cal/")):
                _set_leaf(md, k.split("/", 1)[1], np.array(z[k]))
    xf = synth.make_input(c["B"], c["L"], dims["d_in"], seed=3, scale=c["scale"])
    xf[1:] *= F32(0.25)   # a quiet second sequence: alone it would choose finer compute_best exponents than the batch does
    R = ref.fxparray
    with contextlib.redirect_stdout(io.StringIO()):
        model = refload.build_model(ref, md, qc, dims)
        x = R.fxp_from_fp(jaxlike.numpy.asarray(xf), bits=qc["encoder"]["inp_bits"], exp=qc["encoder"]["inp_exp"], signed=True,
                          round_mode=R.RoundingMode.FLOOR)
        y = model(x, 10)
        ex = model.export()
    small = dims["H"] <= 16
    leaves = {k: v for k, v in flatten(md).items() if isinstance(v, np.ndarray) and v.dtype.kind == "f"}
    if small and not c.get("separate_exponents"):
        arrays = {f"md/{k}": np.asarray(v) for k, v in leaves.items()}
    else:   # the calibrated BatchNorm statistics: the one float input of a wide fixture that is not a pure function of its seed
        arrays = {f"cal/{k}": np.asarray(v) for k, v in leaves.items() if k.endswith(("norm/mean", "norm/var"))}
    for k, v in flatten(ex["params"]).items():
        arrays[f"params/{k}"] = narrow(jaxlike.to_numpy(v))
    arrays["x"] = narrow(jaxlike.to_numpy(x.data))
    arrays["y"] = narrow(jaxlike.to_numpy(y.data))
    meta = dict(qconfig=plain(qc), export_qconfig=plain(ex["qconfig"]), dims=dims, x_bits=x.bits, x_exp=x.exp, y_bits=y.bits,
                y_exp=y.exp, inter={}, B=c["B"], L=c["L"], input_scale=c["scale"])
    inter = flat_intermediates(ex["intermediates"])
    for k, v in inter.items():
        meta["inter"][k] = [v.bits, v.exp]
        if small or k.endswith(KEEP.get(name, WIDE_KEEP)):
            arrays[f"inter/{k}"] = narrow(jaxlike.to_numpy(v.data))
    return arrays, meta


# ---------------------------------------------------------------------------------------------------------------------
# qconfig: the reference's load_modeldict / create_fxp_qconfig / add_target_bits_exp on synth.reference_trees
# ---------------------------------------------------------------------------------------------------------------------
QCONFIG_CASES = {
    "shared": dict(bn_scale_bias=False, seed=1919, separate_exponents=False),
    "shared_bnscale": dict(bn_scale_bias=True, seed=7, separate_exponents=False),
    "separate_bnscale": dict(bn_scale_bias=True, seed=7, separate_exponents=True),
}


def unflatten(flat, sep="/"):
    tree = {}
    for k, v in flat.items():
        node = tree
        *head, last = k.split(sep)
        for p in head:
            node = node.setdefault(p, {})
        node[last] = v
    return tree


def record_qconfig(ref, prior=None):
    U = ref.fxputils
    named, meta = {}, {}
    dims = synth.tiny_dims(**_TINY_B)
    for name, c in QCONFIG_CASES.items():
        md = synth.make_float_params(dims, c["seed"], c["bn_scale_bias"])
        stats = {}
        synth.float_forward(md, synth.make_input(2, 64, dims["d_in"], seed=c["seed"] + 1), dims["n_layers"], calibrate_bn=True, stats=stats)
        params, st = synth.reference_trees(md, stats, dims["n_layers"])
        if prior is not None:   # the committed calibration trees (see load_prior)
            trees = unflatten({k: v for k, v in unpack(*[prior[0], prior[1]["index"]]).items() if k.startswith(name + "/")})[name]
            params, st = trees["params"], trees["stats"]
        with tempfile.TemporaryDirectory() as tmp:
            for fname, tree in (("params.pkl", params), ("stats.pkl", st)):
                with open(os.path.join(tmp, fname), "wb") as f:
                    pickle.dump(jaxlike.tree_wrap(tree), f)
            modeldict = U.load_modeldict(os.path.join(tmp, "params.pkl"), os.path.join(tmp, "stats.pkl"))
        if c["separate_exponents"]:
            qc = U.create_fxp_qconfig(modeldict, agg=None)
        else:
            _, qc = U.create_fxp_qconfig(modeldict, agg="max")
        qc = U.add_target_bits_exp(modeldict, qc, synth.W8A16, shared_exp=not c["separate_exponents"])
        for k, v in flatten(params).items():
            named[f"{name}/params/{k}"] = np.asarray(v)
        for k, v in flatten(st).items():
            named[f"{name}/stats/{k}"] = np.asarray(v)
        meta[name] = dict(separate_exponents=c["separate_exponents"], fxp_qconfig=plain(qc))
    arrays, index = pack(named)
    return arrays, dict(cases=meta, index=index)


# ---------------------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------------------
def generate(ref, only=None, fresh=False):
    """{fixture name: (arrays, meta)} for every fixture (or those named in `only`)."""
    prior = (lambda n: None) if fresh else load_prior
    makers = {"ref_ops": lambda: record_ops(ref), "ref_qconfig": lambda: record_qconfig(ref, prior("ref_qconfig"))}
    makers.update({n: (lambda n=n: record_model(ref, n, prior(n))) for n in MODELS})
    return {n: makers[n]() for n in makers if only is None or n in only}


def json_text(meta) -> str:
    return json.dumps(meta, indent=1, sort_keys=True) + "\n"


def member_bytes(arrays):
    """{npz member name: the bytes numpy stores for it}, the compression-independent content of an npz."""
    out = {}
    for k, v in arrays.items():
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
        out[k + ".npy"] = buf.getvalue()
    return out


def file_member_bytes(path):
    with zipfile.ZipFile(path) as z:
        return {n: z.read(n) for n in z.namelist()}


def main(argv=None):
    argv = list(argv or [])
    fresh = "--fresh" in argv
    names = {a for a in argv if a != "--fresh"}
    ref = refload.load()
    for name, (arrays, meta) in generate(ref, only=names or None, fresh=fresh).items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path + ".npz", **arrays)
        with open(path + ".json", "w") as f:
            f.write(json_text(meta))
        print(f"{name}: {os.path.getsize(path + '.npz') // 1024} KiB npz, {len(arrays)} arrays")


if __name__ == "__main__":
    main(sys.argv[1:])
