"""Float models from outside the one recipe (synth.make_model with its defaults) the float tests draw from.

``s5fxp_float_model_create`` takes any BatchNorm scale / bias, 1..64 layers and whatever poles, gates and variances the
float tree holds; the recipe fills a corner of that: scale 1 and bias 0, three layers, |lambda_bar| in [0.95, 0.9995], every
state live, gates far from saturation.  Every model here is made in float space, by editing the tree
``synth.make_float_params`` returns, so the host forward (synth.float_forward), the float64 restatement
(float_model_ref.forward_f64) and the device (floatmodel.FloatEngine) all start from the same float32 tree.

Builders (``BUILDERS``):
  bn_scale_bias   -- BatchNorm scale in +-[0.5, 1.5], one in ten negative, and a bias
  layers_1/2/4    -- both parities of the layer ping-pong and one depth above the recipe's
  poles           -- per layer every 8th state with |lambda_bar| >= 0.9999, the next with |lambda_bar| <= 0.1, the next dead
  saturated_gate  -- out2.bias at +-150 in chosen columns (the sigmoid at both ends, expf overflowing at the lower one), D
                     negative in some channels and zero in others, norm.var = 0 in one channel
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np

from sparsernns_amd import synth

F32 = np.float32
INPUT_SCALE = 300.0  # the BatchNorm statistics are as drawn, not calibrated: the input the suite's 8-bit recipes use with them
SHAPES = [(2, 70, 11), (3, 33, 12)]  # (B, L, seed): test_float_model.py's two multi-tile shapes

SLOW, FAST, DEAD = 0, 1, 2  # p % 8 of the states the poles builder edits
SLOW_STEP, FAST_RE, FAST_STEP = 1e-4, -30.0, 0.1  # |lambda_bar| = exp(Lambda_re * step): exp(-0.5e-4), exp(-3)
GATE_BIAS = 150.0
HI_COLS, LO_COLS = (0, 17, -1), (1, 16, -2)  # out2 columns driven to g = 1 / g = 0, in the first and the last column tile
NEG_D, ZERO_D, VAR0 = slice(2, None, 7), slice(3, None, 7), 5


class Model:
    def __init__(self, name: str, md: dict, dims: dict, **meta):
        self.name, self.md, self.dims, self.meta = name, md, dims, meta
        self.n_layers = dims["n_layers"]

    def layers(self):
        return [self.md["encoder"][f"layers_{i}"] for i in range(self.n_layers)]

    def x(self, case):
        return synth.make_input(case[0], case[1], self.dims["d_in"], seed=case[2], scale=INPUT_SCALE)


def _dims(ds: float, **over) -> dict:
    d = synth.ndns_dims(ds)
    d.update(over)
    return d


def bn_scale_bias(ds: float) -> Model:
    dims = _dims(ds)
    return Model(f"bn_scale_bias_ds{ds}", synth.make_float_params(dims, 1919, bn_scale_bias=True), dims)


def layers(n: int, ds: float = 0.25) -> Model:
    dims = _dims(ds, n_layers=n)
    return Model(f"layers_{n}_ds{ds}", synth.make_float_params(dims, 1919), dims)


def poles(ds: float) -> Model:
    dims = _dims(ds)
    m = Model(f"poles_ds{ds}", synth.make_float_params(dims, 1919), dims)
    p = np.arange(dims["P"])
    for layer in m.layers():
        mx = layer["mixer"]
        slow, fast, dead = p % 8 == SLOW, p % 8 == FAST, p % 8 == DEAD
        mx["log_step"][slow, 0] = math.log(SLOW_STEP)
        mx["B"][slow] *= F32(1e2)  # B_bar is about step * B: keeps the slow states' drive of the order of the others'
        mx["Lambda_re"][fast] = FAST_RE
        mx["log_step"][fast, 0] = math.log(FAST_STEP)
        mx["B"][dead] = 0
    return m


def saturated_gate(ds: float) -> Model:
    dims = _dims(ds)
    m = Model(f"saturated_gate_ds{ds}", synth.make_float_params(dims, 1919), dims)
    for layer in m.layers():
        b = layer["out2"]["bias"]
        b[list(HI_COLS)], b[list(LO_COLS)] = GATE_BIAS, -GATE_BIAS
        D = layer["mixer"]["D"]
        D[NEG_D] = -np.abs(D[NEG_D]) - F32(0.5)
        D[ZERO_D] = 0
        layer["norm"]["var"][VAR0] = 0
    return m


BUILDERS = {}
for _ds in (0.25, 1.0):
    BUILDERS[f"bn_scale_bias_ds{_ds}"] = (bn_scale_bias, (_ds,))
    BUILDERS[f"poles_ds{_ds}"] = (poles, (_ds,))
    BUILDERS[f"saturated_gate_ds{_ds}"] = (saturated_gate, (_ds,))
for _n in (1, 2, 4):
    BUILDERS[f"layers_{_n}_ds0.25"] = (layers, (_n,))
NAMES = sorted(BUILDERS)
CALIBRATED = [n for n in NAMES if n.startswith(("bn_scale_bias", "layers_1"))]  # these also calibrate and fake-quantise

_CACHE: Dict[str, Model] = {}


def model(name: str) -> Model:
    """The contract model ``name`` (built once per process, never modified)."""
    if name not in _CACHE:
        fn, args = BUILDERS[name]
        _CACHE[name] = fn(*args)
    return _CACHE[name]
