"""float64 restatements of the float model (sparsernns_amd.synth.float_forward, calibrate_bn=False) for tests/test_float_model.py.

Two kinds: ``forward_f64`` evaluates the whole model in float64 from the float32 parameters and records the same observers;
the ``stage_*`` functions evaluate ONE stage in float64 on given (float32) input planes and return, next to the value, S = the
sum of the absolute values of every product and addend entering each element -- the scale of the forward error bound
|float32 chain - exact| <= (K + 8) * 2^-24 * S of a length-K fma chain with its bias / add terms.
"""
import math

import numpy as np

from sparsernns_amd import synth

F64, C128 = np.float64, np.complex128
U = 2.0 ** -24  # float32 unit roundoff


def zoh64(mixer):
    """The float32 discretisation the model uses (synth.zoh), widened: the PARAMETERS are float32 on every side."""
    lam_bar, B_bar, C = synth.zoh(mixer)
    return lam_bar.astype(C128), B_bar.astype(C128), C.astype(C128)


def inv_std32(var):
    """What the packed blob holds: 1 / sqrt(var + 1e-5) in float32."""
    return (np.float32(1.0) / np.sqrt(var.astype(np.float32) + np.float32(1e-5))).astype(np.float32)


def forward_f64(modeldict, x, n_layers, stats=None):
    def obs(key, v):
        if stats is not None:
            stats[key] = max(stats.get(key, 0.0), float(np.abs(v).max()))

    enc = modeldict["encoder"]
    x = x.astype(F64)
    obs("encoder.inp", x)
    h = x @ enc["encoder"]["kernel"].astype(F64) + enc["encoder"]["bias"].astype(F64)
    obs("encoder.out", h)
    h = np.maximum(h, 0)
    for i in range(n_layers):
        layer = enc[f"layers_{i}"]
        nm = layer["norm"]
        u = (h - nm["mean"].astype(F64)) / np.sqrt(nm["var"].astype(F64) + 1e-5)
        if "scale" in nm:
            u = u * nm["scale"].astype(F64)
        if "bias" in nm:
            u = u + nm["bias"].astype(F64)
        obs(f"l{i}.u", u)
        lam_bar, B_bar, C = zoh64(layer["mixer"])
        Bu = u.astype(C128) @ B_bar.T
        obs(f"l{i}.Bu_re", Bu.real)
        obs(f"l{i}.Bu_im", Bu.imag)
        xs = scan_f64(lam_bar, Bu)
        obs(f"l{i}.x_re", xs.real)
        obs(f"l{i}.x_im", xs.imag)
        xs = np.where((xs.real > 0) | ((xs.real == 0) & (xs.imag > 0)), xs, 0)
        y = 2 * (xs.real @ C.real.T - xs.imag @ C.imag.T) + layer["mixer"]["D"].astype(F64) * u
        obs(f"l{i}.y", y)
        x1 = np.maximum(y, 0)
        obs(f"l{i}.out2.inp", x1)
        g_in = x1 @ layer["out2"]["kernel"].astype(F64) + layer["out2"]["bias"].astype(F64)
        obs(f"l{i}.out2.out", g_in)
        g = 1 / (1 + np.exp(-g_in))
        obs(f"l{i}.gate.l", x1)
        obs(f"l{i}.gate.r", g)
        h = np.maximum(x1 * g + h, 0)
    obs("decoder.inp", h)
    out = h @ modeldict["decoder"]["kernel"].astype(F64) + modeldict["decoder"]["bias"].astype(F64)
    obs("decoder.out", out)
    return out


def scan_f64(lam_bar, Bu):
    """x_t = lambda x_{t-1} + Bu_t from zero, sequentially, in complex128.  Bu (B,L,P)."""
    xs = np.empty(Bu.shape, dtype=C128)
    st = np.zeros((Bu.shape[0], Bu.shape[2]), dtype=C128)
    lam = lam_bar.astype(C128)
    for t in range(Bu.shape[1]):
        st = lam * st + Bu[:, t]
        xs[:, t] = st
    return xs


def max_rel_deviation(stats, ref):
    return max(abs(stats[k] - ref[k]) / ref[k] for k in ref)


# ----------------------------------------------------------------------------------------------------------------------
# one stage at a time: (value, S)
# ----------------------------------------------------------------------------------------------------------------------
def stage_dense(a, w, b):
    a, w, b = a.astype(F64), w.astype(F64), b.astype(F64)
    return a @ w + b, np.abs(a) @ np.abs(w) + np.abs(b)


def stage_u(h, nm):
    h = h.astype(F64)
    istd = inv_std32(nm["var"]).astype(F64)
    sc = nm["scale"].astype(F64) if "scale" in nm else 1.0
    bi = nm["bias"].astype(F64) if "bias" in nm else 0.0
    u = (h - nm["mean"].astype(F64)) * istd * sc + bi
    return u, (np.abs(h) + np.abs(nm["mean"].astype(F64))) * np.abs(istd * sc) + np.abs(bi)


def stage_bu(u, B_bar):
    u = u.astype(F64)
    re, im = B_bar.real.astype(F64).T, B_bar.imag.astype(F64).T
    return (u @ re, np.abs(u) @ np.abs(re)), (u @ im, np.abs(u) @ np.abs(im))


def stage_y(xs_raw, u, C, D):
    """y from the device's raw states (the complex ReLU decided on the float32 values) and the device's u."""
    keep = (xs_raw.real > 0) | ((xs_raw.real == 0) & (xs_raw.imag > 0))
    xr = np.where(keep, xs_raw.real, 0).astype(F64)
    xi = np.where(keep, xs_raw.imag, 0).astype(F64)
    cr, ci, u, D = C.real.astype(F64).T, C.imag.astype(F64).T, u.astype(F64), D.astype(F64)
    y = 2 * (xr @ cr - xi @ ci) + D * u
    return y, 2 * (np.abs(xr) @ np.abs(cr) + np.abs(xi) @ np.abs(ci)) + np.abs(D * u)


def stage_hout(y, g, h):
    x1, g, h = np.maximum(y.astype(F64), 0), g.astype(F64), h.astype(F64)
    return np.maximum(x1 * g + h, 0), np.abs(x1 * g) + np.abs(h)


def sigmoid64(v):
    return 1 / (1 + np.exp(-v.astype(F64)))


def bound(K, S):
    return (K + 8) * U * S


# ----------------------------------------------------------------------------------------------------------------------
# the thresholds of synth.get_intbits / fracbits_from_absmax, as distances in log2
# ----------------------------------------------------------------------------------------------------------------------
def threshold_margin(absmax):
    """Smallest distance in log2 from ``absmax`` to a value where derive_qconfig's integer fields change: an integer
    log2(absmax) (get_intbits), a half-integer log2(absmax / 32767) or log2(absmax / 127) (the round() of fracbits)."""
    l2 = math.log2(absmax)
    d_int = abs(l2 - round(l2))
    out = [d_int]
    for q in (32767.0, 127.0):
        f = math.log2(absmax / q) - 0.5
        out.append(abs(f - round(f)))
    return min(out)
