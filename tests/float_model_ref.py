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


def forward_f64(modeldict, x, n_layers, stats=None, planes=None):
    """``planes``: a dict that receives every observed float64 tensor itself under its observer's key."""
    def obs(key, v):
        if stats is not None:
            stats[key] = max(stats.get(key, 0.0), float(np.abs(v).max()))
        if planes is not None:
            planes[key] = v

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


def tree_scan(lam_bar, Bu, reverse=False):
    """oracle.float_ssm.associative_scan (complex64), the oracle's restatement of the reference's own combination tree,
    sequence by sequence on the same lambda and Bu.  Bu (B,L,P)."""
    from oracle import float_ssm

    A = np.broadcast_to(lam_bar.astype(np.complex64), Bu.shape[1:])
    return np.stack([float_ssm.associative_scan((A, Bu[b].astype(np.complex64)), reverse=reverse)[1] for b in range(Bu.shape[0])])


def per_state_errors(xs, ref):
    """(max over b, t of |xs - ref|, max over b, t of |ref|), one value per state.  xs, ref (B,L,P)."""
    return np.abs(xs - ref).max(axis=(0, 1)), np.abs(ref).max(axis=(0, 1))


def per_state_scan(xs_dev, ref, tree, what):
    """The per-state scan criterion: for every state p, with scale_p = max |ref[.., p]|,
        max |xs_dev - ref|[.., p] <= 4 max |tree - ref|[.., p] + 1e-6 scale_p.
    The measure is the reference's tree, not the code under test; the margin of 4 and the 1e-6 floor are what
    test_float_scan.py grants the stand-alone scan globally.  A maximum over all states would let a slow state's magnitude
    hide a fast state's error.  Returns the largest err_dev / err_tree over the states where the tree errs at all."""
    err_dev, scale = per_state_errors(xs_dev, ref)
    err_tree, _ = per_state_errors(tree, ref)
    lim = 4 * err_tree + 1e-6 * scale
    worst = float((err_dev / np.maximum(lim, 1e-300)).max())
    some = err_tree > 0
    ratio = float((err_dev[some] / err_tree[some]).max()) if some.any() else 0.0
    print(f"{what}: per state worst err / limit {worst:.3f}, largest err_dev / err_tree {ratio:.3f}")
    bad = np.flatnonzero(err_dev > lim)
    assert bad.size == 0, (what, bad[:8].tolist(), err_dev[bad[:8]].tolist(), err_tree[bad[:8]].tolist(), scale[bad[:8]].tolist())
    return ratio


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


# ----------------------------------------------------------------------------------------------------------------------
# the checks of one traced device forward, shared by test_float_model.py and test_float_contract.py
# ----------------------------------------------------------------------------------------------------------------------
def within(dev, ref, K, S, what):
    err = np.abs(dev.astype(F64) - ref)
    lim = bound(K, S)
    worst = float((err / np.maximum(lim, 1e-300)).max())
    print(f"{what}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
    assert (err <= lim).all(), (what, float(err.max()), worst)


def check_stages(md, n_layers, x, t, global_scan=True):
    """Every stage of the traced forward ``t`` (host copies of FloatEngine.forward_traced's planes) of model ``md`` on input
    ``x`` against a float64 evaluation of that stage on the device's own float32 input planes: the chain bound per stage,
    the sigmoid within 1e-6, the scan within 1e-5 max|x| (``global_scan``) and within the per-state criterion."""
    enc = md["encoder"]
    H = enc["encoder"]["kernel"].shape[1]
    P = enc["layers_0"]["mixer"]["Lambda_re"].shape[0]
    v, S = stage_dense(x, enc["encoder"]["kernel"], enc["encoder"]["bias"])
    within(t["h_enc"], np.maximum(v, 0), 257, S, "encoder")
    h = t["h_enc"]
    for i in range(n_layers):
        layer = enc[f"layers_{i}"]
        lam_bar, B_bar, Cc = synth.zoh(layer["mixer"])
        u, y, g_in, g, h_out = (t[f"l{i}.{k}"] for k in ("u", "y", "g_in", "g", "h_out"))
        Bu, xs = t[f"l{i}.Bu"], t[f"l{i}.xs"]
        v, S = stage_u(h, layer["norm"])
        within(u, v, 0, S, f"l{i}.u")
        (vr, Sr), (vi, Si) = stage_bu(u, B_bar)
        within(Bu.real, vr, H, Sr, f"l{i}.Bu_re")
        within(Bu.imag, vi, H, Si, f"l{i}.Bu_im")
        ref = scan_f64(lam_bar, Bu)
        err, scale = np.abs(xs - ref).max(), np.abs(ref).max()
        print(f"l{i}.xs: max err {err:.3e} of max|x| {scale:.3e}")
        if global_scan:
            assert err <= 1e-5 * scale
        per_state_scan(xs, ref, tree_scan(lam_bar, Bu), f"l{i}.xs")
        v, S = stage_y(xs, u, Cc, layer["mixer"]["D"])
        within(y, v, P, S, f"l{i}.y")
        v, S = stage_dense(np.maximum(y, 0), layer["out2"]["kernel"], layer["out2"]["bias"])
        within(g_in, v, H, S, f"l{i}.g_in")
        gerr = np.abs(g - sigmoid64(g_in)).max()
        print(f"l{i}.g: max err {gerr:.3e}")
        assert gerr <= 1e-6
        v, S = stage_hout(y, g, h)
        within(h_out, v, 0, S, f"l{i}.h_out")
        h = h_out
    v, S = stage_dense(h, md["decoder"]["kernel"], md["decoder"]["bias"])
    within(t["out"], v, H, S, "decoder")


def check_observers(md, n_layers, x, t):
    """The observers of the traced forward ``t``: bit for bit the absmax of the device's own planes."""
    from sparsernns_amd import floatmodel

    want = {"encoder.inp": x, "decoder.inp": t[f"l{n_layers - 1}.h_out"], "decoder.out": t["out"]}
    for i in range(n_layers):
        x1 = np.maximum(t[f"l{i}.y"], 0)
        want.update({f"l{i}.u": t[f"l{i}.u"], f"l{i}.Bu_re": t[f"l{i}.Bu"].real, f"l{i}.Bu_im": t[f"l{i}.Bu"].imag,
                     f"l{i}.x_re": t[f"l{i}.xs"].real, f"l{i}.x_im": t[f"l{i}.xs"].imag, f"l{i}.y": t[f"l{i}.y"],
                     f"l{i}.out2.inp": x1, f"l{i}.out2.out": t[f"l{i}.g_in"], f"l{i}.gate.l": x1, f"l{i}.gate.r": t[f"l{i}.g"]})
    keys = floatmodel.stat_keys(n_layers)
    assert len(keys) == len(t["stats"])
    got = dict(zip(keys, t["stats"]))
    for k, plane in want.items():
        assert got[k].view(np.uint32) == np.abs(plane).max().astype(np.float32).view(np.uint32), k
    # encoder.out is observed before the ReLU and the stored plane has it behind it: no device plane to take the absmax of.
    # It must cover the stored plane and lie within the encoder's chain bound of the float64 stage's absmax.
    v, S = stage_dense(x, md["encoder"]["encoder"]["kernel"], md["encoder"]["encoder"]["bias"])
    assert set(got) == set(want) | {"encoder.out"} and got["encoder.out"] >= t["h_enc"].max()
    assert abs(float(got["encoder.out"]) - np.abs(v).max()) <= bound(257, S).max()


def check_hot_equals_traced(eng, x, t):
    """The hot (non-trace) forward: output and observers bit for bit the traced ones; a NULL stats array leaves y unchanged."""
    import torch

    xd = torch.from_numpy(x).to(eng.device)
    st = eng.new_stats()
    y = eng.forward_device(xd, st)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), t["out"].view(np.uint32))
    assert np.array_equal(st.cpu().numpy().view(np.uint32), t["stats"].view(np.uint32))
    assert torch.equal(eng.forward_device(xd, None), y)
