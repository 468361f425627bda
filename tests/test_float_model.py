"""The float model on the device (sparsernns_amd.floatmodel, csrc/float_model.hpp).

Stage-wise: every stage of the traced forward against a float64 evaluation of THAT stage on the device's own float32 input
planes (float_model_ref.stage_*), inside the forward error bound of a float32 fma chain, (K + 8) * 2^-24 * S -- derived, not
tuned.  Observers: bit for bit the absmax of the device's own planes.  The hot (non-trace) forward must equal the traced one
bit for bit.  End to end: observers against a float64 model within 8x synth.float_forward's own deviation, and the derived
fxp_qconfig identical to the host calibration's.

The stage-wise checks also run where workgroups walk several tiles (WALK below), at every dim_scale: a hazard between two
tiles of a loop, or a slip in its tile indexing, is shared by all six forms of the kernels, so comparing one form with another
cannot see it.  The scan is held per state as well as globally (float_model_ref.per_state_scan).

Measured on the MI355X, largest error / bound per stage over the six WALK cases ((5,3300) at 0.25 .. 1.0, (3,10930) at 0.5 and
1.0): encoder 0.020, u 0.241, Bu 0.107, y 0.109, g_in 0.111, h_out 0.125, decoder 0.117; xs 2.4e-7 max|x| against 1e-5.  Per
state, over all fourteen cases: largest err_dev / (4 err_tree + 1e-6 scale_p) 0.210 ((3,10930) at 1.0), largest
err_dev / err_tree 2.37 ((2,70) at 0.75, on a state where both errors lie under the 1e-6 floor).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import float_model_ref as R
from sparsernns_amd import synth

CASES = [(1, 1, 13), (2, 70, 11), (3, 33, 12)]
DIMS_FOR = {(1, 1, 13): (0.25, 0.5), (2, 70, 11): (0.25, 0.5, 0.75, 1.0), (3, 33, 12): (0.25, 0.5)}
GRID = [(d, c) for c in CASES for d in DIMS_FOR[c]]
IDS = [f"dim{d}-B{c[0]}L{c[1]}" for d, c in GRID]
# Launches are capped at 512 workgroups, each walking 32-frame tiles with a stride of the grid.  (5, 3300): 516 tiles, so
# workgroups 0..3 walk a second tile (the last of them with 20 valid rows), and 7 chunks of the scan; the smallest shape at
# which a tile loop runs twice.  (3, 10930): 1025 tiles, workgroup 0 walks three and its last one is partial.
WALK2, WALK3 = (5, 3300, 14), (3, 10930, 15)
WALK = [(d, WALK2) for d in (0.25, 0.5, 0.75, 1.0)] + [(d, WALK3) for d in (0.5, 1.0)]
STAGE_GRID = GRID + WALK  # the stage-wise checks; the end-to-end ones keep GRID, which their preconditions (MARGIN) are tied to
STAGE_IDS = [f"dim{d}-B{c[0]}L{c[1]}" for d, c in STAGE_GRID]
MARGIN = 2e-4  # log2 distance every host observer keeps from a threshold of derive_qconfig (precondition of qconfig equality)


@functools.lru_cache(maxsize=None)
def model(dim):
    md, qc, dims = synth.make_model(dim)
    return md, qc, dims


def make_x(dim, case):
    return synth.make_input(case[0], case[1], model(dim)[2]["d_in"], seed=case[2])


@functools.lru_cache(maxsize=None)
def host_run(dim, case):
    """(x, y, stats) of synth.float_forward, and the float64 model's observers."""
    md, _, dims = model(dim)
    x = make_x(dim, case)
    st, st64 = {}, {}
    y = synth.float_forward(md, x, dims["n_layers"], stats=st)
    y64 = R.forward_f64(md, x, dims["n_layers"], stats=st64)
    return x, y, st, y64, st64


def yardstick(dim, case):
    """What the device's observers may deviate from float64: 8x the float32 host model's own deviation, floor 1e-5."""
    _, _, st, _, st64 = host_run(dim, case)
    return max(8 * R.max_rel_deviation(st, st64), 1e-5)


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("s5fxp_float_model_blob_bytes s5fxp_float_model_pack s5fxp_float_model_create s5fxp_float_model_destroy "
               "s5fxp_float_workspace_bytes s5fxp_float_trace_bytes s5fxp_float_model_forward").split()


def test_library_exports_the_float_model_entries():
    from sparsernns_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and hasattr(_lib.lib, name), name
    assert _lib.lib.s5fxp_version() == 115


def test_stat_keys_are_float_forwards_order():
    from sparsernns_amd import floatmodel

    _, _, st, _, _ = host_run(0.25, CASES[0])
    assert list(st.keys()) == floatmodel.STAT_KEYS == floatmodel.stat_keys(3) and len(floatmodel.STAT_KEYS) == 34
    assert len(floatmodel.stat_keys(2)) == 24


@pytest.mark.parametrize("dim", [0.25, 1.0])
def test_packed_blob_layout(dim):
    """K = 257 padded to 260 with zero rows, the decoder's columns to 272, every tensor on a 256-byte boundary, inv_std in
    float32, B_bar / C interleaved along P."""
    from sparsernns_amd import floatmodel

    md, _, dims = model(dim)
    H, P = dims["H"], dims["P"]
    blob = floatmodel.pack_blob(md, dims["n_layers"])
    off = 0

    def take(n):
        nonlocal off
        assert off % 64 == 0
        v = blob[off:off + n]
        pad = blob[off + n:(off + n + 63) // 64 * 64]
        assert not pad.any()
        off = (off + n + 63) // 64 * 64
        return v

    enc = md["encoder"]
    w = take(260 * H).reshape(260, H)
    assert np.array_equal(w[:257], enc["encoder"]["kernel"]) and not w[257:].any()
    assert np.array_equal(take(H), enc["encoder"]["bias"])
    for i in range(dims["n_layers"]):
        layer = enc[f"layers_{i}"]
        lam_bar, B_bar, Cc = synth.zoh(layer["mixer"])
        assert np.array_equal(take(H), layer["norm"]["mean"])
        assert np.array_equal(take(H), R.inv_std32(layer["norm"]["var"]))
        assert np.array_equal(take(H), np.ones(H, np.float32)) and not take(H).any()  # no scale / bias in this model
        assert np.array_equal(take(2 * P).view(np.complex64), lam_bar)
        assert np.array_equal(take(H * 2 * P).reshape(H, P, 2).view(np.complex64)[..., 0], B_bar.T)
        cc = take(2 * P * H).reshape(P, 2, H)
        assert np.array_equal(cc[:, 0], Cc.real.T) and np.array_equal(cc[:, 1], -Cc.imag.T)
        assert np.array_equal(take(H), layer["mixer"]["D"])
        assert np.array_equal(take(H * H).reshape(H, H), layer["out2"]["kernel"])
        assert np.array_equal(take(H), layer["out2"]["bias"])
    wd = take(H * 272).reshape(H, 272)
    assert np.array_equal(wd[:, :257], md["decoder"]["kernel"]) and not wd[:, 257:].any()
    bd = take(272)
    assert np.array_equal(bd[:257], md["decoder"]["bias"]) and not bd[257:].any()
    assert off == blob.size


@pytest.mark.parametrize("dim,case", GRID, ids=IDS)
def test_float64_helper_agrees_with_float_forward(dim, case):
    _, y, st, y64, st64 = host_run(dim, case)
    assert set(st) == set(st64)
    dev = R.max_rel_deviation(st, st64)
    print(f"float_forward vs float64: largest relative observer deviation {dev:.3e}")
    assert dev <= 1e-5  # float32 against float64 through three layers; the yardstick's floor
    assert np.abs(y - y64).max() <= 1e-4 * np.abs(y64).max()


@pytest.mark.parametrize("dim,case", GRID, ids=IDS)
def test_host_observers_keep_clear_of_the_qconfig_thresholds(dim, case):
    """The precondition of qconfig equality: asserted, never skipped."""
    _, _, st, _, _ = host_run(dim, case)
    worst = min((R.threshold_margin(v), k) for k, v in st.items())
    print(f"smallest log2 margin {worst[0]:.5f} at {worst[1]}")
    assert worst[0] >= MARGIN, worst


def test_float_engine_without_the_kernels_is_float_forward(monkeypatch):
    import torch
    from sparsernns_amd import floatmodel

    md, _, dims = model(0.25)
    x = synth.make_input(2, 9, dims["d_in"], seed=5)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    eng = floatmodel.FloatEngine(md, dims["n_layers"])
    assert eng.on_device is False
    st, st_ref, act, act_ref = {}, {}, {}, {}
    y = eng.forward(x, stats=st, activations=act)
    ref = synth.float_forward(md, x, dims["n_layers"], stats=st_ref, activations=act_ref)
    assert y.dtype == np.float32 and np.array_equal(y, ref) and st == st_ref

    def same(a, b):
        assert set(a) == set(b)
        for k in a:
            if isinstance(a[k], dict):
                same(a[k], b[k])
            else:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k

    same(act, act_ref)
    # a shape the kernels refuse takes the same route, GPU or not
    tiny = synth.make_float_params(synth.tiny_dims())
    assert not floatmodel.supported(tiny, 2) and floatmodel.supported(md, 3)
    stats, qc = floatmodel.calibrate(md, [x], dims["n_layers"], engine=eng)
    want = synth.derive_qconfig(md, st_ref, dims["n_layers"])
    assert stats == st_ref and qc["encoder"] == synth.cap_result_exponents(want)["encoder"]


def test_fxprun_parser_accepts_the_float_side():
    from sparsernns_amd import fxprun

    ap = fxprun.build_parser()
    assert ap.parse_args(["--synthetic", "--verify"]).float_side == "numpy"
    assert ap.parse_args(["--synthetic", "--verify", "--float-side", "device"]).float_side == "device"
    with pytest.raises(SystemExit):
        ap.parse_args(["--synthetic", "--float-side", "jax"])


def test_c_entries_validate_before_the_device_is_touched():
    from sparsernns_amd import _lib, floatmodel
    from sparsernns_amd._lib import lib

    md, _, dims = model(0.25)
    d = floatmodel._Desc(md, dims["n_layers"])
    nbytes = lib.s5fxp_float_model_blob_bytes(C.byref(d.desc))
    assert nbytes > 0 and nbytes % 256 == 0
    h = C.c_void_p()
    fake = 0x1000  # never dereferenced: every call below fails its argument checks first
    assert lib.s5fxp_float_model_create(C.byref(d.desc), None, nbytes, None, C.byref(h)) == -1
    assert lib.s5fxp_float_model_create(None, fake, nbytes, None, C.byref(h)) == -1
    assert lib.s5fxp_float_model_create(C.byref(d.desc), fake, nbytes, None, None) == -1
    assert lib.s5fxp_float_model_create(C.byref(d.desc), fake, nbytes - 1, None, C.byref(h)) == -5
    d.desc.n_layers = -1
    assert lib.s5fxp_float_model_create(C.byref(d.desc), fake, nbytes, None, C.byref(h)) == -1
    assert lib.s5fxp_float_model_blob_bytes(C.byref(d.desc)) == 0
    d.desc.n_layers = dims["n_layers"]
    d.desc.enc_w = None
    assert lib.s5fxp_float_model_create(C.byref(d.desc), fake, nbytes, None, C.byref(h)) == -1
    t = floatmodel._Desc(synth.make_float_params(synth.tiny_dims(H=8, P=4, d_in=257, d_out=257)), 2)
    assert t.H == 8 and lib.s5fxp_float_model_create(C.byref(t.desc), fake, 1 << 20, None, C.byref(h)) == -3
    assert lib.s5fxp_float_model_blob_bytes(C.byref(t.desc)) == 0
    assert lib.s5fxp_float_model_pack(C.byref(t.desc), fake, 1 << 20) == -3
    assert lib.s5fxp_float_model_forward(None, fake, 1, 1, fake, None, None, fake, 1 << 20, None) == -1
    assert lib.s5fxp_float_workspace_bytes(None, 1, 1, 0) == 0 and lib.s5fxp_float_trace_bytes(None, 1, 1) == 0
    assert h.value is None
    lib.s5fxp_float_model_destroy(None)


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
    t = engine(dim).forward_traced(make_x(dim, case))
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["x"] = make_x(dim, case)
    return out


_traced_small = functools.lru_cache(maxsize=None)(_traced)
_traced_walk = functools.lru_cache(maxsize=1)(_traced)  # hundreds of megabytes each: only the latest is kept


def traced(dim, case):
    """One traced forward per (dim, case), shared and never modified; host copies of every plane, and the input as ``x``."""
    return (_traced_walk if case in (WALK2, WALK3) else _traced_small)(dim, case)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", STAGE_GRID, ids=STAGE_IDS)
def test_every_stage_within_the_float32_chain_bound(dim, case):
    md, _, dims = model(dim)
    t = traced(dim, case)
    R.check_stages(md, dims["n_layers"], t["x"], t)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", STAGE_GRID, ids=STAGE_IDS)
def test_observers_are_the_absmax_of_the_device_planes(dim, case):
    md, _, dims = model(dim)
    t = traced(dim, case)
    R.check_observers(md, dims["n_layers"], t["x"], t)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", STAGE_GRID, ids=STAGE_IDS)
def test_hot_forward_equals_the_traced_forward(dim, case):
    t = traced(dim, case)
    R.check_hot_equals_traced(engine(dim), t["x"], t)


@pytest.mark.gpu
def test_observer_array_semantics():
    import torch

    dim = 0.5
    eng = engine(dim)
    xa = torch.from_numpy(host_run(dim, CASES[1])[0]).to(eng.device)
    xb = torch.from_numpy(host_run(dim, CASES[2])[0]).to(eng.device)
    sa, sb, both = eng.new_stats(), eng.new_stats(), eng.new_stats()
    eng.forward_device(xa, sa)
    eng.forward_device(xb, sb)
    eng.forward_device(xa, both)
    eng.forward_device(xb, both)
    assert torch.equal(both, torch.maximum(sa, sb)) and not torch.equal(sa, sb)
    # the entry only raises: a sentinel above every observer survives, and the guard word behind the array is never written
    guard = torch.full((len(eng.keys) + 1,), 1e30, dtype=torch.float32, device=eng.device)
    guard[-1] = -123.0
    eng.forward_device(xa, guard[:-1])
    assert torch.equal(guard[:-1], torch.full_like(guard[:-1], 1e30)) and float(guard[-1]) == -123.0
    guard[:-1] = 0
    eng.forward_device(xa, guard[:-1])
    assert torch.equal(guard[:-1], sa) and float(guard[-1]) == -123.0
    # one NaN in the input reaches encoder.inp as NaN
    xn = xa.clone()
    xn[1, 7, 100] = float("nan")
    sn = eng.new_stats()
    eng.forward_device(xn, sn)
    assert bool(torch.isnan(sn[0]))
    # the forward entry's own argument checks, on a live handle: nothing is launched
    from sparsernns_amd._lib import lib
    B, L = xa.shape[:2]
    need = lib.s5fxp_float_workspace_bytes(eng._h, B, L, 0)
    assert need == 4 * (2 * B * L * eng.H + 4 * B * L * eng.P) < lib.s5fxp_float_workspace_bytes(eng._h, B, L, 1)
    assert lib.s5fxp_float_trace_bytes(eng._h, B, L) == 4 * 3 * 5 * B * L * eng.H
    ws, y = torch.empty(need // 4, device=eng.device), torch.full_like(xa, 7.0)
    args = lambda b, l, w, n: (eng._h, xa.data_ptr(), b, l, y.data_ptr(), None, None, w, n, None)
    assert lib.s5fxp_float_model_forward(*args(0, L, ws.data_ptr(), need)) == -1
    assert lib.s5fxp_float_model_forward(*args(B, -1, ws.data_ptr(), need)) == -1
    assert lib.s5fxp_float_model_forward(*args(B, L, None, need)) == -1
    assert lib.s5fxp_float_model_forward(*args(B, L, ws.data_ptr(), need - 1)) == -5
    assert lib.s5fxp_float_workspace_bytes(eng._h, 0, L, 0) == 0
    assert bool((y == 7.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", GRID, ids=IDS)
def test_observers_against_float64_within_the_float32_yardstick(dim, case):
    from sparsernns_amd import floatmodel

    _, _, st, _, st64 = host_run(dim, case)
    got = {k: float(v) for k, v in zip(floatmodel.STAT_KEYS, traced(dim, case)["stats"])}
    dev, host = R.max_rel_deviation(got, st64), R.max_rel_deviation(st, st64)
    print(f"largest relative observer deviation from float64: device {dev:.3e}, float_forward {host:.3e}")
    assert dev <= yardstick(dim, case)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,case", GRID, ids=IDS)
def test_calibrate_gives_the_host_qconfig_and_a_working_engine(dim, case):
    import torch
    from sparsernns_amd import _lib, floatmodel
    from sparsernns_amd.fxpmodel import build_regression_model

    md, _, dims = model(dim)
    x, _, st, _, _ = host_run(dim, case)
    assert min(R.threshold_margin(v) for v in st.values()) >= MARGIN  # the precondition, asserted here too
    stats, qc = floatmodel.calibrate(md, [x], dims["n_layers"], engine=engine(dim))
    want = synth.cap_result_exponents(synth.derive_qconfig(md, st, dims["n_layers"]))

    def ints(a, b, path=""):
        assert set(a) == set(b), path
        for k in a:
            if isinstance(a[k], dict):
                ints(a[k], b[k], f"{path}.{k}")
            elif isinstance(a[k], (int, np.integer)):
                assert a[k] == b[k], (f"{path}.{k}", a[k], b[k])

    ints(qc, want)
    eng = build_regression_model(md, qc, dims["n_layers"]).engine()
    y = eng.forward_float(torch.from_numpy(x).to(eng.device), qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"])
    status = eng.check_status()
    assert y.shape == x.shape and not int(status[0]) & _lib.ST_REDO


@pytest.mark.gpu
def test_forward_mirrors_float_forward_in_keys_and_dtypes():
    """stats by maximum under float_forward's keys; activations = sequence 0 of the traced planes under the reference's keys."""
    dim, case = 0.5, CASES[2]
    md, _, dims = model(dim)
    x, y_ref, st_ref, _, _ = host_run(dim, case)
    t = traced(dim, case)
    eng = engine(dim)
    st, act, act_ref = {"l0.u": 1e9, "decoder.out": 0.0}, {}, {}
    y = eng.forward(x, stats=st, activations=act)
    synth.float_forward(md, x[:1], dims["n_layers"], activations=act_ref)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and np.array_equal(y, t["out"])
    assert set(st) == set(st_ref) and st["l0.u"] == 1e9 and st["decoder.out"] == float(t["stats"][-1])

    def same_tree(a, b, path=""):
        assert set(a) == set(b), path
        for k in a:
            if isinstance(a[k], dict):
                same_tree(a[k], b[k], f"{path}/{k}")
            else:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f"{path}/{k}"

    same_tree(act, act_ref)
    for i in range(dims["n_layers"]):
        a = act["encoder"][f"layers_{i}"]
        xs = t[f"l{i}.xs"][0]
        keep = (xs.real > 0) | ((xs.real == 0) & (xs.imag > 0))
        assert np.array_equal(a["pre_C"], np.where(keep, xs, 0)) and np.array_equal(a["pre_s5"], t[f"l{i}.u"][0])
        assert np.array_equal(a["pre_GLU"], t[f"l{i}.y"][0]) and np.array_equal(a["mixer"]["__call__"], t[f"l{i}.y"][0])
        assert np.array_equal(a["out2"]["__call__"], t[f"l{i}.g_in"][0]) and np.array_equal(a["__call__"], t[f"l{i}.h_out"][0])
        assert np.array_equal(a["input"], (t["h_enc"] if i == 0 else t[f"l{i - 1}.h_out"])[0])
        assert np.array_equal(a["post_GLU"], np.maximum(t[f"l{i}.y"][0], 0) * t[f"l{i}.g"][0])
        assert np.array_equal(a["mixer"]["B_bar"], act_ref["encoder"][f"layers_{i}"]["mixer"]["B_bar"])
    assert np.array_equal(act["__call__"], t["out"][0])
    # a tensor in, a tensor out, on the caller's device
    import torch
    assert torch.equal(eng.forward(torch.from_numpy(x)), torch.from_numpy(t["out"]))


@pytest.mark.gpu
def test_audio_wrappers_equal_their_hand_composed_chains():
    import torch
    from sparsernns_amd import audio

    eng = engine(0.5)
    rng = np.random.default_rng(4)
    T = 512 + 128 * 9
    noisy = torch.from_numpy((0.05 * rng.standard_normal((2, T))).astype(np.float32)).to(eng.device)
    clean = torch.from_numpy((0.05 * rng.standard_normal((2, T))).astype(np.float32)).to(eng.device)
    x = audio.stft_mag(noisy)
    mask = eng.forward(x)
    cleaned, cm = audio.mask_istft(noisy, mask, cleaned_mag=True)
    got = audio.denoise_float(eng, noisy)
    for a, b in zip(got, (cleaned, cm, x, mask)):
        assert torch.equal(a, b)
    loss, snr = audio.validate_float(eng, noisy, clean, lam=0.001)
    wl, ws, _ = audio.score_fused(noisy, clean, mask, 0.001)
    assert torch.equal(loss, wl) and torch.equal(snr, ws)
