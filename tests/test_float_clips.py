"""The float model over clips of different lengths in one launch set: ``s5fxp_float_model_clips``,
``FloatEngine.forward_clips[_device]``, clip pairs in ``calibrate[_clipped]``, ``audio.denoise_float_clips / validate_float_clips``.

The reference of every device test is the device's OWN rectangular forward on each clip alone, ``forward_device(x[e:e+1, :len_e])``:
outputs, observers and histograms of the clip launch must equal it bit for bit and integer for integer, whatever the padding
rows hold.  No tolerance appears anywhere in this file.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from sparsernns_amd import synth

SENT32 = 0x7FC0DEAD  # a NaN bit pattern no kernel produces
SENT64 = -0x0123456789ABCDEF
GUARD = 64  # words either side of y, stats and hist


def _set_d():
    lens = np.random.default_rng(23).integers(0, 449, size=40)
    lens[3], lens[17] = 0, 448
    return [int(v) for v in lens]


# name -> (Lmax, lens): the smallest sets at which the tile mapping can go wrong
SETS = {
    "A": (70, [70, 1, 0, 33, 32]),  # full clip, one frame, empty, one row into a second tile + a skipped third, an exact tile
    "B": (40, [100, -3]),            # clamped to 40 and 0
    "C": (520, [513, 512]),          # either side of the scan's 512-step chunk
    "D": (448, _set_d()),            # 40 x 14 = 560 tiles on at most 512 workgroups
}
SEEDS = {"A": 41, "B": 42, "C": 43, "D": 44}
GRID = [(0.25, "A"), (0.5, "A"), (0.75, "A"), (1.0, "A"), (0.25, "B"), (0.25, "C"), (0.25, "D"),
        # workgroups that walk several tiles (D), and the scan's chunk carry (C), in the other instantiations of every kernel
        (0.5, "D"), (0.75, "D"), (1.0, "D"), (1.0, "C")]
IDS = [f"dim{d}-{s}" for d, s in GRID]
CPU_LENS, CPU_LMAX = [1, 33, 70], 70
P_CLIP = 1e-3


def clamped(name):
    Lmax, lens = SETS[name]
    return [min(max(v, 0), Lmax) for v in lens]


@functools.lru_cache(maxsize=None)
def model(dim):
    return synth.make_model(dim)


def element_counts(dims, N):
    from sparsernns_amd import floatmodel

    out = {}
    for k in floatmodel.stat_keys(dims["n_layers"]):
        last = k.split(".")[-1]
        out[k] = N * (257 if k in ("encoder.inp", "decoder.out") else dims["P"] if last in ("Bu_re", "Bu_im", "x_re", "x_im")
                      else dims["H"])
    return out


def same_ints(a, b, path=""):
    assert set(a) == set(b), path
    for k in a:
        if isinstance(a[k], dict):
            same_ints(a[k], b[k], f"{path}.{k}")
        elif isinstance(a[k], (int, np.integer)):
            assert a[k] == b[k], (f"{path}.{k}", a[k], b[k])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_clip_entry_and_keeps_its_version():
    import os
    from sparsernns_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    name = "s5fxp_float_model_clips"
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and hasattr(_lib.lib, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s5fxp.h")).read()
    assert f"int {name}(const s5fxp_float_model *m, const float *x, int n, int Lmax, const int32_t *lens" in header
    assert _lib.lib.s5fxp_version() == 115


def test_null_model_and_empty_launch_are_bad_arguments():
    from sparsernns_amd import _lib

    fake = 0x1000  # never dereferenced: the argument checks fail first
    call = _lib.lib.s5fxp_float_model_clips
    assert call(None, fake, 1, 1, fake, fake, None, None, fake, 1 << 20, None) == _lib.S5FXP_EBADARG
    assert call(fake, fake, 0, 1, fake, fake, None, None, fake, 1 << 20, None) == _lib.S5FXP_EBADARG
    assert call(fake, fake, 1, 0, fake, fake, None, None, fake, 1 << 20, None) == _lib.S5FXP_EBADARG
    assert call(fake, fake, 1, 1, None, fake, None, None, fake, 1 << 20, None) == _lib.S5FXP_EBADARG


@functools.lru_cache(maxsize=None)
def host_clips(dim):
    """(x padded with zeros, per-clip (y, stats, hist) of synth.float_forward on each clip alone); shared, never modified."""
    md, _, dims = model(dim)
    x = synth.make_input(len(CPU_LENS), CPU_LMAX, dims["d_in"], seed=31).copy()
    per = []
    for e, n in enumerate(CPU_LENS):
        x[e, n:] = 0
        st, h = {}, {}
        y = synth.float_forward(md, x[e:e + 1, :n], dims["n_layers"], stats=st, hist=h)
        per.append((y[0], st, h))
    return x, per


def test_host_forward_clips_is_the_per_clip_forward(monkeypatch):
    import torch
    from sparsernns_amd import floatmodel

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dim = 0.25
    md, _, dims = model(dim)
    x, per = host_clips(dim)
    eng = floatmodel.FloatEngine(md, dims["n_layers"])
    assert not eng.on_device
    st, hist = {}, {}
    ys = eng.forward_clips([x[e, :n] for e, n in enumerate(CPU_LENS)], stats=st, hist=hist)
    assert len(ys) == len(CPU_LENS)
    for y, (want, _, _), n in zip(ys, per, CPU_LENS):
        assert isinstance(y, np.ndarray) and y.shape == (n, 257) and np.array_equal(bits(y), bits(want))
    assert list(st) == eng.keys == list(hist)
    for k in eng.keys:
        assert st[k] == max(p[1][k] for p in per), k
        assert np.array_equal(hist[k], sum(p[2][k] for p in per)), k
    # tensors in, tensors out; dicts that hold something are updated, not replaced
    st2, h2 = {"l0.u": 1e30}, {"l0.u": np.ones(64, dtype=np.int64)}
    yt = eng.forward_clips([torch.from_numpy(x[e, :n]) for e, n in enumerate(CPU_LENS)], stats=st2, hist=h2)
    assert all(isinstance(t, torch.Tensor) and np.array_equal(bits(t.numpy()), bits(p[0])) for t, p in zip(yt, per))
    assert st2["l0.u"] == 1e30 and st2["l0.y"] == st["l0.y"] and np.array_equal(h2["l0.u"], hist["l0.u"] + 1)
    assert eng.forward_clips([]) == []
    with pytest.raises(ValueError):
        eng.forward_clips([x[0, :3, :100]])
    with pytest.raises(RuntimeError):
        eng.forward_clips_device(torch.from_numpy(x), torch.tensor(CPU_LENS, dtype=torch.int32))


@pytest.mark.parametrize("lens_kind", ["list", "array", "tensor"])
def test_host_calibration_from_a_clip_pair_is_the_calibration_from_single_clips(monkeypatch, lens_kind):
    import torch
    from sparsernns_amd import floatmodel

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dim = 0.25
    md, _, dims = model(dim)
    x, _ = host_clips(dim)
    xp = x.copy()
    for e, n in enumerate(CPU_LENS):
        xp[e, n:] = np.nan  # what the padding holds is never looked at
    lens = {"list": list(CPU_LENS), "array": np.array(CPU_LENS, dtype=np.int64), "tensor": torch.tensor(CPU_LENS, dtype=torch.int32)}[lens_kind]
    singles = [x[e:e + 1, :n] for e, n in enumerate(CPU_LENS)]
    s0, q0 = floatmodel.calibrate(md, singles, dims["n_layers"])
    s1, q1 = floatmodel.calibrate(md, [(xp, lens)], dims["n_layers"])
    assert s1 == s0
    same_ints(q1, q0)
    a = floatmodel.calibrate_clipped(md, singles, dims["n_layers"], P_CLIP)
    b = floatmodel.calibrate_clipped(md, [(xp, lens)], dims["n_layers"], P_CLIP)
    assert b[0] == a[0] and b[2] == a[2] and all(np.array_equal(b[1][k], a[1][k]) for k in a[1])
    same_ints(b[3], a[3])
    # both kinds of item in one run
    c = floatmodel.calibrate_clipped(md, [(xp, lens), x[:1]], dims["n_layers"], P_CLIP)
    d = floatmodel.calibrate_clipped(md, singles + [x[:1]], dims["n_layers"], P_CLIP)
    assert c[0] == d[0] and all(np.array_equal(c[1][k], d[1][k]) for k in d[1])
    same_ints(c[3], d[3])


def test_padding_a_batch_inflates_every_histogram_by_the_padding(monkeypatch):
    """What the feature is for: the rectangular route on a zero-padded batch counts (n Lmax - sum len) frames that do not exist."""
    import torch
    from sparsernns_amd import floatmodel

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dim = 0.25
    md, _, dims = model(dim)
    x, _ = host_clips(dim)
    _, h_pad, _, _ = floatmodel.calibrate_clipped(md, [x], dims["n_layers"], P_CLIP)
    _, h_clip, _, _ = floatmodel.calibrate_clipped(md, [(x, CPU_LENS)], dims["n_layers"], P_CLIP)
    pad = len(CPU_LENS) * CPU_LMAX - sum(CPU_LENS)
    width = element_counts(dims, 1)
    assert pad == 106
    for k in h_pad:
        assert int(h_clip[k].sum()) == sum(CPU_LENS) * width[k], k
        assert int(h_pad[k].sum()) - int(h_clip[k].sum()) == pad * width[k], k


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


def guarded(eng, words, dtype, sentinel, fill=None):
    """(whole buffer, the `words` in its middle): GUARD sentinel words either side; the middle holds `fill` or the sentinel."""
    import torch

    buf = torch.full((words + 2 * GUARD,), sentinel, dtype=dtype, device=eng.device)
    if fill is not None:
        buf[GUARD:-GUARD] = fill
    return buf, buf[GUARD:-GUARD]


def guards_intact(buf, sentinel):
    g = buf.cpu().numpy()
    return bool((g[:GUARD] == sentinel).all() and (g[-GUARD:] == sentinel).all())


@functools.lru_cache(maxsize=None)
def clip_run(dim, name):
    """One clip launch per (dim, set) with NaN in every padding row of x, a sentinel in every word of y, guard words round y,
    stats and hist -- and the rectangular forward of every clip alone.  Host copies; shared and never modified."""
    import torch

    eng = engine(dim)
    Lmax, lens = SETS[name]
    eff, n = clamped(name), len(lens)
    x = synth.make_input(n, Lmax, 257, seed=SEEDS[name]).copy()
    for e in range(n):
        x[e, eff[e]:] = 0
    xz = torch.from_numpy(x).to(eng.device)
    xn = xz.clone()
    for e in range(n):
        xn[e, eff[e]:] = float("nan")
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=eng.device)
    nk = len(eng.keys)
    ybuf, y = guarded(eng, n * Lmax * 257, torch.int32, SENT32)
    sbuf, st = guarded(eng, nk, torch.int32, SENT32, 0)
    hbuf, hd = guarded(eng, nk * 64, torch.int64, SENT64, 0)
    y = y.view(torch.float32).view(n, Lmax, 257)
    got = eng.forward_clips_device(xn, lens_dev, st.view(torch.float32), hd, out=y)
    assert got.data_ptr() == y.data_ptr()
    per = []
    for e in range(n):
        if not eff[e]:
            per.append(None)
            continue
        se, he = eng.new_stats(), eng.new_hist()
        ye = eng.forward_device(xz[e:e + 1, :eff[e]].contiguous(), se, hist_dev=he)
        per.append((ye[0].cpu().numpy(), se.cpu().numpy().view(np.uint32), he.cpu().numpy()))
    torch.cuda.synchronize()
    return dict(xz=xz, xn=xn, lens=lens_dev, eff=eff, per=per, y=y.cpu().numpy(), st=st.cpu().numpy().view(np.uint32),
                hist=hd.cpu().numpy().reshape(nk, 64), guards=[guards_intact(b, s) for b, s in
                                                              ((ybuf, SENT32), (sbuf, SENT32), (hbuf, SENT64))])


@pytest.mark.gpu
@pytest.mark.parametrize("dim,name", GRID, ids=IDS)
def test_every_clip_is_its_own_forward_and_padding_is_never_written(dim, name):
    r = clip_run(dim, name)
    y = r["y"].view(np.uint32)
    for e, (n, p) in enumerate(zip(r["eff"], r["per"])):
        if n:
            assert np.array_equal(y[e, :n], bits(p[0])), (e, n, np.count_nonzero(y[e, :n] != bits(p[0])))
        assert (y[e, n:] == np.uint32(SENT32)).all(), (e, n)
    assert r["guards"] == [True, True, True]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,name", GRID, ids=IDS)
def test_observers_and_histograms_are_those_of_the_clips_alone(dim, name):
    from sparsernns_amd import floatmodel

    r = clip_run(dim, name)
    _, _, dims = model(dim)
    live = [p for p in r["per"] if p is not None]
    # stats: bitwise the elementwise maximum (non-negative floats order like their bits); no NaN from the NaN padding
    assert np.array_equal(r["st"], np.maximum.reduce([p[1] for p in live]))
    assert not np.isnan(r["st"].view(np.float32)).any()
    # hist: integer for integer the sum; every row counts sum(len) frames; nothing of the NaN padding in bin 63
    assert np.array_equal(r["hist"], sum(p[2] for p in live))
    counts = element_counts(dims, sum(r["eff"]))
    keys = floatmodel.stat_keys(dims["n_layers"])
    assert [int(row.sum()) for row in r["hist"]] == [counts[k] for k in keys]
    assert r["hist"][keys.index("encoder.inp")][63] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dim,name", GRID, ids=IDS)
def test_array_semantics_and_independence_of_padding_and_hist(dim, name):
    import torch

    eng, r = engine(dim), clip_run(dim, name)
    y0 = torch.from_numpy(r["y"]).to(eng.device).view(torch.int32)
    st0 = torch.from_numpy(r["st"].view(np.int32)).to(eng.device)
    h0 = torch.from_numpy(r["hist"]).to(eng.device)
    valid = torch.zeros(y0.shape[:2], dtype=torch.bool, device=eng.device)
    for e, n in enumerate(r["eff"]):
        valid[e, :n] = True
    sent = lambda: torch.full(y0.shape, SENT32, dtype=torch.int32, device=eng.device).view(torch.float32)
    # zero padding instead of NaN padding: the same valid outputs, observers and histograms
    ya, sa, ha = sent(), eng.new_stats(), eng.new_hist()
    eng.forward_clips_device(r["xz"], r["lens"], sa, ha, out=ya)
    assert torch.equal(ya.view(torch.int32), y0) and torch.equal(sa.view(torch.int32), st0) and torch.equal(ha, h0)
    # without hist: y and stats bit-identical; a second launch into the first one's histogram gives the sum
    yb, sb = sent(), eng.new_stats()
    eng.forward_clips_device(r["xn"], r["lens"], sb, None, out=yb)
    assert torch.equal(yb.view(torch.int32), y0) and torch.equal(sb.view(torch.int32), st0)
    eng.forward_clips_device(r["xn"], r["lens"], None, ha, out=yb)
    assert torch.equal(ha, 2 * h0) and torch.equal(yb.view(torch.int32), y0)
    # a fresh output tensor holds the same valid rows
    yc = eng.forward_clips_device(r["xn"], r["lens"])
    assert torch.equal(yc.view(torch.int32)[valid], y0[valid])
    # an array raised beforehand is only raised
    pre = eng.new_stats()
    pre[0::2] = 1e30
    eng.forward_clips_device(r["xn"], r["lens"], pre)
    assert bool((pre[0::2] == 1e30).all()) and torch.equal(pre[1::2].view(torch.int32), st0[1::2])


@pytest.mark.gpu
def test_an_all_empty_launch_changes_nothing_and_bad_calls_are_refused():
    import torch
    from sparsernns_amd import _lib

    dim, lib = 0.25, _lib.lib
    eng, r = engine(dim), clip_run(dim, "A")
    n, Lmax = r["xn"].shape[:2]
    nk = len(eng.keys)
    ybuf, y = guarded(eng, n * Lmax * 257, torch.int32, SENT32)
    sbuf, st = guarded(eng, nk, torch.int32, SENT32, 5)
    hbuf, hd = guarded(eng, nk * 64, torch.int64, SENT64, 7)
    need = lib.s5fxp_float_workspace_bytes(eng._h, n, Lmax, 0)
    ws = torch.empty(need // 4, dtype=torch.float32, device=eng.device)
    empty = torch.tensor([0, -1, 0, -70, 0], dtype=torch.int32, device=eng.device)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda lens, hp, nbytes, nn=n: lib.s5fxp_float_model_clips(eng._h, r["xn"].data_ptr(), nn, Lmax, lens, y.data_ptr(),
                                                                       st.data_ptr(), hp, ws.data_ptr(), nbytes, stream)
    assert call(empty.data_ptr(), hd.data_ptr(), need) == 0
    assert call(empty.data_ptr(), None, need) == 0
    assert call(r["lens"].data_ptr(), hd.data_ptr() + 4, need) == _lib.S5FXP_EBADARG  # misaligned
    assert call(r["lens"].data_ptr(), hd.data_ptr(), need - 1) == _lib.S5FXP_EWORKSPACE
    assert call(None, hd.data_ptr(), need) == _lib.S5FXP_EBADARG
    assert call(r["lens"].data_ptr(), hd.data_ptr(), need, 0) == _lib.S5FXP_EBADARG
    # 2^20 clips x 512 tiles: a 32-bit LDS counter could wrap, so hist is refused; without hist only the workspace is too small
    wrap = lambda hp: lib.s5fxp_float_model_clips(eng._h, r["xn"].data_ptr(), 1 << 20, 1 << 14, r["lens"].data_ptr(), y.data_ptr(),
                                                  None, hp, ws.data_ptr(), need, stream)
    assert wrap(hd.data_ptr()) == _lib.S5FXP_EBADARG and wrap(None) == _lib.S5FXP_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((ybuf == SENT32).all()) and bool((st == 5).all()) and bool((hd == 7).all())
    assert guards_intact(sbuf, SENT32) and guards_intact(hbuf, SENT64)
    # the Python checks, in forward_device's style
    with pytest.raises(ValueError):
        eng.forward_clips_device(r["xn"], r["lens"][:-1])
    with pytest.raises(ValueError):
        eng.forward_clips_device(r["xn"], r["lens"].to(torch.int64))
    with pytest.raises(ValueError):
        eng.forward_clips_device(r["xn"], r["lens"], out=torch.empty(n, Lmax + 1, 257, device=eng.device))
    with pytest.raises(ValueError):
        eng.forward_clips_device(r["xn"][:, :, :200], r["lens"])


@pytest.mark.gpu
def test_forward_clips_on_the_device_returns_each_clip_in_its_own_kind():
    import torch

    dim = 0.25
    eng, r = engine(dim), clip_run(dim, "A")
    x = r["xz"].cpu().numpy()
    clips = [x[e, :n] if e % 2 else torch.from_numpy(x[e, :n]) for e, n in enumerate(r["eff"])]
    st, hist = {}, {}
    ys = eng.forward_clips(clips, stats=st, hist=hist)
    for e, (y, n, p) in enumerate(zip(ys, r["eff"], r["per"])):
        assert isinstance(y, np.ndarray if e % 2 else torch.Tensor) and tuple(y.shape) == (n, 257)
        if n:
            assert np.array_equal(bits(y if e % 2 else y.numpy()), bits(p[0]))
    assert np.array_equal(bits([st[k] for k in eng.keys]), r["st"])
    assert all(np.array_equal(hist[k], row) for k, row in zip(eng.keys, r["hist"]))


@pytest.mark.gpu
def test_device_calibration_from_a_clip_pair_is_the_calibration_from_single_clips():
    from sparsernns_amd import floatmodel

    dim = 0.5
    eng, r = engine(dim), clip_run(dim, "A")
    md, _, dims = model(dim)
    singles = [r["xz"][e:e + 1, :n] for e, n in enumerate(r["eff"]) if n]
    for lens in (r["lens"], SETS["A"][1]):
        s0, q0 = floatmodel.calibrate(md, singles, dims["n_layers"], engine=eng)
        s1, q1 = floatmodel.calibrate(md, [(r["xn"], lens)], dims["n_layers"], engine=eng)
        assert s1 == s0
        same_ints(q1, q0)
        a = floatmodel.calibrate_clipped(md, singles, dims["n_layers"], P_CLIP, engine=eng)
        b = floatmodel.calibrate_clipped(md, [(r["xn"], lens)], dims["n_layers"], P_CLIP, engine=eng)
        assert b[0] == a[0] and b[2] == a[2] and all(np.array_equal(b[1][k], a[1][k]) for k in a[1])
        same_ints(b[3], a[3])


@pytest.mark.gpu
def test_audio_float_clips_are_the_per_clip_float_loop():
    import torch
    from sparsernns_amd import audio

    eng = engine(0.5)
    rng = np.random.default_rng(5)
    mk = lambda T: torch.from_numpy((0.05 * rng.standard_normal(T)).astype(np.float32)).to(eng.device)
    Ts = [512, 640, 4224, 9000]
    noisy, clean = [mk(T) for T in Ts], [mk(T) for T in Ts]
    loss, snr = audio.validate_float_clips(eng, noisy, clean, lam=0.001)
    assert tuple(loss.shape) == tuple(snr.shape) == (4,) and loss.dtype == torch.float32
    for e in range(4):
        wl, ws = audio.validate_float(eng, noisy[e][None], clean[e][None], 0.001)
        assert torch.equal(loss[e:e + 1].view(torch.int32), wl.view(torch.int32)), e
        assert torch.equal(snr[e:e + 1].view(torch.int32), ws.view(torch.int32)), e
    got = audio.denoise_float_clips(eng, noisy)
    assert len(got) == 4
    for e in range(4):
        want = audio.denoise_float(eng, noisy[e][None])
        assert len(got[e]) == 4
        for a, b in zip(got[e], want):
            assert a.shape == b[0].shape and torch.equal(a.view(torch.int32), b[0].view(torch.int32)), e
    with pytest.raises(NotImplementedError):
        audio.denoise_float_clips(eng, noisy + [mk(511)])
    with pytest.raises(NotImplementedError):
        audio.validate_float_clips(eng, noisy + [mk(511)], clean + [mk(511)])
    assert audio.denoise_float_clips(eng, []) == []
    l0, s0 = audio.validate_float_clips(eng, [], [])
    assert l0.numel() == 0 and s0.numel() == 0
