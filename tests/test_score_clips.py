"""The scored masked inverse for n clips of different lengths in two launches (csrc/audio_score.hpp: k_mask_istft_score_clips,
k_score_finalize_clips; s5fxp_mask_istft_score_clips, s5fxp_score_clips_workspace_bytes) and the loop built on it
(audio.score_clips, audio.validate_clips).

Reference: the batch entry one clip at a time, audio.score_fused / validate_fused at B = 1, T = T_e, and audio.mask_istft_clips
for the planes.  A tile's six sums depend on that tile's frames and on the clip's own T and n_seg only, and the finalize adds a
clip's own tiles in the same order with the same expressions, so every comparison with an existing kernel is torch.equal: no
tolerance.  One test also goes against the float64 restatement of tests/test_audio_score.py, at that file's bounds (its docstring
derives them: 1e-4 dB for |si_snr| <= 40 dB, 1e-6 relative for mag_mse, 1e-5 for the loss recomputed from the returned float32
values); the clips there are that file's inputs(1, T) rows, whose restated si_snr the CPU test below holds within 40 dB.

Clip lengths: tests/test_audio_clips.py's tile edges (frames / output hops from 5/4 to 41/40; 1664 is exactly one inverse tile,
1792 a second tile of one hop), in one launch in shuffled order at Tmax = 5000 and 8192, where stated with a 100-sample clip (no
frames) and a Tmax + 50 one (clamped).  Inputs per clip: test_audio_score.inputs(1, T_e).

The padding is hostile: NaN behind every clip's noisy audio, clean audio and mask rows, a sentinel in out / cleaned_mag that must
survive behind each clip's end, the workspace NaN before every call (a finalize that reads a tile no workgroup wrote shows in the
score) and the score outputs pre-filled with the sentinel.  The GPU tests therefore call the C entry through _launch, which owns
the workspace and the outputs, and check audio.score_clips against it.

ST_WIDE_INPUT: tests/test_audio_clips.py::test_denoise_clips does not provoke one with this model (the float boundary quantises
to the encoder's 16 bits), so no such clip is included here."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_audio_kernels as AK
import test_audio_score as AS
from test_audio_clips import LENS, SENT, TMAXES, _frames, _shuffled

CAP = ((1 << 20) - 1) * 128
RESTATED_T = [512, 777, 1664, 1700, 5000]
NEW_SYMBOLS = ("s5fxp_score_clips_workspace_bytes", "s5fxp_mask_istft_score_clips")


def _clamp(T, Tmax):
    return min(max(T, 0), Tmax)


@functools.lru_cache(maxsize=None)
def _case(Ts, Tmax):
    """noisy, clean (n, Tmax) and mask (n, Lmax, 257) float32: clip e is test_audio_score.inputs(1, T_e), NaN behind it."""
    n, Lmax = len(Ts), _frames(Tmax)
    noisy, clean = (np.full((n, Tmax), np.nan, dtype=np.float32) for _ in range(2))
    mask = np.full((n, Lmax, 257), np.nan, dtype=np.float32)
    for e, T in enumerate(Ts):
        T = _clamp(T, Tmax)
        if T < 2:
            continue
        nz, cl, mk = AS.inputs(1, T)
        noisy[e, :T], clean[e, :T] = nz[0], cl[0]
        mask[e, :_frames(T)] = mk[0, :_frames(T)]
    return noisy, clean, mask


def _with_edges(Tmax):
    return tuple(_shuffled() + [100, Tmax + 50])


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_version():
    from sparsernns_amd import _lib
    assert _lib.lib.s5fxp_version() >= 114
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and hasattr(_lib.lib, name), name


def test_workspace_bytes():
    from sparsernns_amd import _lib
    w = _lib.lib.s5fxp_score_clips_workspace_bytes
    assert w(1, 512) == 48 and w(1, 1664) == 48 and w(1, 1700) == 96 and w(3, 5000) == 3 * 4 * 48
    assert [w(n, T) for n, T in ((0, 512), (-1, 5000), (1, 511), (3, 0), (1, -7), (1, CAP + 1), (5, 1 << 40))] == [0] * 7
    assert w(1, CAP) == 48 * -(-((1 << 20) - 1) // 13)      # frames(CAP) = 2^20
    # a launch at Tmax needs what the batch entry needs for n sequences of Tmax samples
    sizes = [512, 513, 777, 1664, 1665, 1700, 5000, 480000]
    for n in (1, 2, 3, 32):
        by_t = [w(n, T) for T in sizes]
        assert by_t == [_lib.lib.s5fxp_score_workspace_bytes(n, T) for T in sizes]
        assert all(a <= b for a, b in zip(by_t, by_t[1:])) and by_t[0] > 0
        assert all(w(n, T) < w(n + 1, T) for T in sizes)


def _check_arguments():
    """The codes come back for pointers that are not device memory at all: nothing was launched or dereferenced."""
    from sparsernns_amd import _lib
    L, bad, big = _lib.lib, C.c_void_p(64), 1 << 40
    f = lambda a=bad, c=bad, m=bad, n=1, T=512, s=bad, ws=bad, wb=big, si=bad, o=None, cm=None, mse=None, loss=None: \
        L.s5fxp_mask_istft_score_clips(a, c, m, n, T, s, 0.001, o, cm, ws, wb, si, mse, loss, None)
    for kw in (dict(a=None), dict(c=None), dict(s=None), dict(ws=None), dict(si=None), dict(n=0), dict(n=-2), dict(T=CAP + 1)):
        assert f(**kw) == _lib.S5FXP_EBADARG, kw
        assert f(o=bad, cm=bad, mse=bad, loss=bad, **kw) == _lib.S5FXP_EBADARG, kw
    assert f(T=511) == _lib.S5FXP_EUNSUPPORTED and f(T=0, m=None) == _lib.S5FXP_EUNSUPPORTED
    assert f(T=-5, o=bad, cm=bad) == _lib.S5FXP_EUNSUPPORTED
    # a grid beyond 2^31 - 1 workgroups: 80660 tiles at the cap
    assert f(n=30000, T=CAP) == _lib.S5FXP_EUNSUPPORTED and f(n=(1 << 31) - 1, T=CAP) == _lib.S5FXP_EUNSUPPORTED
    assert f(n=(1 << 31) - 1, T=512, wb=((1 << 31) - 1) * 48 - 1) == _lib.S5FXP_EWORKSPACE     # the largest grid itself is not refused
    assert f(wb=47) == _lib.S5FXP_EWORKSPACE and f(wb=0) == _lib.S5FXP_EWORKSPACE
    assert f(n=3, T=5000, wb=L.s5fxp_score_clips_workspace_bytes(3, 5000) - 1) == _lib.S5FXP_EWORKSPACE
    assert f(n=13, T=8192, wb=L.s5fxp_score_clips_workspace_bytes(13, 8192) - 1) == _lib.S5FXP_EWORKSPACE
    # bad arguments come first, then unsupported sizes, then the workspace
    assert f(n=0, T=100) == _lib.S5FXP_EBADARG and f(ws=None, T=100) == _lib.S5FXP_EBADARG and f(si=None, T=511, wb=0) == _lib.S5FXP_EBADARG
    assert f(T=511, wb=0) == _lib.S5FXP_EUNSUPPORTED and f(n=30000, T=CAP, wb=0) == _lib.S5FXP_EUNSUPPORTED


def test_argument_validation_needs_no_device():
    _check_arguments()


@pytest.mark.parametrize("T", RESTATED_T)
def test_restated_inputs_stay_within_40_db(T):
    """The condition of the si_snr bound of test_against_the_float64_restatement, on the float64 restatement of the whole chain."""
    _, si, _ = AS.restated_scores(*AS.inputs(1, T), 0.001)
    print("si_snr (dB):", si)
    assert np.all(np.abs(si) <= 40.0)


@pytest.mark.parametrize("Tmax", TMAXES)
def test_cpu_score_clips_equals_per_clip_score_fused(Tmax):
    import torch
    from sparsernns_amd import audio
    Ts = _with_edges(Tmax)
    n, Lmax = len(Ts), _frames(Tmax)
    nz, cl, mk = (torch.from_numpy(a) for a in _case(Ts, Tmax))
    s = torch.tensor(Ts, dtype=torch.int32)
    out, cm = torch.full((n, (Lmax - 1) * 128), SENT), torch.full((n, Lmax, 257), SENT)
    for lam in AS.LAMS:
        r = audio.score_clips(nz, cl, s, mk, lam=lam, cleaned=True, cleaned_mag=True, out=(out, cm))
        assert len(r) == 5 and r[3] is out and r[4] is cm
        assert all(t.shape == (n,) and t.dtype == torch.float32 for t in r[:3])
        bare = audio.score_clips(nz, cl, s, mk, lam=lam)
        assert len(bare) == 3
        for e, T in enumerate(Ts):
            T = _clamp(T, Tmax)
            L = _frames(T)
            if not L:
                assert all(torch.isnan(t[e]) for t in r[:3] + bare), Ts[e]
            else:
                w = audio.score_fused(nz[e:e + 1, :T], cl[e:e + 1, :T], mk[e:e + 1, :L], lam=lam, cleaned=True, cleaned_mag=True)
                for name, g, b, x in zip(("loss", "si_snr", "mag_mse"), r, bare, w):
                    assert torch.equal(g[e:e + 1], x) and torch.equal(b[e:e + 1], x), (name, Ts[e])
                assert torch.equal(out[e, :(L - 1) * 128], w[3][0]) and torch.equal(cm[e, :L], w[4][0]), Ts[e]
            assert (out[e, max(L - 1, 0) * 128:] == SENT).all() and (cm[e, L:] == SENT).all(), Ts[e]
    assert len(audio.score_clips(nz, cl, s, mk, cleaned_mag=True)) == 4 and len(audio.score_clips(nz, cl, s, mk, cleaned=True)) == 4
    # no mask = a zero mask
    zero = torch.where(torch.isnan(mk), mk, torch.zeros_like(mk))
    a, b = audio.score_clips(nz, cl, s, None), audio.score_clips(nz, cl, s, zero)
    keep = [e for e, T in enumerate(Ts) if _frames(_clamp(T, Tmax))]
    assert all(torch.equal(x[keep], y[keep]) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        audio.score_clips(nz, cl, s.to(torch.int64), mk)
    with pytest.raises(ValueError):
        audio.score_clips(nz, cl[:, :-1], s, mk)
    with pytest.raises(ValueError):
        audio.score_clips(nz, cl[:-1], s, mk)
    with pytest.raises(ValueError):
        audio.score_clips(nz, cl, s, mk[:, :-1])
    with pytest.raises(ValueError):
        audio.score_clips(nz, cl, s, mk, cleaned=True, out=(cm,))
    with pytest.raises(NotImplementedError):
        audio.score_clips(nz[:, :511], cl[:, :511], s, None)


def _clip_pairs(device="cpu"):
    """Clean and noisy clips of LENS, shuffled (test_audio_score.test_validate_fused's recipe)."""
    import torch
    g = torch.Generator().manual_seed(6)
    clean = [0.05 * torch.randn(T, generator=g) for T in _shuffled()]
    noisy = [c + 0.02 * torch.randn(c.shape[0], generator=g) for c in clean]
    return [c.to(device) for c in noisy], [c.to(device) for c in clean]


def test_cpu_validate_clips_equals_per_clip_validate_fused():
    import torch
    from sparsernns_amd import audio
    model = AS._StubModel()
    noisy, clean = _clip_pairs()
    for lam in AS.LAMS:
        loss, score = audio.validate_clips(model, 16, 12, noisy, clean, lam=lam)
        assert loss.shape == score.shape == (len(noisy),) and loss.dtype == score.dtype == torch.float32
        for e, (c, k) in enumerate(zip(noisy, clean)):
            wl, ws = audio.validate_fused(model, 16, 12, c[None], k[None], lam=lam)
            assert torch.equal(loss[e:e + 1], wl) and torch.equal(score[e:e + 1], ws), c.shape[0]


def test_validate_clips_checks_its_lists():
    import torch
    from sparsernns_amd import audio
    model = AS._StubModel()
    loss, score = audio.validate_clips(model, 16, 12, [], [])
    assert loss.shape == score.shape == (0,) and loss.dtype == score.dtype == torch.float32
    with pytest.raises(ValueError):
        audio.validate_clips(model, 16, 12, [torch.zeros(4096), torch.zeros(600)], [torch.zeros(4096), torch.zeros(601)])
    with pytest.raises(ValueError):
        audio.validate_clips(model, 16, 12, [torch.zeros(4096), torch.zeros(600)], [torch.zeros(4096)])
    with pytest.raises(ValueError):
        audio.validate_clips(model, 16, 12, [torch.zeros(1, 4096)], [torch.zeros(1, 4096)])
    with pytest.raises(NotImplementedError):
        audio.validate_clips(model, 16, 12, [torch.zeros(4096), torch.zeros(511)], [torch.zeros(4096), torch.zeros(511)])


def test_denoise_clips_still_serves_the_stub():
    """The front half denoise_clips now shares with validate_clips: same tuples as before for a model without an engine."""
    import torch
    from sparsernns_amd import audio
    model = AS._StubModel()
    noisy, _ = _clip_pairs()
    assert hasattr(audio, "validate_clips")
    for c, g in zip(noisy[:3], audio.denoise_clips(model, 16, 12, noisy[:3])):
        assert all(torch.equal(t, w[0]) for t, w in zip(g, audio.denoise_fused(model, 16, 12, c[None])))


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_case(Ts, Tmax):
    """The case on the device and, per clip, what the batch entry gives it alone at both lam: computed once, never written.
    ref[lam][e] = (loss, si_snr, mag_mse) as (1,) tensors, None for a clip without frames."""
    import torch
    from sparsernns_amd import audio
    nz, cl, mk = (torch.from_numpy(a).cuda() for a in _case(Ts, Tmax))
    ref = {}
    for lam in AS.LAMS:
        ref[lam] = []
        for e, T in enumerate(Ts):
            T = _clamp(T, Tmax)
            L = _frames(T)
            ref[lam].append(audio.score_fused(nz[e:e + 1, :T], cl[e:e + 1, :T], mk[e:e + 1, :L], lam=lam) if L else None)
    s = torch.tensor(Ts, dtype=torch.int32, device="cuda")
    n, Lmax = len(Ts), _frames(Tmax)
    out, cm = torch.full((n, (Lmax - 1) * 128), SENT, device="cuda"), torch.full((n, Lmax, 257), SENT, device="cuda")
    audio.mask_istft_clips(nz, s, mk, cleaned_mag=True, out=(out, cm))
    return nz, cl, mk, s, ref, out, cm


def _launch(nz, cl, mk, s, Tmax, lam, with_out, with_cm):
    """s5fxp_mask_istft_score_clips with a NaN workspace and sentinels everywhere -> (loss, si_snr, mag_mse, out, cleaned_mag)."""
    import torch
    from sparsernns_amd import _lib
    n, Lmax = nz.shape[0], _frames(Tmax)
    wb = _lib.lib.s5fxp_score_clips_workspace_bytes(n, Tmax)
    assert wb == 48 * n * -(-(Lmax - 1) // 13)
    ws = torch.full((wb // 8,), float("nan"), dtype=torch.float64, device="cuda")
    scores = torch.full((3, n), SENT, device="cuda")
    out = torch.full((n, (Lmax - 1) * 128), SENT, device="cuda") if with_out else None
    cm = torch.full((n, Lmax, 257), SENT, device="cuda") if with_cm else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.check(_lib.lib.s5fxp_mask_istft_score_clips(nz.data_ptr(), cl.data_ptr(), ptr(mk), n, Tmax, s.data_ptr(), lam, ptr(out), ptr(cm),
                                                     ws.data_ptr(), wb, scores[1].data_ptr(), scores[2].data_ptr(), scores[0].data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), "s5fxp_mask_istft_score_clips")
    return scores[0], scores[1], scores[2], out, cm


def _check_scores(got, ref, Ts, what):
    import torch
    for e, r in enumerate(ref):
        if r is None:
            assert all(torch.isnan(g[e]) for g in got), (what, Ts[e], [float(g[e]) for g in got])
            continue
        for name, g, w in zip(("loss", "si_snr", "mag_mse"), got, r):
            assert torch.equal(g[e:e + 1], w), (what, name, Ts[e], float(g[e]), float(w))


@pytest.mark.gpu
@pytest.mark.parametrize("Tmax", TMAXES)
def test_scores_and_planes_per_clip(Tmax):
    import torch
    from sparsernns_amd import audio
    Ts = _with_edges(Tmax)
    nz, cl, mk, s, ref, out_ref, cm_ref = _device_case(Ts, Tmax)
    n, Lmax = len(Ts), _frames(Tmax)
    for lam in AS.LAMS:
        full = _launch(nz, cl, mk, s, Tmax, lam, True, True)
        _check_scores(full[:3], ref[lam], Ts, "both planes")
        assert torch.equal(full[3], out_ref) and torch.equal(full[4], cm_ref)
        for with_out, with_cm in ((False, False), (True, False), (False, True), (True, True)):
            r = _launch(nz, cl, mk, s, Tmax, lam, with_out, with_cm)
            _check_scores(r[:3], ref[lam], Ts, (with_out, with_cm))
            assert not with_out or torch.equal(r[3], out_ref)
            assert not with_cm or torch.equal(r[4], cm_ref)
        # the Python entry: fresh scores, the caller's planes
        out, cm = torch.full_like(out_ref, SENT), torch.full_like(cm_ref, SENT)
        r = audio.score_clips(nz, cl, s, mk, lam=lam, cleaned=True, cleaned_mag=True, out=(out, cm))
        _check_scores(r[:3], ref[lam], Ts, "score_clips")
        assert r[3] is out and r[4] is cm and torch.equal(out, out_ref) and torch.equal(cm, cm_ref)
        r = audio.score_clips(nz, cl, s, mk, lam=lam)
        assert len(r) == 3 and all(t.shape == (n,) and t.dtype == torch.float32 for t in r)
        _check_scores(r, ref[lam], Ts, "score_clips, no planes")
    # the clip without frames: nothing of it but the scores is written; the clamped one fills its row
    e0, e1 = Ts.index(100), Ts.index(Tmax + 50)
    assert (out_ref[e0] == SENT).all() and (cm_ref[e0] == SENT).all()
    assert not (out_ref[e1] == SENT).any() and not (cm_ref[e1] == SENT).any()
    # optional score outputs: si_snr alone
    from sparsernns_amd import _lib
    wb = _lib.lib.s5fxp_score_clips_workspace_bytes(n, Tmax)
    ws = torch.full((wb // 8,), float("nan"), dtype=torch.float64, device="cuda")
    si = torch.full((n,), SENT, device="cuda")
    _lib.check(_lib.lib.s5fxp_mask_istft_score_clips(nz.data_ptr(), cl.data_ptr(), mk.data_ptr(), n, Tmax, s.data_ptr(), 0.001, None, None,
                                                     ws.data_ptr(), wb, si.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream))
    _check_scores((si,), [r[1:2] if r else None for r in ref[0.001]], Ts, "si_snr alone")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1792, 5000])
def test_equal_lengths_are_the_batch_kernel(T):
    import torch
    from sparsernns_amd import audio
    nz, cl, mk = (torch.from_numpy(a).cuda() for a in AS.inputs(3, T))
    s = torch.tensor([T] * 3, dtype=torch.int32, device="cuda")
    for lam in AS.LAMS:
        want = audio.score_fused(nz, cl, mk, lam=lam, cleaned=True, cleaned_mag=True)
        got = _launch(nz, cl, mk, s, T, lam, True, True)
        for name, g, w in zip(("loss", "si_snr", "mag_mse", "cleaned", "cleaned_mag"), got, want):
            assert torch.equal(g, w), (name, lam)
        got = audio.score_clips(nz, cl, s, mk, lam=lam, cleaned=True, cleaned_mag=True)
        assert len(got) == 5 and all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [777, 1664, 1792])
def test_a_single_clip(T):
    import torch
    from sparsernns_amd import audio
    for Tmax in (T, 4096):
        nz, cl, mk, s, ref, out_ref, cm_ref = _device_case((T,), Tmax)
        L = _frames(T)
        want = audio.score_fused(nz[:, :T], cl[:, :T], mk[:, :L], cleaned=True, cleaned_mag=True)
        got = _launch(nz, cl, mk, s, Tmax, 0.001, True, True)
        assert all(torch.equal(g, w) for g, w in zip(got[:3], want[:3]))
        assert torch.equal(got[3][:, :(L - 1) * 128], want[3]) and torch.equal(got[4][:, :L], want[4])
        assert torch.equal(got[3], out_ref) and torch.equal(got[4], cm_ref)
        _check_scores(_launch(nz, cl, mk, s, Tmax, 0.001, False, False)[:3], ref[0.001], (T,), "no planes")


@pytest.mark.gpu
def test_null_mask_and_side_stream():
    import torch
    Tmax = TMAXES[0]
    Ts = _with_edges(Tmax)
    nz, cl, mk, s, ref, out_ref, cm_ref = _device_case(Ts, Tmax)
    keep = [e for e, r in enumerate(ref[0.001]) if r is not None]
    zero = torch.where(torch.isnan(mk), mk, torch.zeros_like(mk))
    a = _launch(nz, cl, None, s, Tmax, 0.001, True, True)
    b = _launch(nz, cl, zero, s, Tmax, 0.001, True, True)
    assert all(torch.equal(x[keep], y[keep]) for x, y in zip(a[:3], b[:3])) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert not torch.equal(a[3], out_ref)
    # two calls give identical bits
    c, d = _launch(nz, cl, mk, s, Tmax, 0.001, True, True), _launch(nz, cl, mk, s, Tmax, 0.001, True, True)
    assert all(torch.equal(x[keep], y[keep]) for x, y in zip(c[:3], d[:3])) and torch.equal(c[3], d[3]) and torch.equal(c[4], d[4])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r = _launch(nz, cl, mk, s, Tmax, 0.001, True, True)
    side.synchronize()
    _check_scores(r[:3], ref[0.001], Ts, "side stream")
    assert torch.equal(r[3], out_ref) and torch.equal(r[4], cm_ref)


@pytest.mark.gpu
def test_against_the_float64_restatement():
    """References: fxprun.py:79-88 in float64 (a) on the device's own planes, which the unchanged per-clip entries produce -- the
    reference test_audio_score.py derives its bounds for -- and (b) on the float64 transforms of the inputs, end to end."""
    import torch
    from sparsernns_amd import audio
    Tmax, Ts = 8192, tuple(RESTATED_T)
    nz, cl, mk, s, _, out, cm = _device_case(Ts, Tmax)
    noisy, clean, mask = _case(Ts, Tmax)
    on, cn = out.cpu().numpy(), cm.cpu().numpy()
    for lam in AS.LAMS:
        loss, score, mag_mse = (t.cpu().numpy() for t in _launch(nz, cl, mk, s, Tmax, lam, False, False)[:3])
        for e, T in enumerate(Ts):
            L = _frames(T)
            clean_mag = audio.stft_mag(cl[e:e + 1, :T].contiguous(), sub=0.0).cpu().numpy()
            refs = {"device planes": AS.ref_scores(on[e:e + 1, :(L - 1) * 128], cn[e:e + 1, :L], clean[e:e + 1, :T], clean_mag, lam),
                    "float64 chain": AS.restated_scores(noisy[e:e + 1, :T], clean[e:e + 1, :T], mask[e:e + 1, :L], lam)}
            again = np.float64(lam) * np.float64(mag_mse[e]) + (100.0 - np.float64(score[e]))
            d_loss = abs(np.float64(loss[e]) - again)
            for name, (ls, si, mse) in refs.items():
                assert abs(si[0]) <= 40.0, (name, T, si)
                d_si, d_mse = abs(np.float64(score[e]) - si[0]), abs(np.float64(mag_mse[e]) - mse[0]) / mse[0]
                print(f"T {T} lam {lam} vs {name}: si_snr {si[0]:.4f} dB, |si_snr - ref| = {d_si:.3e}, |mag_mse - ref| / ref = {d_mse:.3e}, "
                      f"|loss - recomputed| = {d_loss:.3e}, |loss - ref| = {abs(np.float64(loss[e]) - ls[0]):.3e}")
                assert d_si <= 1e-4, (name, T, lam)
                assert d_mse <= 1e-6, (name, T, lam)
            assert d_loss <= 1e-5, (T, lam)


@pytest.mark.gpu
@pytest.mark.parametrize("dim_scale", [0.5, 0.25])
def test_validate_clips(dim_scale):
    """Every clip's (loss, si_snr) equals validate_fused of the clip alone; the model launch was the clip kernel."""
    import torch
    from sparsernns_amd import _lib, audio
    model, ib, ie = AK._model(dim_scale)
    noisy, clean = _clip_pairs("cuda")
    n = len(noisy)
    for lam in AS.LAMS:
        want = [audio.validate_fused(model, ib, ie, c[None], k[None], lam=lam) for c, k in zip(noisy, clean)]
        loss, score = audio.validate_clips(model, ib, ie, noisy, clean, lam=lam, lane=1)
        st = model.engine().lane_status(1, n).cpu().numpy()[:n * _lib.STATUS_WORDS].reshape(n, _lib.STATUS_WORDS)
        assert (st[:, 2] == _lib.PATH_CLIP).all(), st[:, :3]
        assert loss.shape == score.shape == (n,) and loss.dtype == score.dtype == torch.float32
        for e, (wl, ws) in enumerate(want):
            assert torch.equal(loss[e:e + 1], wl) and torch.equal(score[e:e + 1], ws), (noisy[e].shape[0], lam)
    # clean clips on another device than the noisy ones: the per-clip route refuses them as validate_fused does
    with pytest.raises(ValueError):
        audio.validate_clips(model, ib, ie, noisy[:2], [c.cpu() for c in clean[:2]])


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["store_intermediates", "other_input_configuration"])
def test_validate_clips_fallback(how):
    """A model that stores intermediates, or an input configuration other than the encoder's, takes validate_fused per clip."""
    import torch
    from sparsernns_amd import audio, synth
    from sparsernns_amd.fxpmodel import build_regression_model
    md, qc, dims = synth.make_model(0.25, calib_L=128)
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    if how == "store_intermediates":
        model = build_regression_model(md, qc, dims["n_layers"], store_intermediates=True)
    else:
        model, ie = build_regression_model(md, qc, dims["n_layers"]), ie - 1
    pairs = [(c, k) for c, k in zip(*_clip_pairs("cuda")) if c.shape[0] in (513, 1792, 2048)]
    loss, score = audio.validate_clips(model, ib, ie, [p[0] for p in pairs], [p[1] for p in pairs])
    assert loss.shape == score.shape == (3,)
    for e, (c, k) in enumerate(pairs):
        wl, ws = audio.validate_fused(model, ib, ie, c[None], k[None])
        assert torch.equal(loss[e:e + 1], wl) and torch.equal(score[e:e + 1], ws), c.shape[0]


@pytest.mark.gpu
def test_argument_validation_before_any_device_access():
    _check_arguments()
