"""The STFT and the masked inverse for n clips of different lengths in one launch each (csrc/audio_stft.hpp: k_stft_mag_clips,
k_mask_istft_clips; s5fxp_stft_mag_clips, s5fxp_mask_istft_clips) and the loop built on them (audio.stft_mag_clips,
mask_istft_clips, denoise_clips).

Reference: the existing kernels, one clip at a time (audio.stft_mag / mask_istft / denoise_fused at B = 1, T = T_e).  A frame's
transform and an output hop's sum do not depend on the workgroup that computes them, so every comparison of a new kernel with
an existing one is torch.equal / np.array_equal: no tolerance.  One case per direction also goes against the float64
restatement of tests/test_audio_kernels.py at that file's tolerance.

Clip lengths: the smallest at which the tiling can go wrong -- 16 frames per forward tile, 13 output hops per inverse tile
(frames / output hops): 512 (5/4), 513 (6/5), 777 (8/7), 1536 (13/12), 1664 (14/13: one inverse tile), 1792 (15/14: a second
inverse tile of one hop), 1920 (16/15: exactly one forward tile), 2048 (17/16: a forward tile of one frame), 3968 (32/31),
4096 (33/32), 5000 (41/40).  All go into one launch in shuffled order, at Tmax = 5000 and at Tmax = 8192 (above every clip).

The padding is hostile: NaN behind every clip's audio and behind its mask rows, a sentinel in every output that must survive
behind the clip's end."""
import ctypes as C

import numpy as np
import pytest

import test_audio_kernels as AK
from test_audio_kernels import ATOL_AUDIO, ATOL_SPEC, ref_istft, ref_stft

LENS = [512, 513, 777, 1536, 1664, 1792, 1920, 2048, 3968, 4096, 5000]
FRAMES = [5, 6, 8, 13, 14, 15, 16, 17, 32, 33, 41]
TMAXES = [5000, 8192]
SENT = 7.5   # no transform of the test audio produces it, and it is not NaN, so `==` finds it


def _frames(T):
    return 0 if T < 512 else -(-T // 128) + 1


def _clips(Ts, Tmax, amp=1.0, seed=0):
    """(n, Tmax) float32: clip e in the first min(Ts[e], Tmax) samples of row e, NaN behind it."""
    rng = np.random.default_rng(seed)
    a = np.full((len(Ts), Tmax), np.nan, dtype=np.float32)
    for e, T in enumerate(Ts):
        T = min(max(T, 0), Tmax)
        a[e, :T] = amp * rng.standard_normal(T)
    return a


def _shuffled(seed=4):
    return [LENS[i] for i in np.random.default_rng(seed).permutation(len(LENS))]


def _masks(Ts, Tmax, lo=-1.0, hi=1.0, seed=1):
    """(n, Lmax, 257) float32: uniform in [lo, hi] in the clip's rows, NaN behind them."""
    rng = np.random.default_rng(seed)
    m = np.full((len(Ts), _frames(Tmax), 257), np.nan, dtype=np.float32)
    for e, T in enumerate(Ts):
        L = _frames(min(max(T, 0), Tmax))
        m[e, :L] = rng.uniform(lo, hi, (L, 257))
    return m


def test_lengths_are_the_tile_edges():
    assert [_frames(T) for T in LENS] == FRAMES
    assert sorted(_shuffled()) == LENS and _shuffled() != LENS


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_version():
    from sparsernns_amd import _lib
    assert _lib.lib.s5fxp_version() >= 113
    for name in ("s5fxp_stft_mag_clips", "s5fxp_mask_istft_clips"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)


def test_argument_validation_before_any_device_access():
    """The codes come back for pointers that are not device memory at all: nothing was launched or dereferenced."""
    from sparsernns_amd import _lib
    L, bad = _lib.lib, C.c_void_p(64)  # an address no allocation holds
    cap = ((1 << 20) - 1) * 128
    f = L.s5fxp_stft_mag_clips     # (audio, n, Tmax, samples, sub, x, spec, lens, stream)
    assert f(None, 1, 512, bad, 0.0, bad, None, None, None) == _lib.S5FXP_EBADARG
    assert f(bad, 1, 512, None, 0.0, bad, None, None, None) == _lib.S5FXP_EBADARG
    assert f(bad, 1, 512, bad, 0.0, None, None, None, None) == _lib.S5FXP_EBADARG
    assert f(bad, 0, 512, bad, 0.0, bad, bad, bad, None) == _lib.S5FXP_EBADARG
    assert f(bad, 1, cap + 1, bad, 0.0, bad, None, None, None) == _lib.S5FXP_EBADARG
    assert f(bad, 1, 511, bad, 0.0, bad, None, None, None) == _lib.S5FXP_EUNSUPPORTED
    assert f(bad, 1, 0, bad, 0.0, bad, bad, bad, None) == _lib.S5FXP_EUNSUPPORTED
    g = L.s5fxp_mask_istft_clips   # (audio, mask, n, Tmax, samples, out, cleaned_mag, stream)
    assert g(None, None, 1, 512, bad, bad, None, None) == _lib.S5FXP_EBADARG
    assert g(bad, None, 1, 512, None, bad, None, None) == _lib.S5FXP_EBADARG
    assert g(bad, bad, 1, 512, bad, None, None, None) == _lib.S5FXP_EBADARG
    assert g(bad, bad, -1, 512, bad, bad, bad, None) == _lib.S5FXP_EBADARG
    assert g(bad, None, 1, cap + 1, bad, bad, None, None) == _lib.S5FXP_EBADARG
    assert g(bad, bad, 1, 511, bad, bad, bad, None) == _lib.S5FXP_EUNSUPPORTED


@pytest.mark.parametrize("Tmax", TMAXES)
def test_cpu_tensors_equal_the_per_clip_route(Tmax):
    import torch
    from sparsernns_amd import audio
    Ts = _shuffled() + [100, Tmax + 50]          # a clip without frames, and one that is clamped to Tmax
    n, Lmax = len(Ts), _frames(Tmax)
    a, m = torch.from_numpy(_clips(Ts, Tmax, seed=2)), torch.from_numpy(_masks(Ts, Tmax))
    s = torch.tensor(Ts, dtype=torch.int32)
    x = torch.full((n, Lmax, 257), SENT)
    spec = torch.full((n, Lmax, 257), complex(SENT, -SENT), dtype=torch.complex64)
    lens = torch.full((n,), -1, dtype=torch.int32)
    r = audio.stft_mag_clips(a, s, spectrum=True, out=(x, lens, spec))
    assert r[0] is x and r[1] is lens and r[2] is spec
    out = torch.full((n, (Lmax - 1) * 128), SENT)
    cm = torch.full((n, Lmax, 257), SENT)
    audio.mask_istft_clips(a, s, m, cleaned_mag=True, out=(out, cm))
    assert lens.tolist() == [_frames(min(T, Tmax)) for T in Ts] and lens[-2] == 0 and lens[-1] == Lmax
    for e, T in enumerate(Ts):
        T, L = min(T, Tmax), int(lens[e])
        if L:
            xe, se = audio.stft_mag(a[e:e + 1, :T], spectrum=True)
            oe, ce = audio.mask_istft(a[e:e + 1, :T], m[e:e + 1, :L], cleaned_mag=True)
            assert torch.equal(x[e, :L], xe[0]) and torch.equal(spec[e, :L], se[0])
            assert torch.equal(out[e, :(L - 1) * 128], oe[0]) and torch.equal(cm[e, :L], ce[0])
        assert (x[e, L:] == SENT).all() and (spec[e, L:] == complex(SENT, -SENT)).all() and (cm[e, L:] == SENT).all()
        assert (out[e, max(L - 1, 0) * 128:] == SENT).all()
    # fresh outputs, no spectrum / magnitude plane, no mask
    x2, lens2 = audio.stft_mag_clips(a, s)
    o2 = audio.mask_istft_clips(a, s, None)
    o0 = audio.mask_istft_clips(a, s, torch.zeros_like(m))
    for e in range(n):
        L = int(lens[e])
        assert torch.equal(x2[e, :L], x[e, :L]) and torch.equal(o2[e, :max(L - 1, 0) * 128], o0[e, :max(L - 1, 0) * 128])
    assert torch.equal(lens2, lens)
    with pytest.raises(ValueError):
        audio.stft_mag_clips(a, s.to(torch.int64))
    with pytest.raises(ValueError):
        audio.mask_istft_clips(a, s, m[:, :-1])
    with pytest.raises(NotImplementedError):
        audio.stft_mag_clips(a[:, :511], s)


def test_cpu_denoise_clips_equals_per_clip_denoise_fused():
    """Without a GPU no engine exists, so the model here is test_audio_kernels' float-route stub; the synthetic fixed-point
    model of test_audio_kernels._model serves the same comparison on the GPU (test_denoise_clips)."""
    import torch
    from sparsernns_amd import audio
    model = AK._StubModel()
    clips = [torch.from_numpy(AK._audio(1, T, amp=0.02, seed=T)[0]) for T in _shuffled()]
    got = audio.denoise_clips(model, 16, 12, clips)
    assert len(got) == len(clips)
    for c, g in zip(clips, got):
        want = audio.denoise_fused(model, 16, 12, c[None])
        L = _frames(c.shape[0])
        assert [tuple(t.shape) for t in g] == [((L - 1) * 128,), (L, 257), (L, 257), (L, 257)]
        for t, w in zip(g, want):
            assert torch.equal(t, w[0])


def test_short_clip_and_empty_list():
    import torch
    from sparsernns_amd import audio
    assert audio.denoise_clips(AK._StubModel(), 16, 12, []) == []
    with pytest.raises(NotImplementedError):
        audio.denoise_clips(AK._StubModel(), 16, 12, [torch.zeros(4096), torch.zeros(511)])
    with pytest.raises(ValueError):
        audio.denoise_clips(AK._StubModel(), 16, 12, [torch.zeros(1, 4096)])


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
_REF = {}


def _per_clip(Ts, Tmax, amp, sub, lo=-1.0, hi=1.0):
    """The existing kernels, one clip at a time: computed once per configuration, shared, never modified.
    Returns (audio, masks, [(x, spec, out, cleaned_mag) per clip, None for a clip without frames])."""
    import torch
    from sparsernns_amd import audio
    key = (tuple(Ts), Tmax, amp, sub, lo, hi)
    if key not in _REF:
        a, m = torch.from_numpy(_clips(Ts, Tmax, amp, seed=Tmax)).cuda(), torch.from_numpy(_masks(Ts, Tmax, lo, hi)).cuda()
        ref = []
        for e, T in enumerate(Ts):
            T = min(max(T, 0), Tmax)
            L = _frames(T)
            if not L:
                ref.append(None)
                continue
            ae = a[e:e + 1, :T].contiguous()
            x, spec = audio.stft_mag(ae, sub=sub, spectrum=True)
            out, cm = audio.mask_istft(ae, m[e:e + 1, :L].contiguous(), cleaned_mag=True)
            ref.append((x[0], spec[0], out[0], cm[0]))
        _REF[key] = (a, m, ref)
    return _REF[key]


def _samples(Ts):
    import torch
    return torch.tensor(Ts, dtype=torch.int32, device="cuda")


def _check_stft(Ts, Tmax, amp, sub, spectrum):
    import torch
    from sparsernns_amd import audio
    a, _, ref = _per_clip(Ts, Tmax, amp, sub)
    n, Lmax = len(Ts), _frames(Tmax)
    x = torch.full((n, Lmax, 257), SENT, device="cuda")
    lens = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    spec = torch.full((n, Lmax, 257), complex(SENT, -SENT), dtype=torch.complex64, device="cuda") if spectrum else None
    audio.stft_mag_clips(a, _samples(Ts), sub=sub, spectrum=spectrum, out=(x, lens, spec) if spectrum else (x, lens))
    assert lens.tolist() == [_frames(min(max(T, 0), Tmax)) for T in Ts]
    for e, r in enumerate(ref):
        L = int(lens[e])
        if r is not None:
            assert torch.equal(x[e, :L], r[0]), (e, Ts[e])
            assert not spectrum or torch.equal(spec[e, :L], r[1]), (e, Ts[e])
        assert (x[e, L:] == SENT).all(), (e, Ts[e])
        assert not spectrum or (spec[e, L:] == complex(SENT, -SENT)).all(), (e, Ts[e])
    return x, lens


@pytest.mark.gpu
@pytest.mark.parametrize("amp", [1.0, 0.02])
@pytest.mark.parametrize("Tmax", TMAXES)
def test_stft_mag_clips(Tmax, amp):
    import torch
    from sparsernns_amd import _lib
    Ts = _shuffled()
    for sub in (0.0007, 0.0):
        x, lens = _check_stft(Ts, Tmax, amp, sub, True)
        x2, _ = _check_stft(Ts, Tmax, amp, sub, False)
        assert torch.equal(x, x2)
    # lens = NULL at the ABI: the same x
    a = _per_clip(Ts, Tmax, amp, 0.0)[0]
    x3 = torch.full_like(x, SENT)
    _lib.check(_lib.lib.s5fxp_stft_mag_clips(a.data_ptr(), len(Ts), Tmax, _samples(Ts).data_ptr(), 0.0, x3.data_ptr(), None, None,
                                             torch.cuda.current_stream().cuda_stream))
    assert torch.equal(x3, x)
    # against the float64 restatement (sub = 0 here)
    if Tmax == TMAXES[0]:
        an, xn = a.cpu().numpy(), x.cpu().numpy()
        for e, T in enumerate(Ts):
            z = ref_stft(an[e:e + 1, :T])
            assert AK._maxdiff(f"mag T={T}", xn[e, :z.shape[1]], np.abs(z[0])) <= ATOL_SPEC * amp


def _check_istft(Ts, Tmax, amp, lo, hi, with_mag):
    import torch
    from sparsernns_amd import audio
    a, m, ref = _per_clip(Ts, Tmax, amp, 0.0007, lo, hi)
    n, Lmax = len(Ts), _frames(Tmax)
    out = torch.full((n, (Lmax - 1) * 128), SENT, device="cuda")
    cm = torch.full((n, Lmax, 257), SENT, device="cuda") if with_mag else None
    audio.mask_istft_clips(a, _samples(Ts), m, cleaned_mag=with_mag, out=(out, cm) if with_mag else (out,))
    for e, r in enumerate(ref):
        L = _frames(min(max(Ts[e], 0), Tmax))
        if r is not None:
            assert torch.equal(out[e, :(L - 1) * 128], r[2]), (e, Ts[e])
            assert not with_mag or torch.equal(cm[e, :L], r[3]), (e, Ts[e])
        assert (out[e, max(L - 1, 0) * 128:] == SENT).all(), (e, Ts[e])
        assert not with_mag or (cm[e, L:] == SENT).all(), (e, Ts[e])
    return out, cm


@pytest.mark.gpu
@pytest.mark.parametrize("rng", [(-1.0, 1.0), (-2.5, -1.5)], ids=["mask", "negative-factors"])
@pytest.mark.parametrize("Tmax", TMAXES)
def test_mask_istft_clips(Tmax, rng):
    import torch
    from sparsernns_amd import audio
    Ts, amp = _shuffled(), 1.0
    out, cm = _check_istft(Ts, Tmax, amp, *rng, True)
    out2, cm2 = _check_istft(Ts, Tmax, amp, *rng, True)     # two calls: identical bits
    out3, _ = _check_istft(Ts, Tmax, amp, *rng, False)      # without the magnitude plane
    assert torch.equal(out, out2) and torch.equal(cm, cm2) and torch.equal(out, out3)
    if rng[1] < -1.0:
        lens = [_frames(T) for T in Ts]
        assert all((cm[e, :L] <= 0).all() for e, L in enumerate(lens))
        return
    # mask = None is a zero mask (the zero mask has NaN rows behind every clip, the outputs a sentinel)
    a, m, _ = _per_clip(Ts, Tmax, amp, 0.0007, *rng)
    s = _samples(Ts)
    zero = torch.where(torch.isnan(m), m, torch.zeros_like(m))
    o_none, o_zero = (torch.full_like(out, SENT) for _ in range(2))
    audio.mask_istft_clips(a, s, None, out=(o_none,))
    audio.mask_istft_clips(a, s, zero, out=(o_zero,))
    assert torch.equal(o_none, o_zero) and not torch.equal(o_none, out)
    # against the float64 restatement
    if Tmax == TMAXES[0]:
        an, mn, on, cn = a.cpu().numpy(), m.cpu().numpy(), out.cpu().numpy(), cm.cpu().numpy()
        for e, T in enumerate(Ts):
            z = ref_stft(an[e:e + 1, :T])
            L = z.shape[1]
            f = 1.0 + mn[e:e + 1, :L].astype(np.float64)
            assert AK._maxdiff(f"cleaned T={T}", on[e:e + 1, :(L - 1) * 128], ref_istft(z * f)) <= ATOL_AUDIO * amp
            assert AK._maxdiff(f"cleaned_mag T={T}", cn[e:e + 1, :L], np.abs(z) * f) <= ATOL_SPEC * amp


@pytest.mark.gpu
def test_short_and_clamped_clips_among_valid_ones():
    """0, 100 and 511 samples: no frames, lens 0, nothing written.  samples[e] > Tmax: clamped to the row.  The neighbours get
    what they get alone (_check_* compare every clip with the per-clip kernels and every padding with its sentinel)."""
    Tmax = 2048
    Ts = [1792, 0, 777, 100, 2048, 511, 4000, 513, -3]
    for spectrum in (True, False):
        _, lens = _check_stft(Ts, Tmax, 1.0, 0.0007, spectrum)
    assert lens.tolist() == [15, 0, 8, 0, 17, 0, 17, 6, 0]
    _check_istft(Ts, Tmax, 1.0, -1.0, 1.0, True)
    _check_istft(Ts, Tmax, 1.0, -1.0, 1.0, False)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [777, 1664, 1792])
def test_a_single_clip(T):
    _check_stft([T], T, 1.0, 0.0007, True)
    _check_istft([T], T, 1.0, -1.0, 1.0, True)
    _check_stft([T], 4096, 1.0, 0.0007, False)
    _check_istft([T], 4096, 1.0, -1.0, 1.0, True)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1792, 5000])
def test_equal_lengths_are_the_batch_kernels(T):
    import torch
    from sparsernns_amd import audio
    B = 5
    a = torch.from_numpy(AK._audio(B, T, seed=T)).cuda()
    m = torch.from_numpy(AK._mask(B, T)).cuda()
    s = _samples([T] * B)
    x, lens, spec = audio.stft_mag_clips(a, s, spectrum=True)
    xb, sb = audio.stft_mag(a, spectrum=True)
    assert torch.equal(x, xb) and torch.equal(spec, sb) and lens.tolist() == [_frames(T)] * B
    out, cm = audio.mask_istft_clips(a, s, m, cleaned_mag=True)
    ob, cb = audio.mask_istft(a, m, cleaned_mag=True)
    assert torch.equal(out, ob) and torch.equal(cm, cb)


@pytest.mark.gpu
def test_side_stream():
    import torch
    from sparsernns_amd import audio
    Ts, Tmax = _shuffled(), TMAXES[0]
    a, m, ref = _per_clip(Ts, Tmax, 1.0, 0.0007)
    smp = _samples(Ts)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x, lens = audio.stft_mag_clips(a, smp)
        out, cm = audio.mask_istft_clips(a, smp, m, cleaned_mag=True)
    s.synchronize()
    for e, r in enumerate(ref):
        L = int(lens[e])
        assert torch.equal(x[e, :L], r[0]) and torch.equal(out[e, :(L - 1) * 128], r[2]) and torch.equal(cm[e, :L], r[3])


def _noisy_clips(amp=0.02):
    import torch
    g = torch.Generator().manual_seed(5)
    return [(amp * torch.randn(T, generator=g)).cuda() for T in _shuffled() + [8192]]


@pytest.mark.gpu
@pytest.mark.parametrize("dim_scale", [0.5, 0.25])
def test_denoise_clips(dim_scale):
    """Every clip and all four tensors equal denoise_fused of the clip alone; the mask is the C oracle's forward of the
    FLOOR-quantised x; the launch in between was the clip kernel (PATH_CLIP in every clip's status words)."""
    import torch
    from sparsernns_amd import _lib, audio
    model, ib, ie = AK._model(dim_scale)
    clips = _noisy_clips()
    n = len(clips)
    want = [audio.denoise_fused(model, ib, ie, c[None]) for c in clips]
    got = audio.denoise_clips(model, ib, ie, clips, lane=1)
    st = model.engine().lane_status(1, n).cpu().numpy()[:n * _lib.STATUS_WORDS].reshape(n, _lib.STATUS_WORDS)
    assert (st[:, 2] == _lib.PATH_CLIP).all(), st[:, :3]
    assert len(got) == n
    for c, g, w in zip(clips, got, want):
        L = _frames(c.shape[0])
        assert [tuple(t.shape) for t in g] == [((L - 1) * 128,), (L, 257), (L, 257), (L, 257)]
        for name, t, r in zip(("cleaned", "cleaned_mag", "x", "mask"), g, w):
            assert torch.equal(t, r[0]), (name, c.shape[0])
        _, mref = AK._oracle_mask(model, g[2].cpu().numpy()[None], ib, ie)
        assert np.array_equal(g[3].cpu().numpy(), mref[0]), c.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["store_intermediates", "other_input_configuration"])
def test_denoise_clips_fallback(how):
    """A model that stores intermediates, or an input configuration other than the encoder's, takes denoise_fused per clip."""
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd import synth
    from sparsernns_amd.fxpmodel import build_regression_model
    md, qc, dims = synth.make_model(0.25, calib_L=128)
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    if how == "store_intermediates":
        model = build_regression_model(md, qc, dims["n_layers"], store_intermediates=True)
    else:
        model, ie = build_regression_model(md, qc, dims["n_layers"]), ie - 1
    clips = [c for c in _noisy_clips() if c.shape[0] in (513, 1792, 2048)]
    got = audio.denoise_clips(model, ib, ie, clips)
    for c, g in zip(clips, got):
        for t, r in zip(g, audio.denoise_fused(model, ib, ie, c[None])):
            assert torch.equal(t, r[0]), c.shape[0]
