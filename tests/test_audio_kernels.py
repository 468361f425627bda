"""The HIP STFT / masked iSTFT (csrc/audio_stft.hpp: s5fxp_stft_mag, s5fxp_mask_istft) and the loop built on them
(audio.stft_mag, mask_istft, denoise_fused, validate_batch).

Reference: a float64 numpy restatement of scipy.signal.stft / istft for the recipe's parameters (nperseg = nfft = 512, hop 128,
boxcar, one-sided, boundary="zeros", padded=True, scaling="spectrum"), frame-major.  One test pins it to scipy at 1e-12; the
others use it, so they need numpy only.

Tolerance: what tests/test_cpu_suite.py holds the torch route to against scipy for unit-variance audio -- 2e-6 on spectrum and
magnitude, 2e-5 on audio -- times the amplitude of the input.  Every element is compared."""
import ctypes as C

import numpy as np
import pytest

from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth

ATOL_SPEC, ATOL_AUDIO = 2e-6, 2e-5
SIZES = [512, 513, 640, 777, 4096, 5000]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def ref_stft(x):
    """(B, T) -> (B, n_seg, 257) complex128."""
    x = np.asarray(x, dtype=np.float64)
    p = np.pad(x, ((0, 0), (256, 256)))
    p = np.pad(p, ((0, 0), (0, (-(p.shape[-1] - 512)) % 128)))
    n_seg = (p.shape[-1] - 512) // 128 + 1
    frames = np.stack([p[:, 128 * k: 128 * k + 512] for k in range(n_seg)], axis=1)
    return np.fft.rfft(frames, n=512, axis=-1) / 512.0


def ref_istft(z):
    """(B, n_seg, 257) -> (B, (n_seg - 1) * 128) float64."""
    seg = np.fft.irfft(z, n=512, axis=-1) * 512.0
    n_seg = seg.shape[1]
    total = 512 + 128 * (n_seg - 1)
    out, cover = np.zeros((seg.shape[0], total)), np.zeros(total)
    for k in range(n_seg):
        out[:, 128 * k: 128 * k + 512] += seg[:, k]
        cover[128 * k: 128 * k + 512] += 1.0
    out /= np.where(cover > 1e-10, cover, 1.0)
    return out[:, 256: total - 256]


def ref_si_snr(target, estimate):
    """train_helpers.py:15-53 in float64."""
    st = target - target.mean(-1, keepdims=True)
    se = estimate - estimate.mean(-1, keepdims=True)
    proj = (st * se).sum(-1, keepdims=True) * st / (st ** 2).sum(-1, keepdims=True)
    return 10 * np.log10((proj ** 2).sum(-1) / (((se - proj) ** 2).sum(-1) + 1e-8) + 1e-8)


def _audio(B, T, amp=1.0, seed=0):
    return (amp * np.random.default_rng(seed).standard_normal((B, T))).astype(np.float32)


def _mask(B, T, lo=-1.0, hi=1.0, seed=1):
    n_seg = -(-T // 128) + 1
    return np.random.default_rng(seed).uniform(lo, hi, (B, n_seg, 257)).astype(np.float32)


def _maxdiff(name, got, want):
    got = np.asarray(got)
    d = float(np.abs(got.astype(np.complex128 if np.iscomplexobj(got) else np.float64) - want).max())
    print(f"{name}: max |diff| = {d:.3e}")
    return d


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [512, 513, 777, 4096, 5000])
def test_restatement_is_scipy(T):
    sig = pytest.importorskip("scipy.signal")
    x = _audio(2, T, seed=T).astype(np.float64)
    kw = dict(nperseg=512, nfft=512, noverlap=384, window="boxcar")
    _, _, Z = sig.stft(x, return_onesided=True, **kw)
    z = ref_stft(x)
    assert z.shape == (2, -(-T // 128) + 1, 257)
    assert np.abs(z - Z.transpose(0, 2, 1)).max() <= 1e-12
    zm = z * (1.0 + _mask(2, T))
    _, xr = sig.istft(zm.transpose(0, 2, 1), input_onesided=True, **kw)
    back = ref_istft(zm)
    assert back.shape == xr.shape == (2, (z.shape[1] - 1) * 128)
    assert np.abs(back - xr).max() <= 1e-12


def test_symbols_and_version():
    from sparsernns_amd import _lib
    assert _lib.lib.s5fxp_version() >= 107
    for name in ("s5fxp_stft_frames", "s5fxp_stft_mag", "s5fxp_mask_istft"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)


def test_stft_frames():
    from sparsernns_amd import _lib, audio
    f = _lib.lib.s5fxp_stft_frames
    assert [f(T) for T in (512, 513, 640, 777, 4096, 5000, 480000)] == [5, 6, 6, 8, 33, 41, 3751]
    assert [f(T) for T in (511, 0, -5)] == [-1, -1, -1]
    for T in (512, 513, 640, 777, 4096, 5000):
        assert f(T) == ref_stft(np.zeros((1, T))).shape[1] == audio.stft_frames(T)
    with pytest.raises(NotImplementedError):
        audio.stft_frames(511)


def test_argument_validation_before_any_device_access():
    """The codes come back for pointers that are not device memory at all: nothing was launched or dereferenced."""
    from sparsernns_amd import _lib
    L, bad = _lib.lib, C.c_void_p(64)  # an address no allocation holds
    assert L.s5fxp_stft_mag(None, 1, 512, 0.0, bad, None, None) == _lib.S5FXP_EBADARG
    assert L.s5fxp_stft_mag(bad, 1, 512, 0.0, None, None, None) == _lib.S5FXP_EBADARG
    assert L.s5fxp_stft_mag(bad, 0, 512, 0.0, bad, None, None) == _lib.S5FXP_EBADARG
    assert L.s5fxp_stft_mag(bad, 1, 511, 0.0, bad, None, None) == _lib.S5FXP_EUNSUPPORTED
    assert L.s5fxp_mask_istft(None, None, 1, 512, bad, None, None) == _lib.S5FXP_EBADARG
    assert L.s5fxp_mask_istft(bad, None, 1, 512, None, None, None) == _lib.S5FXP_EBADARG
    assert L.s5fxp_mask_istft(bad, bad, -1, 512, bad, None, None) == _lib.S5FXP_EBADARG
    assert L.s5fxp_mask_istft(bad, bad, 1, 100, bad, bad, None) == _lib.S5FXP_EUNSUPPORTED


class _StubModel:
    """A float-route 'model' that runs anywhere: forward_float(x) is a fixed smooth function of x."""
    fxp_qconfig = {"encoder": {"inp_bits": 16, "inp_exp": 12}}

    def forward_float(self, x):
        import torch
        return torch.tanh(40.0 * x) - 0.25


@pytest.mark.parametrize("T", [512, 777, 5000])
def test_cpu_tensors_against_the_restatement(T):
    import torch
    from sparsernns_amd import audio
    a, m = _audio(2, T, seed=3), _mask(2, T)
    z = ref_stft(a)
    x, spec = audio.stft_mag(torch.from_numpy(a), spectrum=True)
    assert x.shape == z.shape and x.dtype == torch.float32 and spec.dtype == torch.complex64 and x.is_contiguous()
    assert _maxdiff("x", x.numpy() + audio.STFT_MAG_MEAN, np.abs(z)) <= ATOL_SPEC
    assert _maxdiff("spec", spec.numpy(), z) <= ATOL_SPEC
    assert _maxdiff("mag", audio.stft_mag(torch.from_numpy(a), sub=0.0).numpy(), np.abs(z)) <= ATOL_SPEC
    out, cm = audio.mask_istft(torch.from_numpy(a), torch.from_numpy(m), cleaned_mag=True)
    assert _maxdiff("cleaned", out.numpy(), ref_istft(z * (1.0 + m))) <= ATOL_AUDIO
    assert _maxdiff("cleaned_mag", cm.numpy(), np.abs(z) * (1.0 + m)) <= ATOL_SPEC
    rt = audio.mask_istft(torch.from_numpy(a), None).numpy()
    assert rt.shape == (2, (z.shape[1] - 1) * 128) and _maxdiff("round trip", rt[:, :T], a.astype(np.float64)) <= ATOL_AUDIO
    with pytest.raises(NotImplementedError):
        audio.stft_mag(torch.zeros(1, 511))
    with pytest.raises(ValueError):
        audio.mask_istft(torch.from_numpy(a), torch.from_numpy(m[:, :-1]))


def test_cpu_denoise_fused_and_validate_batch():
    import torch
    from sparsernns_amd import audio
    T, model = 2000, _StubModel()
    clean = _audio(3, T, amp=0.05, seed=8)
    noisy = clean + _audio(3, T, amp=0.02, seed=9)
    cleaned, cm, x, mask = audio.denoise_fused(model, 16, 12, torch.from_numpy(noisy))
    z = ref_stft(noisy)
    assert _maxdiff("x", x.numpy() + audio.STFT_MAG_MEAN, np.abs(z)) <= ATOL_SPEC
    assert torch.equal(mask, model.forward_float(x))
    m = mask.numpy().astype(np.float64)
    want = ref_istft(z * (1.0 + m))
    assert _maxdiff("cleaned", cleaned.numpy(), want) <= ATOL_AUDIO
    assert _maxdiff("cleaned_mag", cm.numpy(), np.abs(z) * (1.0 + m)) <= ATOL_SPEC
    loss, score = audio.validate_batch(model, 16, 12, torch.from_numpy(noisy), torch.from_numpy(clean))
    si = ref_si_snr(want[:, :T], clean.astype(np.float64))
    ls = 0.001 * ((np.abs(z) * (1.0 + m) - np.abs(ref_stft(clean))) ** 2).mean(axis=(1, 2)) + (100.0 - si)
    assert score.shape == loss.shape == (3,)
    assert _maxdiff("si_snr", score.numpy(), si) <= 1e-4 and _maxdiff("loss", loss.numpy(), ls) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
GPU_CASES = [(3, T, amp) for T in SIZES for amp in (1.0, 0.02)] + [(2, 480000, 1.0), (2, 480000, 0.02)]


def _ids(c):
    return f"B{c[0]}-T{c[1]}-amp{c[2]}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=_ids)
def test_stft_mag(case):
    import torch
    from sparsernns_amd import audio
    B, T, amp = case
    a = _audio(B, T, amp, seed=T)
    z = ref_stft(a)
    ad = torch.from_numpy(a).cuda()
    x, spec = audio.stft_mag(ad, spectrum=True)
    assert tuple(x.shape) == z.shape == tuple(spec.shape)
    assert _maxdiff("x + sub", x.cpu().numpy().astype(np.float64) + audio.STFT_MAG_MEAN, np.abs(z)) <= ATOL_SPEC * amp
    assert _maxdiff("spec", spec.cpu().numpy(), z) <= ATOL_SPEC * amp
    mag = audio.stft_mag(ad, sub=0.0)
    assert _maxdiff("mag", mag.cpu().numpy(), np.abs(z)) <= ATOL_SPEC * amp
    assert torch.equal(audio.stft_mag(ad), x)  # with and without the spectrum plane
    # one sequence alone = the same row of the batch
    for b in range(B):
        assert torch.equal(audio.stft_mag(ad[b:b + 1]), x[b:b + 1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        xs = audio.stft_mag(ad)
    s.synchronize()
    assert torch.equal(xs, x)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=_ids)
def test_mask_istft(case):
    import torch
    from sparsernns_amd import audio
    B, T, amp = case
    a, m = _audio(B, T, amp, seed=T + 1), _mask(B, T)
    z = ref_stft(a)
    ad, md = torch.from_numpy(a).cuda(), torch.from_numpy(m).cuda()
    out, cm = audio.mask_istft(ad, md, cleaned_mag=True)
    want = ref_istft(z * (1.0 + m))
    assert tuple(out.shape) == want.shape == (B, (z.shape[1] - 1) * 128)
    assert _maxdiff("cleaned", out.cpu().numpy(), want) <= ATOL_AUDIO * amp
    assert _maxdiff("cleaned_mag", cm.cpu().numpy(), np.abs(z) * (1.0 + m)) <= ATOL_SPEC * amp
    # no atomics: the same bits twice, with and without the magnitude plane, alone and in a batch
    out2, cm2 = audio.mask_istft(ad, md, cleaned_mag=True)
    assert torch.equal(out, out2) and torch.equal(cm, cm2) and torch.equal(audio.mask_istft(ad, md), out)
    assert torch.equal(audio.mask_istft(ad[1:2], md[1:2]), out[1:2])
    # NULL mask: the round trip; the tail beyond T is the zero padding
    rt = audio.mask_istft(ad, None).cpu().numpy()
    assert _maxdiff("round trip", rt, ref_istft(z)) <= ATOL_AUDIO * amp
    assert _maxdiff("round trip vs input", rt[:, :T], a.astype(np.float64)) <= ATOL_AUDIO * amp
    assert np.abs(rt[:, T:]).max(initial=0.0) <= ATOL_AUDIO * amp
    assert torch.equal(audio.mask_istft(ad, torch.zeros_like(md)), audio.mask_istft(ad, None))
    # the |Z| inside mask_istft is stft_mag's, bit for bit
    _, cm0 = audio.mask_istft(ad, None, cleaned_mag=True)
    assert torch.equal(cm0, audio.stft_mag(ad, sub=0.0))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        outs = audio.mask_istft(ad, md)
    s.synchronize()
    assert torch.equal(outs, out)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [777, 4096])
def test_mask_istft_negative_factor(T):
    """1 + mask in [-1.5, -0.5]: scaling the complex value is polar(|Z| * (1 + mask), angle) with a negative magnitude."""
    import torch
    from sparsernns_amd import audio
    a, m = _audio(3, T, seed=21), _mask(3, T, -2.5, -1.5)
    z = ref_stft(a)
    out, cm = audio.mask_istft(torch.from_numpy(a).cuda(), torch.from_numpy(m).cuda(), cleaned_mag=True)
    polar = np.abs(z) * (1.0 + m) * np.exp(1j * np.angle(z))
    assert _maxdiff("cleaned", out.cpu().numpy(), ref_istft(polar)) <= ATOL_AUDIO
    assert _maxdiff("cleaned_mag", cm.cpu().numpy(), np.abs(z) * (1.0 + m)) <= ATOL_SPEC
    assert (cm <= 0).all()


@pytest.mark.gpu
def test_all_zero_audio():
    import torch
    from sparsernns_amd import audio
    ad = torch.zeros(3, 5000, device="cuda")
    md = torch.from_numpy(_mask(3, 5000)).cuda()
    out, cm = audio.mask_istft(ad, md, cleaned_mag=True)
    x, spec = audio.stft_mag(ad, sub=0.0, spectrum=True)
    for t in (out, cm, x, spec.real, spec.imag):
        assert torch.count_nonzero(t) == 0  # exactly 0: NaN counts as nonzero


def _model(dim_scale):
    from sparsernns_amd.fxpmodel import build_regression_model
    md, qc, dims = synth.make_model(dim_scale, calib_L=128)
    return build_regression_model(md, qc, dims["n_layers"]), qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]


def _oracle_mask(model, x, ib, ie):
    fx = O.from_fp(x, ib, ie, True, O.FLOOR)
    ref, _, re_, _ = cref.CModel(model.export()).forward(fx.data, fx.bits, fx.exp)
    return fx.data, ref.astype(np.float32) / np.float32(1 << re_)


@pytest.mark.gpu
@pytest.mark.parametrize("dim_scale", [0.5, 0.25])
def test_denoise_fused(dim_scale):
    """The middle is exact: mask = the CPU oracle's forward of the FLOOR-quantised x the kernel produced.  The ends are within
    the file's tolerance of the restatement at the input's amplitude, 0.02 (the synthetic models' |1 + mask| reaches 2.8 and
    4.3; the bound is not widened for it).

    Against audio.denoise (rocFFT + torch ops) nothing is bit-identical: the two |Z| differ in their last bits and FLOOR turns
    some of that into one input LSB (the count is printed, not asserted).  Bound on the outputs: both sides' tolerance against
    the restatement, plus the effect of those flips measured through the oracle and the float64 restatement."""
    import torch
    from sparsernns_amd import audio
    model, ib, ie = _model(dim_scale)
    amp = 0.02
    noisy = (amp * torch.randn(2, 128 * 63, generator=torch.Generator().manual_seed(5))).cuda()
    cleaned, cm, x, mask = audio.denoise_fused(model, ib, ie, noisy)
    a = noisy.cpu().numpy()
    z = ref_stft(a)
    assert _maxdiff("x + sub", x.cpu().numpy().astype(np.float64) + audio.STFT_MAG_MEAN, np.abs(z)) <= ATOL_SPEC * amp
    xi, mref = _oracle_mask(model, x.cpu().numpy(), ib, ie)
    assert np.array_equal(mask.cpu().numpy(), mref)
    m = mref.astype(np.float64)
    print(f"max |1 + mask| = {np.abs(1.0 + m).max():.3f}")
    want = ref_istft(z * (1.0 + m))
    assert _maxdiff("cleaned", cleaned.cpu().numpy(), want) <= ATOL_AUDIO * amp
    assert _maxdiff("cleaned_mag", cm.cpu().numpy(), np.abs(z) * (1.0 + m)) <= ATOL_SPEC * amp

    c_t, cm_t, mag_t = audio.denoise(model, ib, ie, noisy)
    x_t = (mag_t - audio.STFT_MAG_MEAN).transpose(-1, -2).contiguous().cpu().numpy()
    xi_t, mref_t = _oracle_mask(model, x_t, ib, ie)
    print(f"input words that differ between the two routes: {np.count_nonzero(xi != xi_t)} of {xi.size}, "
          f"max |mask difference| = {np.abs(mref - mref_t).max():.3e}")
    m_t = mref_t.astype(np.float64)
    flips_audio = float(np.abs(want - ref_istft(z * (1.0 + m_t))).max())
    flips_mag = float((np.abs(z) * np.abs(m - m_t)).max())
    assert _maxdiff("x vs denoise", x.cpu().numpy(), x_t.astype(np.float64)) <= 2 * ATOL_SPEC * amp
    assert _maxdiff("cleaned vs denoise", cleaned.cpu().numpy(), c_t.cpu().numpy().astype(np.float64)) \
        <= 2 * ATOL_AUDIO * amp + flips_audio
    assert _maxdiff("cleaned_mag vs denoise", cm.cpu().numpy(), cm_t.transpose(-1, -2).cpu().numpy().astype(np.float64)) \
        <= 2 * ATOL_SPEC * amp + flips_mag


@pytest.mark.gpu
def test_validate_batch():
    """si_snr and loss against a float64 evaluation of fxprun.py:79-88 on the device's own mask, atol 1e-3 (dB).
    Measured on the MI355X: si_snr differs by 2.9e-7 dB and loss by 1.0e-6 (si_snr -1.35 and -0.36 dB)."""
    import torch
    from sparsernns_amd import audio
    model, ib, ie = _model(0.5)
    T = 128 * 63
    clean = _audio(2, T, amp=0.05, seed=30)
    noisy = clean + _audio(2, T, amp=0.02, seed=31)
    nd, cd = torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()
    loss, score = audio.validate_batch(model, ib, ie, nd, cd)
    mask = audio.denoise_fused(model, ib, ie, nd)[3].cpu().numpy().astype(np.float64)
    z = ref_stft(noisy)
    cleaned = ref_istft(z * (1.0 + mask))
    si = ref_si_snr(cleaned[:, :T], clean.astype(np.float64))
    ls = 0.001 * ((np.abs(z) * (1.0 + mask) - np.abs(ref_stft(clean))) ** 2).mean(axis=(1, 2)) + (100.0 - si)
    print("si_snr (dB):", si)
    assert tuple(score.shape) == tuple(loss.shape) == (2,)
    assert _maxdiff("si_snr", score.cpu().numpy(), si) <= 1e-3
    assert _maxdiff("loss", loss.cpu().numpy(), ls) <= 1e-3
