"""The audio kernels either side of the model (s5fxp_stft_mag, s5fxp_mask_istft, s5fxp_mask_istft_score and their _clips
forms) at B x T where the (B, frames, 257) float planes pass 2^32 bytes -- 4.2 M frames, 2.1 GB of audio.  Audio, clean audio
and masks repeat with period R = 7; T gives 4099 frames per clip, a prime.  Every output is bit for bit the R-clip launch's,
which tests/test_audio_kernels.py, test_audio_score.py and the _clips suites hold to the float64 restatement.
"""
import functools
import time

import numpy as np
import pytest

import large_extents as LX
from large_extents import P32, R

pytestmark = pytest.mark.gpu

HOP, NFFT, BINS = 128, 512, 257
T = HOP * 4097 + 37   # 4099 frames
FRAMES = -(-T // HOP) + 1
SENT = -123.5


def _report(name, t0, **figures):
    print(f"[large] {name}: {time.perf_counter() - t0:.2f} s " + " ".join(f"{k}={v}" for k, v in figures.items()), flush=True)


@functools.lru_cache(maxsize=None)
def _small():
    """(noisy, clean, mask) of the R clips, host arrays, never modified."""
    rng = np.random.Generator(np.random.PCG64(2049))
    clean = (0.1 * rng.standard_normal((R, T))).astype(np.float32)
    noisy = (clean + 0.05 * rng.standard_normal((R, T))).astype(np.float32)
    mask = rng.uniform(-0.9, 0.4, (R, FRAMES, BINS)).astype(np.float32)
    return noisy, clean, mask


def _dev(a):
    import torch
    return torch.from_numpy(a).cuda()


def _batch():
    B = R * (P32 // (R * FRAMES * BINS * 4) + 1)
    assert FRAMES == 4099 and B * FRAMES * BINS * 4 > P32 and (B - R) * FRAMES * BINS * 4 <= P32
    return B


def test_stft_mag_past_2_32_bytes():
    import torch
    from sparsernns_amd import audio

    t0 = time.perf_counter()
    B = _batch()
    plane = B * FRAMES * BINS * 4
    LX.memory_guard(B * T * 4 + 3 * plane + LX.COPIES_PER_CHUNK * R * FRAMES * BINS * 2, "stft_mag")
    a_s = _dev(_small()[0])
    x_s, z_s = audio.stft_mag(a_s, spectrum=True)
    x, z = audio.stft_mag(LX.repeated(a_s, B // R), spectrum=True)
    torch.cuda.synchronize()
    assert x.shape == (B, FRAMES, BINS) and float(x_s.abs().max()) > 0
    LX.assert_repeats(x, x_s, "stft_mag x")
    LX.assert_repeats(torch.view_as_real(z), torch.view_as_real(z_s), "stft_mag spectrum")
    _report("stft_mag", t0, B=B, frames=B * FRAMES, x_bytes=plane, spectrum_bytes=2 * plane)
    del x, z
    LX.release()


def test_mask_istft_past_2_32_bytes():
    import torch
    from sparsernns_amd import audio

    t0 = time.perf_counter()
    B = _batch()
    plane = B * FRAMES * BINS * 4
    LX.memory_guard(2 * B * T * 4 + 2 * plane + LX.COPIES_PER_CHUNK * R * FRAMES * BINS, "mask_istft")
    a_s, m_s = _dev(_small()[0]), _dev(_small()[2])
    o_s, c_s = audio.mask_istft(a_s, m_s, cleaned_mag=True)
    o, c = audio.mask_istft(LX.repeated(a_s, B // R), LX.repeated(m_s, B // R), cleaned_mag=True)
    torch.cuda.synchronize()
    assert o.shape == (B, (FRAMES - 1) * HOP) and float(o_s.abs().max()) > 0
    LX.assert_repeats(o, o_s, "mask_istft audio")
    LX.assert_repeats(c, c_s, "mask_istft cleaned_mag")
    _report("mask_istft", t0, B=B, mask_bytes=plane, out_bytes=o.numel() * 4)
    del o, c
    LX.release()


def test_mask_istft_score_past_2_32_bytes():
    import torch
    from sparsernns_amd import audio

    t0 = time.perf_counter()
    B = _batch()
    plane = B * FRAMES * BINS * 4
    LX.memory_guard(3 * B * T * 4 + 2 * plane + LX.COPIES_PER_CHUNK * R * FRAMES * BINS, "mask_istft_score")
    a_s, cl_s, m_s = (_dev(v) for v in _small())
    small = audio.score_fused(a_s, cl_s, m_s, cleaned=True, cleaned_mag=True)
    k = B // R
    big = audio.score_fused(LX.repeated(a_s, k), LX.repeated(cl_s, k), LX.repeated(m_s, k), cleaned=True, cleaned_mag=True)
    torch.cuda.synchronize()
    for name, b, s in zip(("loss", "si_snr", "mag_mse", "cleaned", "cleaned_mag"), big, small):
        assert bool(torch.isfinite(s).all())
        LX.assert_repeats(b, s, f"score {name}")
    # the scores alone, no plane stored: the same bits
    for b, s in zip(audio.score_fused(LX.repeated(a_s, k), LX.repeated(cl_s, k), LX.repeated(m_s, k)), small[:3]):
        LX.assert_repeats(b, s, "score without planes")
    _report("mask_istft_score", t0, B=B, mask_bytes=plane)
    del big, b
    LX.release()


CLIP_T = (T, 0, NFFT - 1, NFFT, T + 1000, 300001)   # cycled; the fifth is clamped to Tmax


def test_clip_forms_past_2_32_bytes():
    """s5fxp_stft_mag_clips, s5fxp_mask_istft_clips and s5fxp_mask_istft_score_clips on n clips padded to T samples, lengths
    cycling through CLIP_T and contents through the 7 clips (period 42): planes -- padding keeps its sentinel -- lens and
    scores bit for bit the 42-clip launch's."""
    import torch
    from sparsernns_amd import audio

    t0 = time.perf_counter()
    period = R * len(CLIP_T)
    k = P32 // (period * FRAMES * BINS * 4) + 1
    n = k * period
    plane = n * FRAMES * BINS * 4
    assert plane > P32
    LX.memory_guard(2 * n * T * 4 + 6 * plane + LX.COPIES_PER_CHUNK * period * FRAMES * BINS * 2, "audio clip forms")
    idx = torch.arange(period, device="cuda") % R
    a_s, cl_s, m_s = (_dev(v)[idx].contiguous() for v in _small())
    smp_s = torch.tensor([CLIP_T[e % len(CLIP_T)] for e in range(period)], dtype=torch.int32, device="cuda")
    full = lambda m, *shape, dtype=torch.float32: torch.full((m,) + shape, SENT, dtype=dtype, device="cuda")
    f_outs = lambda m: [full(m, FRAMES, BINS), torch.full((m,), -5, dtype=torch.int32, device="cuda"),
                        full(m, FRAMES, BINS, dtype=torch.complex64)]
    i_outs = lambda m: [full(m, (FRAMES - 1) * HOP), full(m, FRAMES, BINS)]

    def run(a, cl, m, smp):
        cnt = a.shape[0]
        x, lens, z = audio.stft_mag_clips(a, smp, spectrum=True, out=f_outs(cnt))
        o, c = audio.mask_istft_clips(a, smp, m, cleaned_mag=True, out=i_outs(cnt))
        sc = audio.score_clips(a, cl, smp, m, cleaned=True, cleaned_mag=True, out=i_outs(cnt))
        return dict(x=x, lens=lens, spectrum=torch.view_as_real(z), audio=o, cleaned_mag=c, loss=sc[0], si_snr=sc[1], mag_mse=sc[2],
                    scored_audio=sc[3], scored_mag=sc[4])

    small = run(a_s, cl_s, m_s, smp_s)
    lens = small["lens"].cpu().numpy()
    want = [0 if t < NFFT else -(-min(t, T) // HOP) + 1 for t in smp_s.tolist()]
    assert lens.tolist() == want and max(want) == FRAMES
    assert bool((small["x"][1] == SENT).all()) and bool((small["x"][3, 5:] == SENT).all())   # the padding was left alone
    big = run(LX.repeated(a_s, k), LX.repeated(cl_s, k), LX.repeated(m_s, k), LX.repeated(smp_s, k))
    torch.cuda.synchronize()
    for name in small:
        LX.assert_repeats(big[name], small[name], f"clips {name}")
    _report("audio_clips", t0, n=n, plane_bytes=plane)
    del big, small
    LX.release()
