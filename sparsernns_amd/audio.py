"""The steps either side of the model in the reference's N-DNS denoising loop, on the device.

Reference: ``sparseRNNs/train_helpers.py:1382-1412`` (``stft_splitter`` / ``stft_mixer``: ``jax.scipy.signal.stft`` /
``istft`` with nperseg = nfft = 512, hop 128, boxcar window, one-sided, the SciPy defaults ``boundary="zeros"``,
``padded=True``, ``scaling="spectrum"``), ``:15-53`` (``si_snr_jax``) and ``sparseRNNs/fxprun.py:63-88`` (the
validation step that strings them together around ``model(fxp_x)``).

Everything here is plain torch tensor code (rocFFT does the transforms on a ROCm device), so the whole
STFT -> fixed-point model -> iSTFT -> SI-SNR chain stays in HBM.  ``jax.scipy.signal`` mirrors ``scipy.signal``, which is
importable here: ``tests/test_cpu_suite.py`` checks these functions against it.
"""
from __future__ import annotations

import numpy as np
import torch

NFFT = 512
HOP = 128
STFT_MAG_MEAN = 0.0007  # fxprun.py:65


def _frames(x: torch.Tensor) -> torch.Tensor:
    """scipy.signal.stft's segmentation: 256 zeros each side (boundary="zeros"), zero padding at the end to a whole
    number of hops (padded=True), then windows of 512 every 128 samples.  (..., T) -> (..., n_seg, 512)"""
    x = torch.nn.functional.pad(x, (NFFT // 2, NFFT // 2))
    nadd = (-(x.shape[-1] - NFFT) % HOP) % NFFT
    if nadd:
        x = torch.nn.functional.pad(x, (0, nadd))
    return x.unfold(-1, NFFT, HOP)


def stft(audio: torch.Tensor) -> torch.Tensor:
    """Complex one-sided STFT, (..., T) -> (..., 257, n_seg), scaled by 1/sum(window) = 1/512 ("spectrum")."""
    seg = _frames(audio.to(torch.float32))
    z = torch.fft.rfft(seg, n=NFFT, dim=-1) / NFFT
    return z.transpose(-1, -2)


def stft_splitter(audio: torch.Tensor):
    """train_helpers.py:1382-1396: magnitude and phase, each (..., 257, n_seg)."""
    z = stft(audio)
    return z.abs(), z.angle()


def istft(z: torch.Tensor) -> torch.Tensor:
    """scipy.signal.istft for the same parameters: (..., 257, n_seg) -> (..., (n_seg - 1) * 128)."""
    seg = torch.fft.irfft(z.transpose(-1, -2), n=NFFT, dim=-1) * NFFT  # (..., n_seg, 512), undo the spectrum scaling
    n_seg = seg.shape[-2]
    total = NFFT + HOP * (n_seg - 1)
    lead = seg.shape[:-2]
    flat = seg.reshape(-1, n_seg, NFFT)
    # overlap-add; with the boxcar window the normaliser is the number of windows that cover a sample
    idx = (torch.arange(n_seg, device=seg.device)[:, None] * HOP + torch.arange(NFFT, device=seg.device)[None, :]).reshape(-1)
    out = torch.zeros(flat.shape[0], total, dtype=seg.dtype, device=seg.device)
    out.index_add_(1, idx, flat.reshape(flat.shape[0], -1))
    norm = torch.zeros(total, dtype=seg.dtype, device=seg.device)
    norm.index_add_(0, idx, torch.ones_like(idx, dtype=seg.dtype))
    out = out / torch.where(norm > 1e-10, norm, torch.ones_like(norm))
    return out[:, NFFT // 2: total - NFFT // 2].reshape(*lead, -1)


def stft_mixer(stft_mag: torch.Tensor, stft_angle: torch.Tensor) -> torch.Tensor:
    """train_helpers.py:1399-1412."""
    return istft(torch.polar(stft_mag.to(torch.float32), stft_angle.to(torch.float32)))


def si_snr(target: torch.Tensor, estimate: torch.Tensor) -> torch.Tensor:
    """train_helpers.py:15-53 (last dimension = time)."""
    eps = 1e-8
    s_t = target - target.mean(dim=-1, keepdim=True)
    s_e = estimate - estimate.mean(dim=-1, keepdim=True)
    dot = (s_t * s_e).sum(dim=-1, keepdim=True)
    proj = dot * s_t / (s_t ** 2).sum(dim=-1, keepdim=True)
    noise = s_e - proj
    sdr = (proj ** 2).sum(dim=-1) / ((noise ** 2).sum(dim=-1) + eps)
    return 10.0 * torch.log10(sdr + eps)


def _takes(model, inp_bits: int, inp_exp: int) -> bool:
    """forward_float quantises to the encoder's input configuration: the float route applies when that is what was asked."""
    q = getattr(model, "fxp_qconfig", None)
    try:
        return (int(q["encoder"]["inp_bits"]), int(q["encoder"]["inp_exp"])) == (int(inp_bits), int(inp_exp))
    except (TypeError, KeyError):
        return False


def denoise(model, inp_bits: int, inp_exp: int, noisy: torch.Tensor):
    """fxprun.py:63-78: noisy audio (B, T) -> (cleaned audio, cleaned magnitude, noisy magnitude).

    ``model`` is an ``FxpRegressionModel`` (or anything callable FxpArray -> FxpArray with ``to_float``).  A model with
    ``forward_float`` whose encoder takes (inp_bits, inp_exp) runs the quantisation, the forward and to_float in one engine
    call (s5fxp_model_forward_f32, bit for bit the same mask), unless it stores intermediates (the op-by-op path)."""
    from .fxparray import RoundingMode, fxp_from_fp

    mag, phase = stft_splitter(noisy)
    x = (mag - STFT_MAG_MEAN).transpose(-1, -2).contiguous()  # (B, n_seg, 257)
    if hasattr(model, "forward_float") and not getattr(model, "store_intermediates", False) and _takes(model, inp_bits, inp_exp):
        mask = model.forward_float(x).transpose(-1, -2)
    else:
        fx = fxp_from_fp(x, bits=inp_bits, exp=inp_exp, signed=True, round_mode=RoundingMode.FLOOR)
        mask = model(fx).to_float().transpose(-1, -2)
    cleaned_mag = mag * (1.0 + mask)
    return stft_mixer(cleaned_mag, phase), cleaned_mag, mag


# ---------------------------------------------------------------------------------------------------------------------
# The same loop on the HIP kernels of csrc/audio_stft.hpp (s5fxp_stft_mag / s5fxp_mask_istft).  Everything below is
# frame-major, (B, n_seg, 257): the rows the model's encoder streams, so no transpose pass exists; the reference's
# (B, 257, n_seg) is ``.transpose(-1, -2)`` of it.  CUDA tensors go to the kernels on the current stream; CPU tensors take
# the torch functions above, arranged frame-major.
# ---------------------------------------------------------------------------------------------------------------------
def stft_frames(T: int) -> int:
    """Frames of a T-sample signal, ceil(T / 128) + 1.  Below 512 samples scipy changes nperseg: not supported."""
    if T < NFFT:
        raise NotImplementedError(f"stft needs at least {NFFT} samples, got {T}")
    return -(-T // HOP) + 1


def _audio2d(audio: torch.Tensor) -> torch.Tensor:
    if audio.dim() != 2:
        raise ValueError(f"audio must be (B, T), got {tuple(audio.shape)}")
    return audio.to(torch.float32).contiguous()


def _stft_launch(audio: torch.Tensor, n_seg: int, dtype: torch.dtype, spectrum: bool, entry: str, *extra):
    """The GPU route of ``stft_mag`` / ``stft_mag_i16``: audio (B, T) float32 on a GPU -> x (B, n_seg, 257) of `dtype` (and the
    complex64 spectrum) from one launch of `entry`, whose arguments between T and x are `extra`."""
    from . import _lib
    B, T = audio.shape
    shape = (B, n_seg, NFFT // 2 + 1)
    x = torch.empty(shape, dtype=dtype, device=audio.device)
    spec = torch.empty(shape, dtype=torch.complex64, device=audio.device) if spectrum else None
    with torch.cuda.device(audio.device):
        _lib.check(getattr(_lib.lib, entry)(audio.data_ptr(), B, T, *extra, x.data_ptr(), spec.data_ptr() if spectrum else None,
                                            torch.cuda.current_stream().cuda_stream), entry)
    return (x, spec) if spectrum else x


def _istft_launch(audio: torch.Tensor, n_seg: int, cleaned_mag: bool, entry: str, *mask):
    """The GPU route of ``mask_istft`` / ``mask_istft_i16``: one launch of `entry`, whose arguments between audio and B are
    `mask`."""
    from . import _lib
    B, T = audio.shape
    out = torch.empty(B, (n_seg - 1) * HOP, dtype=torch.float32, device=audio.device)
    cm = torch.empty((B, n_seg, NFFT // 2 + 1), dtype=torch.float32, device=audio.device) if cleaned_mag else None
    with torch.cuda.device(audio.device):
        _lib.check(getattr(_lib.lib, entry)(audio.data_ptr(), *mask, B, T, out.data_ptr(), cm.data_ptr() if cleaned_mag else None,
                                            torch.cuda.current_stream().cuda_stream), entry)
    return (out, cm) if cleaned_mag else out


def stft_mag(audio: torch.Tensor, sub: float = STFT_MAG_MEAN, spectrum: bool = False):
    """audio (B, T) -> x = |Z| - sub, (B, n_seg, 257) float32 (fxprun.py:64-65: the model's input rows); with ``spectrum``
    also the complex64 spectrum Z, same shape."""
    audio = _audio2d(audio)
    n_seg = stft_frames(audio.shape[1])
    if not audio.is_cuda:
        z = stft(audio).transpose(-1, -2).contiguous()
        x = z.abs() - sub
        return (x, z) if spectrum else x
    return _stft_launch(audio, n_seg, torch.float32, spectrum, "s5fxp_stft_mag", float(sub))


def mask_istft(audio: torch.Tensor, mask, cleaned_mag: bool = False):
    """fxprun.py:76-78: the spectrum of ``audio`` (B, T) times 1 + mask (B, n_seg, 257), back to audio
    (B, (n_seg - 1) * 128); with ``cleaned_mag`` also |Z| * (1 + mask).  ``mask=None`` is the plain round trip.  The complex
    value is scaled, which is polar(|Z| * (1 + mask), angle(Z)) for either sign of 1 + mask."""
    audio = _audio2d(audio)
    B, T = audio.shape
    n_seg = stft_frames(T)
    shape = (B, n_seg, NFFT // 2 + 1)
    if mask is not None:
        if tuple(mask.shape) != shape or mask.device != audio.device:
            raise ValueError(f"mask must be {shape} on {audio.device}, got {tuple(mask.shape)} on {mask.device}")
        mask = mask.to(torch.float32).contiguous()
    if not audio.is_cuda:
        z = stft(audio).transpose(-1, -2)
        f = 1.0 + mask if mask is not None else torch.ones(shape, dtype=torch.float32)
        out = istft((z * f).transpose(-1, -2))
        return (out, z.abs() * f) if cleaned_mag else out
    return _istft_launch(audio, n_seg, cleaned_mag, "s5fxp_mask_istft", mask.data_ptr() if mask is not None else None)


def _int16_range(bits: int, exp: int, what: str) -> None:
    if not 1 <= int(bits) <= 16 or not 0 <= int(exp) <= 31:
        raise ValueError(f"{what}: bits must be 1..16 and the exponent 0..31, got ({bits}, {exp})")


def stft_mag_i16(audio: torch.Tensor, x_bits: int, x_exp: int, sub: float = STFT_MAG_MEAN, spectrum: bool = False):
    """``stft_mag`` with the model's int16 boundary: x = fxp_from_fp(|Z| - sub, FLOOR) at (x_bits <= 16, x_exp) as an int16
    tensor (B, n_seg, 257) -- exactly ``fxp_from_fp(stft_mag(audio, sub), bits=x_bits, exp=x_exp, FLOOR).data`` in half the
    bytes of the float rows, which are never written."""
    _int16_range(x_bits, x_exp, "stft_mag_i16")
    audio = _audio2d(audio)
    n_seg = stft_frames(audio.shape[1])
    if not audio.is_cuda:
        r = stft_mag(audio, sub, spectrum)
        xf, z = r if spectrum else (r, None)
        # fxp_from_fp with FLOOR (fxparray.py:287-307) in torch: the scale is a power of two, so the float32 product is exact
        hi = float((1 << (int(x_bits) - 1)) - 1)
        q = torch.floor(xf * float(2.0 ** int(x_exp)))
        x = torch.nan_to_num(q, nan=0.0, posinf=hi, neginf=-hi - 1.0).clamp(-hi - 1.0, hi).to(torch.int16)
        return (x, z) if spectrum else x
    return _stft_launch(audio, n_seg, torch.int16, spectrum, "s5fxp_stft_mag_i16", float(sub), int(x_bits), int(x_exp))


def mask_istft_i16(audio: torch.Tensor, mask: torch.Tensor, mask_exp: int, cleaned_mag: bool = False):
    """``mask_istft`` for a mask as the model's decoder leaves it: int16 (B, n_seg, 257) at ``mask_exp``.  The factor is
    1 + to_float(mask), so the results are bit for bit ``mask_istft(audio, FxpArray(mask, 16, mask_exp).to_float())``."""
    _int16_range(16, mask_exp, "mask_istft_i16")
    audio = _audio2d(audio)
    B, T = audio.shape
    n_seg = stft_frames(T)
    shape = (B, n_seg, NFFT // 2 + 1)
    if mask.dtype != torch.int16 or tuple(mask.shape) != shape or mask.device != audio.device:
        raise ValueError(f"mask must be int16 {shape} on {audio.device}, got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
    mask = mask.contiguous()
    if not audio.is_cuda:
        return mask_istft(audio, torch.ldexp(mask.to(torch.float32), torch.tensor(-int(mask_exp))), cleaned_mag)
    return _istft_launch(audio, n_seg, cleaned_mag, "s5fxp_mask_istft_i16", mask.data_ptr(), int(mask_exp))


def _forward_at(model, x: torch.Tensor, inp_bits: int, inp_exp: int, exps) -> torch.Tensor:
    """The model on the rows x (float32 or int16) at stated exponents: ``Engine.forward_float`` / ``forward_int16`` with ``exps=``.
    There is no 32-bit fallback at stated exponents, so the model needs its fused engine."""
    if not hasattr(model, "engine") or getattr(model, "store_intermediates", False):
        raise ValueError("stated exponents need a model with a fused engine that does not store intermediates")
    eng = model.engine()
    run = eng.forward_int16 if x.dtype == torch.int16 else eng.forward_float
    return run(x, inp_bits, inp_exp, exps=exps)


def denoise_fused(model, inp_bits: int, inp_exp: int, noisy: torch.Tensor, boundary: str = "float32", exps=None):
    """fxprun.py:63-78 as stft_mag -> model -> mask_istft: noisy audio (B, T) -> (cleaned audio, cleaned magnitude, x, mask),
    the last three (B, n_seg, 257).  On a GPU that is two launches plus the forward.

    boundary="int16": the rows cross the model's boundary as int16 (stft_mag_i16 -> model.forward_int16 -> mask_istft_i16), 2
    bytes per value instead of 4, and ``x`` / ``mask`` come back as int16 tensors at (inp_bits, inp_exp) / the model's output
    exponent.  The cleaned audio and magnitude are bit for bit the default route's: float32 restates the same 16-bit integers.
    It needs a model with ``forward_int16`` (and ``engine()`` or an ``out_exp`` attribute) and an output of at most 16 bits;
    a model that stores intermediates (the op-by-op path, which the default route takes for it) is refused with ValueError.

    NOT bit-identical to ``denoise``: two FFT implementations differ in the last bits of |Z|, and the FLOOR quantiser turns a
    few of those differences into one LSB of the model's input.  The model itself stays exact on the ``x`` returned here.

    exps: an (n_layers, 5) array of stated exponents (``Engine.calibrate_exps``) runs the model's batch forward at them
    (``Engine.enqueue(..., exps=)``): every sequence gets the mask ``denoise_clips(..., exps=)`` gives it alone, on the whole
    chip.  None: the forward on the batch's own exponents, as it always was."""
    from .fxparray import RoundingMode, fxp_from_fp

    if boundary not in ("float32", "int16"):
        raise ValueError(f'boundary must be "float32" or "int16", got {boundary!r}')
    if boundary == "int16":
        if getattr(model, "store_intermediates", False):
            raise ValueError("a model that stores intermediates runs op by op on FxpArrays: use the float32 boundary")
        x = stft_mag_i16(noisy, inp_bits, inp_exp)
        mask = model.forward_int16(x, inp_bits, inp_exp) if exps is None else _forward_at(model, x, inp_bits, inp_exp, exps)
        out_exp = model.out_exp if hasattr(model, "out_exp") else model.engine().out_exp
        cleaned, cleaned_mag = mask_istft_i16(noisy, mask, out_exp, cleaned_mag=True)
        return cleaned, cleaned_mag, x, mask
    x = stft_mag(noisy)
    if exps is not None:
        mask = _forward_at(model, x, inp_bits, inp_exp, exps)
    elif hasattr(model, "forward_float") and not getattr(model, "store_intermediates", False) and _takes(model, inp_bits, inp_exp):
        mask = model.forward_float(x)
    else:
        fx = fxp_from_fp(x, bits=inp_bits, exp=inp_exp, signed=True, round_mode=RoundingMode.FLOOR)
        mask = model(fx).to_float()
    cleaned, cleaned_mag = mask_istft(noisy, mask, cleaned_mag=True)
    return cleaned, cleaned_mag, x, mask


# ---------------------------------------------------------------------------------------------------------------------
# The same loop for n clips of DIFFERENT lengths: s5fxp_stft_mag_clips -> s5fxp_model_clips_f32 -> s5fxp_mask_istft_clips, one
# launch each.  Clip e is row e of audio (n, Tmax) with T_e = clamp(samples[e], 0, Tmax) samples; every row tensor is padded to
# Lmax = stft_frames(Tmax) frames.  A clip below 512 samples has no frames (lens[e] = 0) and nothing of it is written.
# ---------------------------------------------------------------------------------------------------------------------
def _clips_args(audio: torch.Tensor, samples: torch.Tensor):
    audio = _audio2d(audio)
    n, Tmax = audio.shape
    Lmax = stft_frames(Tmax)
    if n < 1:
        raise ValueError("a launch holds at least one clip")
    if samples.dtype != torch.int32 or tuple(samples.shape) != (n,) or samples.device != audio.device:
        raise ValueError(f"samples must be int32 ({n},) on {audio.device}, got {samples.dtype} {tuple(samples.shape)} on {samples.device}")
    return audio, samples.contiguous(), n, Tmax, Lmax


def _clips_out(given, want, what: str):
    """The caller's output tensors (`out=`), checked against want = [(shape, dtype, device), ...], or fresh ones."""
    if given is None:
        return [torch.empty(shape, dtype=dtype, device=dev) for shape, dtype, dev in want]
    given = list(given)
    if len(given) != len(want):
        raise ValueError(f"{what}: out must hold {len(want)} tensors, got {len(given)}")
    for t, (shape, dtype, dev) in zip(given, want):
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{what}: out needs a contiguous {dtype} {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return given


def _clip_lengths(samples: torch.Tensor, Tmax: int):
    """Host copies of (T_e, len_e) as the kernels derive them."""
    T = [min(max(int(v), 0), Tmax) for v in samples.tolist()]
    return T, [0 if t < NFFT else -(-t // HOP) + 1 for t in T]


def stft_mag_clips(audio: torch.Tensor, samples: torch.Tensor, sub: float = STFT_MAG_MEAN, spectrum: bool = False, out=None):
    """``stft_mag`` for n clips of different lengths in ONE launch: audio (n, Tmax) float32, padded; samples (n,) int32 on the
    audio's device -> (x, lens[, spec]): x (n, Lmax, 257) float32 with clip e in rows 0 .. lens[e]-1, lens (n,) int32 on the
    device -- what ``Engine.clips`` takes, with no host step in between -- and with ``spectrum`` the complex64 spectrum.  Rows
    x[e, :lens[e]] are bit for bit ``stft_mag(audio[e:e+1, :T_e])[0]``.  Rows from lens[e] on are never written (``out``: the
    tensors to write into, in the order returned; otherwise they are fresh and that padding is unspecified) and samples from
    T_e on never read.  A clip below 512 samples gets lens[e] = 0."""
    audio, samples, n, Tmax, Lmax = _clips_args(audio, samples)
    dev, shape = audio.device, (n, Lmax, NFFT // 2 + 1)
    res = _clips_out(out, [(shape, torch.float32, dev), ((n,), torch.int32, dev)] + ([(shape, torch.complex64, dev)] if spectrum else []),
                     "stft_mag_clips")
    x, lens, spec = res[0], res[1], res[2] if spectrum else None
    if not audio.is_cuda:
        T, L = _clip_lengths(samples, Tmax)
        for e in range(n):
            lens[e] = L[e]
            if L[e]:
                r = stft_mag(audio[e:e + 1, :T[e]], sub, spectrum)
                x[e, :L[e]] = r[0][0] if spectrum else r[0]
                if spectrum:
                    spec[e, :L[e]] = r[1][0]
        return tuple(res)
    from . import _lib
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.s5fxp_stft_mag_clips(audio.data_ptr(), n, Tmax, samples.data_ptr(), float(sub), x.data_ptr(),
                                                 spec.data_ptr() if spectrum else None, lens.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "s5fxp_stft_mag_clips")
    return tuple(res)


def mask_istft_clips(audio: torch.Tensor, samples: torch.Tensor, mask, cleaned_mag: bool = False, out=None):
    """``mask_istft`` for n clips of different lengths in ONE launch: audio, samples as ``stft_mag_clips``; mask (n, Lmax, 257)
    float32 (rows from len_e on are never read) or None (zeros) -> cleaned audio (n, (Lmax - 1) * 128), clip e in its first
    (len_e - 1) * 128 samples, bit for bit ``mask_istft(audio[e:e+1, :T_e], mask[e:e+1, :len_e])[0]``; with ``cleaned_mag`` also
    |Z| * (1 + mask), (n, Lmax, 257).  Nothing behind a clip's end is written (``out`` as in ``stft_mag_clips``)."""
    audio, samples, n, Tmax, Lmax = _clips_args(audio, samples)
    dev, shape = audio.device, (n, Lmax, NFFT // 2 + 1)
    if mask is not None:
        if tuple(mask.shape) != shape or mask.device != dev:
            raise ValueError(f"mask must be {shape} on {dev}, got {tuple(mask.shape)} on {mask.device}")
        mask = mask.to(torch.float32).contiguous()
    res = _clips_out(out, [((n, (Lmax - 1) * HOP), torch.float32, dev)] + ([(shape, torch.float32, dev)] if cleaned_mag else []),
                     "mask_istft_clips")
    o, cm = res[0], res[1] if cleaned_mag else None
    if not audio.is_cuda:
        T, L = _clip_lengths(samples, Tmax)
        for e in range(n):
            if L[e]:
                r = mask_istft(audio[e:e + 1, :T[e]], mask[e:e + 1, :L[e]] if mask is not None else None, cleaned_mag)
                o[e, :(L[e] - 1) * HOP] = r[0][0] if cleaned_mag else r[0]
                if cleaned_mag:
                    cm[e, :L[e]] = r[1][0]
        return (o, cm) if cleaned_mag else o
    from . import _lib
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.s5fxp_mask_istft_clips(audio.data_ptr(), mask.data_ptr() if mask is not None else None, n, Tmax,
                                                   samples.data_ptr(), o.data_ptr(), cm.data_ptr() if cleaned_mag else None,
                                                   torch.cuda.current_stream().cuda_stream), "s5fxp_mask_istft_clips")
    return (o, cm) if cleaned_mag else o


def _clips_front(model, inp_bits: int, inp_exp: int, clips, lane, exps=None):
    """What ``denoise_clips`` and ``validate_clips`` share in front of the inverse: the checks of the clip list, and on the
    one-launch route the padding, ``stft_mag_clips``, ``Engine.clips`` and the one read of the status words.  Returns
    (clips, front) with front = (audio, samples, x, mask, L) -- padded tensors and the frame counts -- or None where the clips
    go through the per-clip functions (and for an empty list).  `exps`: stated exponents for ``Engine.clips``; only the one-launch
    route honours them, so where that route is closed (or a clip comes back with ST_WIDE_INPUT) this raises."""
    clips = [torch.as_tensor(c) for c in clips]
    for c in clips:
        if c.dim() != 1:
            raise ValueError(f"every clip must be 1-D audio, got {tuple(c.shape)}")
        stft_frames(int(c.shape[0]))
    if not clips:
        return clips, None
    Ts = [int(c.shape[0]) for c in clips]
    Tmax, Lmax, dev = max(Ts), stft_frames(max(Ts)), clips[0].device
    one_launch = (all(c.is_cuda and c.device == dev for c in clips) and hasattr(model, "engine") and hasattr(model, "forward_float")
                  and not getattr(model, "store_intermediates", False) and _takes(model, inp_bits, inp_exp)
                  and model.engine().clips_ok(Lmax))
    if not one_launch:
        if exps is not None:
            raise NotImplementedError("exps= needs the one-launch clip route: device clips and a model on the fused path")
        return clips, None
    from . import _lib
    eng, n = model.engine(), len(clips)
    audio = torch.nn.utils.rnn.pad_sequence([c.to(torch.float32) for c in clips], batch_first=True)
    samples = torch.tensor(Ts, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        x, lens = stft_mag_clips(audio, samples)
        mask = eng.clips(x, lens, lane=lane, exps=exps)
        st = eng.lane_status(lane, n)[:n * _lib.STATUS_WORDS].cpu().numpy().reshape(n, _lib.STATUS_WORDS)
        bad = int(np.bitwise_or.reduce(st[:, 0] & ~_lib.ST_WIDE_INPUT))
        if bad & _lib.ST_NEGSHIFT:
            raise ValueError("invalid result_exp: a data-dependent shift came out negative (fxparray.py:619-621)")
        if bad & _lib.ST_NEGEXP:
            raise ValueError("a compute_best exponent came out negative")
        L = [stft_frames(T) for T in Ts]
        if exps is not None and (st[:, 0] & _lib.ST_WIDE_INPUT).any():
            raise OverflowError("a clip holds input values beyond 16 bits: only the generic engine serves it, and that engine "
                                "chooses its own exponents")
        for e in np.nonzero(st[:, 0] & _lib.ST_WIDE_INPUT)[0]:
            mask[e, :L[e]] = eng.generic_twin()._forward(x[e, :L[e]].contiguous(), eng.inp_bits, eng.inp_exp, torch.float32, False,
                                                         None, True)[0]
    return clips, (audio, samples, x, mask, L)


def denoise_clips(model, inp_bits: int, inp_exp: int, clips, lane=0, exps=None):
    """``denoise_fused`` for a list of 1-D float audio clips of any lengths >= 512 (below: NotImplementedError, before any
    launch; an empty list gives []).  Returns per clip (cleaned ((len_e - 1) * 128,), cleaned_mag, x, mask), the last three
    (len_e, 257): bit for bit the tuple ``denoise_fused(model, inp_bits, inp_exp, clip[None])`` returns, without the batch axis.

    On a GPU, for a model on the fused path that does not store intermediates and takes (inp_bits, inp_exp) at its encoder, that
    is THREE launches whatever n: the audio is padded once, ``stft_mag_clips`` writes the padded rows and the frame counts,
    ``Engine.clips`` runs on those very tensors, the status words are read once (a clip flagged ST_WIDE_INPUT gets its mask rows
    from the generic engine), ``mask_istft_clips`` follows.  Any other model or device takes ``denoise_fused`` clip by clip.

    One CU walks one clip through the model, tile after tile, so the launch is as long as its longest clip: this is for MANY
    clips.  A single long clip, or a few, belong on ``denoise_fused``, which spreads a sequence over the chip.

    exps: an (n_layers, 5) array of stated exponents (``Engine.calibrate_exps``) for the model launch: every clip then runs at
    them, bit for bit what ``StreamDenoiser(model, 1, exps=exps)`` computes for the same signal however it is pushed.  One-launch
    route only (NotImplementedError otherwise)."""
    clips, front = _clips_front(model, inp_bits, inp_exp, clips, lane, exps)
    if front is None:
        return [tuple(t[0] for t in denoise_fused(model, inp_bits, inp_exp, c[None])) for c in clips]
    audio, samples, x, mask, L = front
    cleaned, cm = mask_istft_clips(audio, samples, mask, cleaned_mag=True)
    return [(cleaned[e, :(L[e] - 1) * HOP], cm[e, :L[e]], x[e, :L[e]], mask[e, :L[e]]) for e in range(len(clips))]


def validate_batch(model, inp_bits: int, inp_exp: int, noisy: torch.Tensor, clean: torch.Tensor, lam: float = 0.001,
                   boundary: str = "float32"):
    """fxprun.py:79-88: (loss, si_snr), one value per sequence: si_snr = si_snr(cleaned, clean) -- the cleaned audio is the
    reference's ``target`` argument -- over the clean audio's length, loss = lam * mean((cleaned_mag - clean_mag)^2) +
    (100 - si_snr), with clean_mag = stft_mag(clean, sub=0).  ``boundary`` as in ``denoise_fused`` (the same numbers either way)."""
    cleaned, cleaned_mag, _, _ = denoise_fused(model, inp_bits, inp_exp, noisy, boundary=boundary)
    clean_mag = stft_mag(clean, sub=0.0)
    score = si_snr(cleaned[..., : clean.shape[-1]], clean.to(torch.float32))
    loss = lam * torch.mean((cleaned_mag - clean_mag) ** 2, dim=(1, 2)) + (100.0 - score)
    return loss, score


def score_fused(noisy: torch.Tensor, clean: torch.Tensor, mask, lam: float = 0.001, mask_exp=None, cleaned: bool = False,
                cleaned_mag: bool = False):
    """fxprun.py:76-88 behind the model in two launches (csrc/audio_score.hpp): ``mask_istft`` of ``noisy`` (B, T) with
    ``mask`` (B, n_seg, 257), scored against ``clean`` (B, T) -> (loss, si_snr, mag_mse), one float32 per sequence, as
    ``validate_batch`` defines them (mag_mse = mean((cleaned_mag - clean_mag)^2)).  With ``cleaned`` / ``cleaned_mag`` the
    planes of ``mask_istft`` follow, bit for bit; without them they are never stored.  An int16 mask with its ``mask_exp``
    takes the int16 entry (the same scores bit for bit as for its to_float()); ``mask=None`` is all zeros.  On a GPU the sums
    are taken in double on the very float32 values the planes would hold; CPU tensors take torch code with
    ``validate_batch``'s arithmetic."""
    noisy = _audio2d(noisy)
    B, T = noisy.shape
    n_seg = stft_frames(T)
    shape = (B, n_seg, NFFT // 2 + 1)
    if clean.dim() != 2 or tuple(clean.shape) != (B, T) or clean.device != noisy.device:
        raise ValueError(f"clean must be {(B, T)} on {noisy.device}, got {tuple(clean.shape)} on {clean.device}")
    clean = clean.to(torch.float32).contiguous()
    i16 = mask is not None and mask.dtype == torch.int16
    if i16:
        if mask_exp is None:
            raise ValueError("an int16 mask needs its mask_exp")
        _int16_range(16, mask_exp, "score_fused")
    elif mask_exp is not None:
        raise ValueError("mask_exp goes with an int16 mask")
    if mask is not None:
        if tuple(mask.shape) != shape or mask.device != noisy.device:
            raise ValueError(f"mask must be {shape} on {noisy.device}, got {tuple(mask.shape)} on {mask.device}")
        mask = mask.contiguous() if i16 else mask.to(torch.float32).contiguous()
    if not noisy.is_cuda:
        if i16:
            mask = torch.ldexp(mask.to(torch.float32), torch.tensor(-int(mask_exp)))
        out, cm = mask_istft(noisy, mask, cleaned_mag=True)
        score = si_snr(out[..., :T], clean)
        mse = torch.mean((cm - stft_mag(clean, sub=0.0)) ** 2, dim=(1, 2))
        loss = lam * mse + (100.0 - score)
    else:
        from . import _lib
        dev = noisy.device
        out = torch.empty(B, (n_seg - 1) * HOP, dtype=torch.float32, device=dev) if cleaned else None
        cm = torch.empty(shape, dtype=torch.float32, device=dev) if cleaned_mag else None
        scores = torch.empty(3, B, dtype=torch.float32, device=dev)
        ws_bytes = _lib.lib.s5fxp_score_workspace_bytes(B, T)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None
        entry, m = ("s5fxp_mask_istft_score_i16", (ptr(mask), int(mask_exp))) if i16 else ("s5fxp_mask_istft_score", (ptr(mask),))
        with torch.cuda.device(dev):
            _lib.check(getattr(_lib.lib, entry)(noisy.data_ptr(), clean.data_ptr(), *m, B, T, float(lam), ptr(out), ptr(cm),
                                                ws.data_ptr(), ws_bytes, scores[1].data_ptr(), scores[2].data_ptr(),
                                                scores[0].data_ptr(), torch.cuda.current_stream().cuda_stream), entry)
        loss, score, mse = scores[0], scores[1], scores[2]
    return (loss, score, mse) + ((out,) if cleaned else ()) + ((cm,) if cleaned_mag else ())


def validate_fused(model, inp_bits: int, inp_exp: int, noisy: torch.Tensor, clean: torch.Tensor, lam: float = 0.001,
                   boundary: str = "float32", exps=None):
    """``validate_batch`` as stft_mag -> model -> score_fused: (loss, si_snr), one value per sequence, without the cleaned audio
    or a magnitude plane ever being stored -- on a GPU three launches plus the forward.  The model's route is chosen as in
    ``denoise_fused``, ``boundary`` and ``exps`` included; the numbers are ``validate_batch``'s up to the rounding of its
    float32 sums.  With ``exps`` they are ``validate_clips(..., exps=)``'s on the same clips: the masks are bit-equal."""
    from .fxparray import RoundingMode, fxp_from_fp

    if boundary not in ("float32", "int16"):
        raise ValueError(f'boundary must be "float32" or "int16", got {boundary!r}')
    if boundary == "int16":
        if getattr(model, "store_intermediates", False):
            raise ValueError("a model that stores intermediates runs op by op on FxpArrays: use the float32 boundary")
        xi = stft_mag_i16(noisy, inp_bits, inp_exp)
        mask = model.forward_int16(xi, inp_bits, inp_exp) if exps is None else _forward_at(model, xi, inp_bits, inp_exp, exps)
        out_exp = model.out_exp if hasattr(model, "out_exp") else model.engine().out_exp
        return score_fused(noisy, clean, mask, lam, mask_exp=out_exp)[:2]
    x = stft_mag(noisy)
    if exps is not None:
        mask = _forward_at(model, x, inp_bits, inp_exp, exps)
    elif hasattr(model, "forward_float") and not getattr(model, "store_intermediates", False) and _takes(model, inp_bits, inp_exp):
        mask = model.forward_float(x)
    else:
        fx = fxp_from_fp(x, bits=inp_bits, exp=inp_exp, signed=True, round_mode=RoundingMode.FLOOR)
        mask = model(fx).to_float()
    return score_fused(noisy, clean, mask, lam)[:2]


def denoise_float(float_engine, noisy: torch.Tensor, fq=None):
    """``denoise_fused`` with the FLOAT model (``floatmodel.FloatEngine``) in the middle: stft_mag -> FloatEngine.forward ->
    mask_istft -> (cleaned audio, cleaned magnitude, x, mask).  What the fixed-point loop approximates, on the same clips.
    ``fq`` (``floatmodel.fq_spec``) goes to the model's forward: the float loop with chosen tensors fake-quantised."""
    x = stft_mag(noisy)
    mask = float_engine.forward(x, fq=fq)
    cleaned, cleaned_mag = mask_istft(noisy, mask, cleaned_mag=True)
    return cleaned, cleaned_mag, x, mask


def validate_float(float_engine, noisy: torch.Tensor, clean: torch.Tensor, lam: float = 0.001, fq=None):
    """``validate_fused`` with the FLOAT model: stft_mag -> FloatEngine.forward -> score_fused -> (loss, si_snr), one value per
    sequence.  The difference to ``validate_fused`` on the same clips is the cost of quantisation in dB; the difference
    between a call with ``fq`` (``floatmodel.fq_spec``) and one without is the SI-SNR cost of those quantisers alone."""
    return score_fused(noisy, clean, float_engine.forward(stft_mag(noisy), fq=fq), lam)[:2]


def score_clips(noisy: torch.Tensor, clean: torch.Tensor, samples: torch.Tensor, mask, lam: float = 0.001, cleaned: bool = False,
                cleaned_mag: bool = False, out=None):
    """``score_fused`` for n clips of different lengths in TWO launches whatever n (csrc/audio_score.hpp:
    k_mask_istft_score_clips, k_score_finalize_clips): noisy and clean (n, Tmax) float32, padded; samples (n,) int32 on their
    device; mask (n, Lmax, 257) float32 or None (zeros), the layouts of ``mask_istft_clips`` -> (loss, si_snr, mag_mse), each
    (n,) float32.  Clip e is scored over its own T_e samples and len_e frames -- padding enters neither N, the means nor the MSE
    denominator -- and gets bit for bit ``score_fused(noisy[e:e+1, :T_e], clean[e:e+1, :T_e], mask[e:e+1, :len_e])``.  With
    ``cleaned`` / ``cleaned_mag`` the planes of ``mask_istft_clips`` follow, bit for bit, nothing written behind a clip's end
    (``out``: the plane tensors to write into, in the order returned); without them they are never stored.  A clip below 512
    samples has no frames: its three scores are NaN and nothing else of it is written."""
    noisy, samples, n, Tmax, Lmax = _clips_args(noisy, samples)
    dev, shape = noisy.device, (n, Lmax, NFFT // 2 + 1)
    if clean.dim() != 2 or tuple(clean.shape) != (n, Tmax) or clean.device != dev:
        raise ValueError(f"clean must be {(n, Tmax)} on {dev}, got {tuple(clean.shape)} on {clean.device}")
    clean = clean.to(torch.float32).contiguous()
    if mask is not None:
        if tuple(mask.shape) != shape or mask.device != dev:
            raise ValueError(f"mask must be {shape} on {dev}, got {tuple(mask.shape)} on {mask.device}")
        mask = mask.to(torch.float32).contiguous()
    planes = _clips_out(out, ([((n, (Lmax - 1) * HOP), torch.float32, dev)] if cleaned else [])
                        + ([(shape, torch.float32, dev)] if cleaned_mag else []), "score_clips")
    o, cm = planes[0] if cleaned else None, planes[-1] if cleaned_mag else None
    scores = torch.empty(3, n, dtype=torch.float32, device=dev)
    if not noisy.is_cuda:
        T, L = _clip_lengths(samples, Tmax)
        for e in range(n):
            if not L[e]:
                scores[:, e] = float("nan")
                continue
            r = score_fused(noisy[e:e + 1, :T[e]], clean[e:e + 1, :T[e]], mask[e:e + 1, :L[e]] if mask is not None else None, lam,
                            cleaned=cleaned, cleaned_mag=cleaned_mag)
            scores[0, e], scores[1, e], scores[2, e] = r[0][0], r[1][0], r[2][0]
            if cleaned:
                o[e, :(L[e] - 1) * HOP] = r[3][0]
            if cleaned_mag:
                cm[e, :L[e]] = r[-1][0]
        return (scores[0], scores[1], scores[2]) + tuple(planes)
    from . import _lib
    ws_bytes = _lib.lib.s5fxp_score_clips_workspace_bytes(n, Tmax)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.s5fxp_mask_istft_score_clips(noisy.data_ptr(), clean.data_ptr(), ptr(mask), n, Tmax, samples.data_ptr(),
                                                         float(lam), ptr(o), ptr(cm), ws.data_ptr(), ws_bytes, scores[1].data_ptr(),
                                                         scores[2].data_ptr(), scores[0].data_ptr(),
                                                         torch.cuda.current_stream().cuda_stream), "s5fxp_mask_istft_score_clips")
    return (scores[0], scores[1], scores[2]) + tuple(planes)


def validate_clips(model, inp_bits: int, inp_exp: int, noisy_clips, clean_clips, lam: float = 0.001, lane=0, exps=None):
    """``validate_fused`` for lists of 1-D float audio clips of any lengths >= 512 (below: NotImplementedError, before any
    launch): clean_clips[e] has noisy_clips[e]'s length (otherwise, or for lists of different counts, ValueError).  Returns
    (loss, si_snr), (n,) float32 each (two empty tensors for empty lists): per clip bit for bit
    ``validate_fused(model, inp_bits, inp_exp, noisy[None], clean[None], lam)`` on the float32 boundary.

    Under ``denoise_clips``' conditions for its one-launch route, with the clean clips on the noisy clips' device, that is FOUR
    launches whatever n: ``stft_mag_clips`` -> ``Engine.clips`` -> the scored inverse -> its finalize (``score_clips``); the
    status words are read once, before the scored inverse (a clip flagged ST_WIDE_INPUT gets its mask rows from the generic
    engine).  Any other model or device takes ``validate_fused`` clip by clip.

    One CU walks one clip through the model, tile after tile, so the launch is as long as its longest clip: this is for MANY
    clips.  A single long clip, or a few, belong on ``validate_fused``, which spreads a sequence over the chip.

    exps: stated exponents for the model launch, as ``denoise_clips`` takes them (one-launch route only)."""
    noisy_clips, clean_clips = list(noisy_clips), [torch.as_tensor(c) for c in clean_clips]
    if len(noisy_clips) != len(clean_clips):
        raise ValueError(f"{len(noisy_clips)} noisy clips but {len(clean_clips)} clean ones")
    for e, (c, r) in enumerate(zip(noisy_clips, clean_clips)):
        if tuple(r.shape) != tuple(torch.as_tensor(c).shape):
            raise ValueError(f"clean clip {e} must be {tuple(torch.as_tensor(c).shape)}, got {tuple(r.shape)}")
    same_device = all(r.device == torch.as_tensor(c).device for c, r in zip(noisy_clips, clean_clips))
    # clean clips elsewhere: no model qualifies for the one-launch route
    noisy_clips, front = _clips_front(model if same_device else None, inp_bits, inp_exp, noisy_clips, lane, exps)
    if not noisy_clips:
        return torch.empty(0, dtype=torch.float32), torch.empty(0, dtype=torch.float32)
    if front is None:
        r = [validate_fused(model, inp_bits, inp_exp, c[None], k[None], lam) for c, k in zip(noisy_clips, clean_clips)]
        return torch.cat([t[0] for t in r]), torch.cat([t[1] for t in r])
    audio, samples, _, mask, _ = front
    clean = torch.nn.utils.rnn.pad_sequence([c.to(torch.float32) for c in clean_clips], batch_first=True)
    return score_clips(audio, clean, samples, mask, lam)[:2]


def _float_clips_front(float_engine, clips, one_launch: bool = True, fq=None):
    """``_clips_front`` with the FLOAT model in the middle: the same checks of the clip list, and where every clip lies on the
    engine's device the padding, ``stft_mag_clips`` and ``FloatEngine.forward_clips_device`` on those very tensors.  Returns
    (clips, front), front = (audio, samples, x, mask, L) or None for the per-clip route (and for an empty list)."""
    clips = [torch.as_tensor(c) for c in clips]
    for c in clips:
        if c.dim() != 1:
            raise ValueError(f"every clip must be 1-D audio, got {tuple(c.shape)}")
        stft_frames(int(c.shape[0]))
    if not clips or not one_launch or not float_engine.on_device or not all(c.is_cuda and c.device == float_engine.device for c in clips):
        return clips, None
    Ts = [int(c.shape[0]) for c in clips]
    audio = torch.nn.utils.rnn.pad_sequence([c.to(torch.float32) for c in clips], batch_first=True)
    samples = torch.tensor(Ts, dtype=torch.int32, device=audio.device)
    with torch.cuda.device(audio.device):
        x, lens = stft_mag_clips(audio, samples)
        mask = float_engine.forward_clips_device(x, lens, fq=fq)
    return clips, (audio, samples, x, mask, [stft_frames(T) for T in Ts])


def denoise_float_clips(float_engine, clips, fq=None):
    """``denoise_float`` for a list of 1-D float audio clips of any lengths >= 512 (below: NotImplementedError, before any
    launch; an empty list gives []).  Returns what ``denoise_clips`` returns, per clip (cleaned ((len_e - 1) * 128,),
    cleaned_mag, x, mask): bit for bit the tuple ``denoise_float(float_engine, clip[None])`` returns, without the batch axis.
    With the engine and every clip on one GPU that is ``stft_mag_clips`` -> ``FloatEngine.forward_clips_device`` ->
    ``mask_istft_clips``, whatever n; otherwise ``denoise_float`` clip by clip.  ``fq`` as in ``denoise_float``."""
    clips, front = _float_clips_front(float_engine, clips, fq=fq)
    if front is None:
        return [tuple(t[0] for t in denoise_float(float_engine, c[None], fq=fq)) for c in clips]
    audio, samples, x, mask, L = front
    cleaned, cm = mask_istft_clips(audio, samples, mask, cleaned_mag=True)
    return [(cleaned[e, :(L[e] - 1) * HOP], cm[e, :L[e]], x[e, :L[e]], mask[e, :L[e]]) for e in range(len(clips))]


def validate_float_clips(float_engine, noisy_clips, clean_clips, lam: float = 0.001, fq=None):
    """``validate_float`` for lists of 1-D float audio clips, with ``validate_clips``' checks of the two lists -> (loss, si_snr),
    (n,) float32 each (two empty tensors for empty lists): per clip bit for bit
    ``validate_float(float_engine, noisy[None], clean[None], lam)``.  With the engine and all clips on one GPU that is
    ``stft_mag_clips`` -> ``FloatEngine.forward_clips_device`` -> ``score_clips``; otherwise ``validate_float`` clip by clip.
    The difference to ``validate_clips`` on the same clips is the cost of quantisation in dB.  ``fq`` as in ``validate_float``."""
    noisy_clips, clean_clips = list(noisy_clips), [torch.as_tensor(c) for c in clean_clips]
    if len(noisy_clips) != len(clean_clips):
        raise ValueError(f"{len(noisy_clips)} noisy clips but {len(clean_clips)} clean ones")
    for e, (c, r) in enumerate(zip(noisy_clips, clean_clips)):
        if tuple(r.shape) != tuple(torch.as_tensor(c).shape):
            raise ValueError(f"clean clip {e} must be {tuple(torch.as_tensor(c).shape)}, got {tuple(r.shape)}")
    same_device = all(r.device == torch.as_tensor(c).device for c, r in zip(noisy_clips, clean_clips))
    noisy_clips, front = _float_clips_front(float_engine, noisy_clips, one_launch=same_device, fq=fq)
    if not noisy_clips:
        return torch.empty(0, dtype=torch.float32), torch.empty(0, dtype=torch.float32)
    if front is None:
        r = [validate_float(float_engine, c[None], k[None], lam, fq=fq) for c, k in zip(noisy_clips, clean_clips)]
        return torch.cat([t[0] for t in r]), torch.cat([t[1] for t in r])
    audio, samples, _, mask, _ = front
    clean = torch.nn.utils.rnn.pad_sequence([c.to(torch.float32) for c in clean_clips], batch_first=True)
    return score_clips(audio, clean, samples, mask, lam)[:2]


# ---------------------------------------------------------------------------------------------------------------------
# The loop for a live signal: csrc/audio_stream.hpp (s5fxp_stream_stft / s5fxp_stream_mask_istft) either side of
# SessionPool.push.
# ---------------------------------------------------------------------------------------------------------------------
STREAM_MAX_HOPS = 32


def stream_frames(hops_before: int, c: int) -> int:
    """Frames a push of c hops completes after hops_before hops: frame k covers audio hops k-2 .. k+1."""
    return c - (1 if hops_before == 0 else 0)


def stream_out_hops(hops_before: int, c: int, final: bool = False) -> int:
    """Output hops of that push: hop o needs frames o-1 .. o+2, the last hop of a stream (``final``) has only three."""
    return min(c, max(0, hops_before + c - 3)) + (1 if final else 0)


class StreamDenoiser:
    """``denoise_fused`` for ``sessions`` live signals in lock step: whole hops of 128 samples in, cleaned audio out, three
    hops (24 ms at 16 kHz) behind the input.  A caller zero-fills its last hop.

        d = StreamDenoiser(model, sessions)
        for hops in source:                 # (sessions, c * 128) float32, c = 1 .. 32
            sink(d.push(hops))              # (sessions, O * 128); O = 0 while the first three hops arrive
        sink(d.finish())                    # the last 3 * 128 samples; reset() before the next signal

    With h hops received, a push of c completes frames h-1 .. h+c-2 of the batch framing and yields output hops
    max(0, h-3) .. h+c-4; ``finish`` pushes scipy's two trailing hops of zeros.  On a GPU a push is three launches: the x rows
    and the audio of all pushes, concatenated, are bit for bit ``stft_mag`` / ``mask_istft`` of the whole signal with the
    concatenated masks, and the masks are what a fresh ``SessionPool`` returns for the same rows in the same chunks.  They
    are NOT the masks of one forward over the whole clip: every chunk is its own compute_best batch and chooses its own
    exponents, so low bits differ (as for ``s5fxp_forward_opts.state_in``).

    CPU tensors, and models without an engine (anything with a stateless ``forward_float``), take torch ops with the same
    bookkeeping.  What ``push`` returns is valid until the next push of the same shape.

    exps: an (n_layers, 5) array of stated exponents (``Engine.calibrate_exps``) for the pool (``SessionPool(exps=)``): no chunk
    chooses exponents, so the audio is the same however the hops are grouped, and bit for bit that of
    ``denoise_clips(..., [signal], exps=exps)``.  Needs a model with an engine (NotImplementedError otherwise)."""

    latency_hops = 3

    def __init__(self, model, sessions: int, sub: float = STFT_MAG_MEAN, exps=None):
        if sessions < 1:
            raise ValueError("sessions must be >= 1")
        if exps is not None and not hasattr(model, "engine"):
            raise NotImplementedError("exps= needs a model with an engine")
        self.exps = exps
        self.model, self.sessions, self.sub = model, int(sessions), float(sub)
        self.hops = 0
        self._done = False
        self._pool = None     # the model's SessionPool (kernel route)
        self._state = None    # kernel route: (S, state floats); torch route: (audio history, segment carry)
        self._buf = {}

    # -- bookkeeping ----------------------------------------------------------------------------
    def reset(self) -> None:
        """All sessions start a new signal."""
        self.hops, self._done = 0, False
        if self._pool is not None:
            self._pool.reset()
        if torch.is_tensor(self._state):
            self._state.zero_()
        else:
            self._state = None

    def _kernels(self, dev: torch.device) -> bool:
        return dev.type == "cuda" and hasattr(self.model, "engine")

    def push(self, hops: torch.Tensor, check: bool = True, details: bool = False):
        """hops: (sessions, c * 128) float32, c = 1 .. 32.  Returns the cleaned audio (sessions, O * 128); with ``details``
        (cleaned, x, mask, cleaned_mag), the last three (sessions, F, 257).  ``check`` is SessionPool.push's."""
        if hops.dim() != 2 or hops.shape[0] != self.sessions or hops.shape[1] % HOP or hops.dtype != torch.float32:
            raise ValueError(f"hops must be ({self.sessions}, c * {HOP}) float32, got {tuple(hops.shape)} {hops.dtype}")
        c = hops.shape[1] // HOP
        if not 1 <= c <= STREAM_MAX_HOPS:
            raise ValueError(f"a push takes 1 .. {STREAM_MAX_HOPS} hops, got {c}")
        return self._push(hops.contiguous(), c, hops.device, False, check, details)

    def finish(self, check: bool = True, details: bool = False, device=None):
        """The end of the signal: scipy's trailing boundary, two hops of zeros.  Returns the last 3 * 128 samples per session
        (and with ``details`` the last two frames' rows) and leaves the object needing a ``reset()``."""
        if self.hops < 4:
            raise NotImplementedError(f"stft needs at least {NFFT} samples, got {self.hops * HOP}")
        if device is None:
            device = self._state.device if torch.is_tensor(self._state) else self._state[0].device
        return self._push(None, 2, torch.device(device), True, check, details)

    def _push(self, hops, c, dev, final, check, details):
        if self._done:
            raise RuntimeError("the signal has ended: reset() first")
        h, S = self.hops, self.sessions
        F, n_out = stream_frames(h, c), stream_out_hops(h, c, final)
        run = self._push_kernels if self._kernels(dev) else self._push_torch
        res = run(hops, c, dev, final, check, details, h, S, F, n_out)
        self.hops += c
        self._done = final
        return res

    # -- HIP kernels + SessionPool ----------------------------------------------------------------
    def _buffers(self, dev, F, n_out, details):
        key = (F, n_out)
        b = self._buf.get(key)
        if b is None:
            b = self._buf[key] = [torch.empty(self.sessions, F, NFFT // 2 + 1, dtype=torch.float32, device=dev),
                                  torch.empty(self.sessions, n_out * HOP, dtype=torch.float32, device=dev), None]
        if details and b[2] is None:
            b[2] = torch.empty(self.sessions, F, NFFT // 2 + 1, dtype=torch.float32, device=dev)
        return b

    def _push_kernels(self, hops, c, dev, final, check, details, h, S, F, n_out):
        from . import _lib
        if self._pool is None:
            self._pool = self.model.engine().pool(S, exps=self.exps)
        if self._state is None:
            self._state = torch.zeros(S, _lib.lib.s5fxp_stream_audio_state_bytes() // 4, dtype=torch.float32, device=dev)
        x, out, cm = self._buffers(dev, F, n_out, details)
        ptr = lambda t, n: t.data_ptr() if t is not None and n else None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib.s5fxp_stream_stft(ptr(hops, 1), S, c, h, self.sub, self._state.data_ptr(), ptr(x, F), stream),
                       "s5fxp_stream_stft")
            mask = self._pool.push(x, check=check) if F else x
            _lib.check(_lib.lib.s5fxp_stream_mask_istft(ptr(mask, F), S, c, h, int(final), self._state.data_ptr(),
                                                        ptr(out, n_out), ptr(cm, F) if details else None, stream),
                       "s5fxp_stream_mask_istft")
        return (out, x, mask, cm) if details else out

    # -- torch ops --------------------------------------------------------------------------------
    def _mask(self, x, check):
        if hasattr(self.model, "engine"):
            if self._pool is None:
                self._pool = self.model.engine().pool(self.sessions, exps=self.exps)
            return self._pool.push(x.to(self._pool.engine.device), check=check).to(x.device)
        return self.model.forward_float(x)

    def _push_torch(self, hops, c, dev, final, check, details, h, S, F, n_out):
        if self._state is None:
            self._state = (torch.zeros(S, 3 * HOP, device=dev), torch.zeros(S, 3, NFFT, device=dev))
        hist, carry = self._state
        if hops is None:
            hops = torch.zeros(S, c * HOP, device=dev)
        window = torch.cat([hist, hops], dim=1)
        fr = window.unfold(-1, NFFT, HOP)[:, c - F:]           # frames h-1 .. h+c-2 without frame -1
        if F:
            z = torch.fft.rfft(fr, n=NFFT, dim=-1) / NFFT
            x = (z.abs() - self.sub).contiguous()
            mask = self._mask(x, check)
            f = 1.0 + mask
            seg, cm = torch.fft.irfft(z * f, n=NFFT, dim=-1) * NFFT, z.abs() * f
        else:  # the first hop of a signal completes no frame
            x = mask = cm = torch.zeros(S, 0, NFFT // 2 + 1, device=dev)
            seg = torch.zeros(S, 0, NFFT, device=dev)
        # the segment list of the push: carried, (frame -1,) new, (the frame beyond the end); row r sums entries r .. r+3
        zero = torch.zeros(S, 1, NFFT, device=dev)
        v = torch.cat([carry] + [zero] * (c - F) + [seg] + [zero] * int(final), dim=1)
        rows = c + int(final)
        acc = torch.zeros(S, rows, HOP, device=dev)
        for q in range(4):
            acc = acc + v[:, q:q + rows, HOP * (3 - q):HOP * (4 - q)]
        cover = torch.full((rows,), 4.0, device=dev)
        if 0 <= 3 - h < rows:
            cover[3 - h] = 3.0          # output hop 0: frame -1 does not exist
        if final:
            cover[-1] = 3.0
        out = (acc / cover[None, :, None])[:, rows - n_out:].reshape(S, n_out * HOP)
        self._state = (window[:, -3 * HOP:].contiguous(), v[:, c:c + 3].contiguous())
        return (out, x, mask, cm) if details else out


class SessionDenoiser:
    """``StreamDenoiser`` for ``slots`` live signals that start, stop and idle on their own: one ``push`` serves any subset
    of the slots, each with its own hop count and phase, and sessions that end join the same call.

        d = SessionDenoiser(model, slots)
        out, n_out = d.push([0, 3], hops, counts=[1, 4], finish=[2])   # slots 0 and 3 push samples, slot 2 ends, 1 idles
        d.start([2])                                                   # slot 2 begins its next signal

    On a GPU a push is three launches whatever the mix (``s5fxp_stream_stft_ragged``, ``s5fxp_model_step_ragged_f32``,
    ``s5fxp_stream_mask_istft_ragged``) and one small host-to-device copy of the descriptors all three read.  Every session
    computes, bit for bit, what a ``StreamDenoiser(model, 1)`` fed the same chunks computes.  Results are padded: entry e of a
    push is ``ids[e]``, then the sessions of ``finish`` in order; its ``n_out[e]`` output hops and ``frames[e]`` rows sit at the
    front of row e, and what lies behind them is unspecified.  What ``push`` returns is valid until the next push of the same
    shape.  CPU tensors and models without an engine run one ``StreamDenoiser(model, 1)`` per slot.

    exps: stated exponents for the pool, as ``StreamDenoiser`` takes them: every session's audio is then independent of how its
    hops are grouped and of what shares its pushes."""

    latency_hops = 3

    def __init__(self, model, slots: int, sub: float = STFT_MAG_MEAN, exps=None):
        if slots < 1:
            raise ValueError("slots must be >= 1")
        if exps is not None and not hasattr(model, "engine"):
            raise NotImplementedError("exps= needs a model with an engine")
        self.exps = exps
        self.model, self.slots, self.sub = model, int(slots), float(sub)
        self.hops = np.zeros(self.slots, dtype=np.int64)   # hops received per slot
        self._done = np.zeros(self.slots, dtype=bool)
        self._fresh = np.ones(self.slots, dtype=bool)      # the slot's next push starts a signal
        self._pool = None       # the model's SessionPool (kernel route)
        self._state = None      # kernel route: (slots, state floats)
        self._each = None       # torch route: one StreamDenoiser(model, 1) per slot
        self._dev = None
        self._buf = {}

    def _ids(self, ids, what):
        ids = np.asarray(ids if isinstance(ids, np.ndarray) else list(ids), dtype=np.int64).reshape(-1)
        if len(ids):
            seen = np.zeros(self.slots, dtype=bool)
            if ids.min() < 0 or ids.max() >= self.slots:
                raise ValueError(f"{what} must be slots 0 .. {self.slots - 1}, got {ids.tolist()}")
            seen[ids] = True
            if int(seen.sum()) != len(ids):
                raise ValueError(f"{what} name a slot twice: {ids.tolist()}")
        return ids

    def start(self, ids) -> None:
        """The slots in `ids` begin a new signal: their next push carries FRESH, so nothing is cleared on the device."""
        ids = self._ids(ids, "ids")
        self.hops[ids], self._done[ids], self._fresh[ids] = 0, False, True
        if self._each is not None:
            for i in ids:
                self._each[i].reset()

    def finish(self, ids, check: bool = True, details: bool = False):
        """The end of the signals in `ids`: ``push`` with only ``finish``."""
        return self.push((), None, finish=ids, check=check, details=details)

    def push(self, ids, hops, counts=None, finish=(), check: bool = True, details: bool = False):
        """ids: the slots that push samples; hops: (len(ids), cmax * 128) float32, cmax = 1 .. 32 (None when only sessions
        finish); counts: hops of each entry, 1 .. cmax (default cmax for all), an entry's samples at the front of its row.
        Sessions in `finish` end in the same call: two hops of zeros with ``final``.  Returns (cleaned audio (n, (cmax' + 1) *
        128), n_out), cmax' = max(cmax, 2 if any session finishes), n_out[e] the output hops of entry e; with ``details``
        (cleaned, n_out, x, mask, cleaned_mag, frames), the three tensors (n, cmax', 257).  ``check`` is SessionPool.push's.
        When sessions finish in a push whose rows are one hop wide, the samples are first copied into rows two hops wide.

        RuntimeError for a slot whose signal has ended (``start`` it first), NotImplementedError for a signal that ends below
        four hops (512 samples), ValueError for shapes, counts and slots named twice."""
        ids = self._ids(ids, "ids")
        fin = self._ids(finish, "finish") if len(finish) else ids[:0]
        entries = self._ids(np.concatenate([ids, fin]), "ids and finish together") if len(fin) else ids
        n = len(entries)
        if n < 1:
            raise ValueError("a push names at least one slot")
        if len(ids):
            if hops is None or hops.dim() != 2 or hops.shape[0] != len(ids) or hops.shape[1] % HOP or hops.dtype != torch.float32:
                raise ValueError(f"hops must be ({len(ids)}, cmax * {HOP}) float32")
            cmax = hops.shape[1] // HOP
            if not 1 <= cmax <= STREAM_MAX_HOPS:
                raise ValueError(f"a push takes 1 .. {STREAM_MAX_HOPS} hops, got {cmax}")
            self._dev = hops.device
        else:
            cmax = 0
            if self._dev is None:
                raise RuntimeError("no signal has been pushed yet")
        c = np.full(n, 2, dtype=np.int64)      # a finishing entry is two hops of zeros
        if counts is None:
            c[:len(ids)] = cmax
        else:
            counts = np.asarray(counts, dtype=np.int64).reshape(-1)
            if len(counts) != len(ids) or (len(ids) and (counts.min() < 1 or counts.max() > cmax)):
                raise ValueError(f"counts must be {len(ids)} hop counts 1 .. {cmax}, got {counts.tolist()}")
            c[:len(ids)] = counts
        if self._done[entries].any():
            raise RuntimeError(f"the signal of slots {entries[self._done[entries]].tolist()} has ended: start() them first")
        h = self.hops[entries]
        if len(fin) and h[len(ids):].min() < 4:
            raise NotImplementedError(f"stft needs at least {NFFT} samples: slots {fin[self.hops[fin] < 4].tolist()} have received "
                                      f"fewer than four hops")
        final = np.arange(n) >= len(ids)
        frames = c - (h == 0)
        n_out = np.minimum(c, np.maximum(0, h + c - 3)) + final
        cw = max(cmax, 2 if len(fin) else 0)
        dev = self._dev
        run = self._push_kernels if dev.type == "cuda" and hasattr(self.model, "engine") else self._push_each
        res = run(entries, len(ids), hops, cmax, cw, c, h, final, frames, n_out, dev, check, details)
        self.hops[entries] += c
        self._fresh[entries] = False
        self._done[fin] = True
        return (res[0], n_out) + ((res[1], res[2], res[3], frames) if details else ())

    # -- HIP kernels + SessionPool.push_ragged ------------------------------------------------------
    def _push_kernels(self, entries, n_push, hops, cmax, cw, c, h, final, frames, n_out, dev, check, details):
        from . import _lib
        n, nb = len(entries), NFFT // 2 + 1
        if self._pool is None:
            self._pool = self.model.engine().pool(self.slots, exps=self.exps)
        if self._state is None:
            self._state = torch.zeros(self.slots, _lib.lib.s5fxp_stream_audio_state_bytes() // 4, dtype=torch.float32, device=dev)
        b = self._buf.get((n, cw))
        if b is None:
            b = self._buf[(n, cw)] = [torch.empty(n, cw, nb, dtype=torch.float32, device=dev),
                                      torch.empty(n, (cw + 1) * HOP, dtype=torch.float32, device=dev), None, None]
        if details and b[2] is None:
            b[2] = torch.empty(n, cw, nb, dtype=torch.float32, device=dev)
        x, out, cm = b[0], b[1], b[2] if details else None
        audio = hops.contiguous() if n_push else None
        if n_push and cmax != cw:   # sessions finish beside one-hop rows: the launch's rows are two hops wide
            if b[3] is None:
                b[3] = torch.zeros(n, cw * HOP, dtype=torch.float32, device=dev)
            b[3][:n_push, :cmax * HOP] = audio
            audio = b[3]
        fresh = self._fresh[entries]
        flags = (fresh * _lib.PUSH_FRESH + final * (_lib.PUSH_ZEROS | _lib.PUSH_FINAL)).astype(np.int32)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            desc = self._pool.stage_desc(entries, frames, flags, hops=c, h4=np.minimum(h, 4), Lmax=cw, cmax=cw)
            _lib.check(_lib.lib.s5fxp_stream_stft_ragged(audio.data_ptr() if audio is not None else None, n, cw, desc.data_ptr(),
                                                         self.sub, self._state.data_ptr(), self.slots, x.data_ptr(), stream),
                       "s5fxp_stream_stft_ragged")
            mask = self._pool.push_ragged(entries, x, frames, fresh=entries[fresh] if fresh.any() else (), check=check, desc=desc)
            _lib.check(_lib.lib.s5fxp_stream_mask_istft_ragged(mask.data_ptr(), n, cw, desc.data_ptr(), self._state.data_ptr(),
                                                               self.slots, out.data_ptr(), cm.data_ptr() if details else None,
                                                               stream), "s5fxp_stream_mask_istft_ragged")
        return out, x, mask, cm

    # -- one StreamDenoiser per slot (CPU tensors, models without an engine) -------------------------
    def _push_each(self, entries, n_push, hops, cmax, cw, c, h, final, frames, n_out, dev, check, details):
        n, nb = len(entries), NFFT // 2 + 1
        if self._each is None:
            self._each = [StreamDenoiser(self.model, 1, self.sub, exps=self.exps) for _ in range(self.slots)]
        out = torch.zeros(n, (cw + 1) * HOP, dtype=torch.float32, device=dev)
        x, mask, cm = (torch.zeros(n, cw, nb, dtype=torch.float32, device=dev) for _ in range(3))
        for e, slot in enumerate(entries):
            d = self._each[slot]
            if final[e]:
                r = d.finish(check=check, details=True, device=dev)
            else:
                r = d.push(hops[e:e + 1, :int(c[e]) * HOP].contiguous(), check=check, details=True)
            out[e, :int(n_out[e]) * HOP] = r[0][0]
            for dst, src in zip((x, mask, cm), r[1:]):
                dst[e, :int(frames[e])] = src[0]
        return out, x, mask, cm
