"""The streaming denoising loop: csrc/audio_stream.hpp (s5fxp_stream_stft, s5fxp_stream_mask_istft) and audio.StreamDenoiser.

Contract (include/s5fxp.h): with h hops of 128 samples received, a push of c hops completes F = c - (h == 0) frames (frames
h-1 .. h+c-2 of the batch framing) and yields O = min(c, max(0, h+c-3)) + final output hops; a stream of m hops ends with two
hops of zeros and `final`.  Streamed this way x, cleaned_mag and the audio are BIT FOR BIT what the batch kernels give for the
whole signal and the concatenated masks (torch.equal below), and the masks are a fresh SessionPool's for the same rows in the
same chunks.

The restatement (ref_stft / ref_istft) and the tolerances of the CPU route are those of tests/test_audio_kernels.py."""
import ctypes as C

import numpy as np
import pytest

import test_audio_kernels as AK
from test_audio_kernels import ATOL_AUDIO, ATOL_SPEC, ref_istft, ref_stft

HOP = 128


def F_of(h, c):
    return c - (1 if h == 0 else 0)


def O_of(h, c, final):
    return min(c, max(0, h + c - 3)) + (1 if final else 0)


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("s5fxp_stream_audio_state_bytes", "s5fxp_stream_frames", "s5fxp_stream_out_hops", "s5fxp_stream_stft",
               "s5fxp_stream_mask_istft")


def test_symbols_and_version():
    from sparsernns_amd import _lib
    assert _lib.lib.s5fxp_version() >= 108
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)


def test_counts_and_state_size():
    from sparsernns_amd import _lib, audio
    L = _lib.lib
    for h in range(7):
        for c in (1, 2, 3, 4, 32):
            assert L.s5fxp_stream_frames(h, c) == F_of(h, c) == audio.stream_frames(h, c)
            for final in (0, 1):
                assert L.s5fxp_stream_out_hops(h, c, final) == O_of(h, c, final) == audio.stream_out_hops(h, c, bool(final))
    for h, c in ((0, 0), (5, 0), (0, 33), (5, 33), (-1, 1), (-1, 4)):
        assert L.s5fxp_stream_frames(h, c) == -1
        assert L.s5fxp_stream_out_hops(h, c, 0) == -1 and L.s5fxp_stream_out_hops(h, c, 1) == -1
    n = L.s5fxp_stream_audio_state_bytes()
    assert n > 0 and n % 16 == 0


def test_argument_validation_before_any_device_access():
    """The codes come back for pointers that are not device memory at all: nothing was launched or dereferenced."""
    from sparsernns_amd import _lib
    L, bad = _lib.lib, C.c_void_p(64)  # an address no allocation holds
    E, U = _lib.S5FXP_EBADARG, _lib.S5FXP_EUNSUPPORTED
    # front: audio, S, c, hops_before, sub, state, x, stream
    assert L.s5fxp_stream_stft(bad, 1, 1, 4, 0.0, None, bad, None) == E     # null state
    assert L.s5fxp_stream_stft(bad, 0, 1, 4, 0.0, bad, bad, None) == E      # S < 1
    assert L.s5fxp_stream_stft(bad, 1, 0, 4, 0.0, bad, bad, None) == E      # c outside 1..32
    assert L.s5fxp_stream_stft(bad, 1, 33, 4, 0.0, bad, bad, None) == E
    assert L.s5fxp_stream_stft(bad, 1, 1, -1, 0.0, bad, bad, None) == E     # negative hops_before
    assert L.s5fxp_stream_stft(bad, 1, 1, 4, 0.0, bad, None, None) == E     # null x with F == 1
    assert L.s5fxp_stream_stft(bad, 1, 2, 0, 0.0, bad, None, None) == E     # null x with F == 1 (first push)
    # back: mask, S, c, hops_before, final, state, out, cleaned_mag, stream
    assert L.s5fxp_stream_mask_istft(bad, 1, 1, 4, 0, None, bad, None, None) == E
    assert L.s5fxp_stream_mask_istft(bad, 0, 1, 4, 0, bad, bad, None, None) == E
    assert L.s5fxp_stream_mask_istft(bad, 1, 0, 4, 0, bad, bad, None, None) == E
    assert L.s5fxp_stream_mask_istft(bad, 1, 33, 4, 0, bad, bad, None, None) == E
    assert L.s5fxp_stream_mask_istft(bad, 1, 1, -1, 0, bad, bad, None, None) == E
    assert L.s5fxp_stream_mask_istft(bad, 1, 1, 4, 0, bad, None, None, None) == E   # null out with O == 1
    assert L.s5fxp_stream_mask_istft(bad, 1, 2, 3, 1, bad, None, None, None) == E   # null out (O == 3) before the final check
    assert L.s5fxp_stream_mask_istft(bad, 1, 2, 3, 1, bad, bad, None, None) == U    # final with hops_before < 4
    assert L.s5fxp_stream_mask_istft(bad, 1, 2, 0, 1, bad, bad, None, None) == U


def _stream(d, a, schedule, details=True, **kw):
    """Pushes the hops of a (S, m * 128) per `schedule`, then finish().  Returns the list of per-push results."""
    res, at = [], 0
    for c in schedule:
        res.append(d.push(a[:, at * HOP:(at + c) * HOP], details=details, **kw))
        at += c
    assert at * HOP == a.shape[1] and d.hops == at
    res.append(d.finish(details=details, **kw))
    return res


def _check_counts(res, schedule):
    h = 0
    for (out, x, mask, cm), (c, final) in zip(res, [(c, False) for c in schedule] + [(2, True)]):
        S = out.shape[0]
        assert tuple(out.shape) == (S, O_of(h, c, final) * HOP)
        assert tuple(x.shape) == tuple(mask.shape) == tuple(cm.shape) == (S, F_of(h, c), 257)
        h += c


@pytest.mark.parametrize("schedule", [[14, 1, 5], [1] * 20], ids=["14-1-5", "1x20"])
def test_cpu_stream_denoiser_against_the_restatement(schedule):
    import torch
    from sparsernns_amd import audio
    S, m, amp = 2, 20, 0.05
    a = AK._audio(S, HOP * m, amp, seed=11)
    d = audio.StreamDenoiser(AK._StubModel(), S)
    assert d.latency_hops == 3 and d.hops == 0
    res = _stream(d, torch.from_numpy(a), schedule)
    _check_counts(res, schedule)
    out, x, mask, cm = (torch.cat([r[i] for r in res], dim=1).numpy() for i in range(4))
    z = ref_stft(a)
    assert x.shape == z.shape == (S, m + 1, 257) and out.shape == (S, m * HOP)
    assert AK._maxdiff("x + sub", x.astype(np.float64) + audio.STFT_MAG_MEAN, np.abs(z)) <= ATOL_SPEC * amp
    assert np.array_equal(mask, AK._StubModel().forward_float(torch.from_numpy(x)).numpy())
    mk = mask.astype(np.float64)
    assert AK._maxdiff("cleaned", out, ref_istft(z * (1.0 + mk))) <= ATOL_AUDIO * amp
    assert AK._maxdiff("cleaned_mag", cm, np.abs(z) * (1.0 + mk)) <= ATOL_SPEC * amp
    with pytest.raises(RuntimeError):
        d.push(torch.zeros(S, HOP))  # ended: needs a reset()
    d.reset()
    assert d.hops == 0
    d.push(torch.from_numpy(a[:, :3 * HOP]))
    with pytest.raises(NotImplementedError):
        d.finish()  # fewer than 4 hops: scipy changes nperseg
    with pytest.raises(ValueError):
        d.push(torch.zeros(S, HOP + 1))
    with pytest.raises(ValueError):
        d.push(torch.zeros(S, 33 * HOP))


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU: the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
class _Raw:
    """The two entry points with a state of its own: what StreamDenoiser does without a model."""

    def __init__(self, S, device="cuda"):
        import torch
        from sparsernns_amd import _lib
        self.S, self.h, self.L = S, 0, _lib
        self.state = torch.zeros(S, _lib.lib.s5fxp_stream_audio_state_bytes() // 4, dtype=torch.float32, device=device)

    def front(self, hops, c, sub):
        import torch
        F = F_of(self.h, c)
        x = torch.empty(self.S, F, 257, dtype=torch.float32, device=self.state.device)
        self.L.check(self.L.lib.s5fxp_stream_stft(hops.data_ptr() if hops is not None else None, self.S, c, self.h, sub,
                                                  self.state.data_ptr(), x.data_ptr() if F else None,
                                                  torch.cuda.current_stream().cuda_stream), "s5fxp_stream_stft")
        return x

    def back(self, mask, c, final=False, cleaned_mag=True):
        import torch
        F, n = F_of(self.h, c), O_of(self.h, c, final)
        out = torch.empty(self.S, n * HOP, dtype=torch.float32, device=self.state.device)
        cm = torch.empty(self.S, F, 257, dtype=torch.float32, device=self.state.device) if cleaned_mag else None
        self.L.check(self.L.lib.s5fxp_stream_mask_istft(mask.data_ptr() if mask is not None and F else None, self.S, c, self.h,
                                                        int(final), self.state.data_ptr(), out.data_ptr() if n else None,
                                                        cm.data_ptr() if cleaned_mag and F else None,
                                                        torch.cuda.current_stream().cuda_stream), "s5fxp_stream_mask_istft")
        self.h += c
        return out, cm


def _run_raw(a, masks, schedule, sub, S=None):
    """a: (S, m*128) device audio; masks: (S, m+1, 257) device masks or None.  Returns concatenated (x, out, cleaned_mag)."""
    import torch
    r = _Raw(a.shape[0])
    xs, outs, cms, at = [], [], [], 0
    for c, final in [(c, False) for c in schedule] + [(2, True)]:
        hops = None if final else a[:, at * HOP:(at + c) * HOP].contiguous()
        F, k0 = F_of(r.h, c), max(r.h - 1, 0)
        xs.append(r.front(hops, c, sub))
        mk = masks[:, k0:k0 + F].contiguous() if masks is not None else None
        o, cm = r.back(mk, c, final)
        outs.append(o)
        cms.append(cm)
        at += c
    return torch.cat(xs, 1), torch.cat(outs, 1), torch.cat(cms, 1)


RAW_CASES = [(4, [4]), (4, [1, 1, 1, 1]), (5, [2, 3]), (7, [1, 2, 4]), (40, [3, 5, 16, 13, 3]), (33, [17, 16]), (70, [32, 32, 6])]


@pytest.mark.gpu
@pytest.mark.parametrize("amp", [1.0, 0.02])
@pytest.mark.parametrize("case", RAW_CASES, ids=lambda c: f"m{c[0]}-" + "-".join(map(str, c[1])))
def test_kernels_equal_the_batch_kernels(case, amp):
    import torch
    from sparsernns_amd import audio
    m, schedule = case
    S, T = 3, HOP * m
    a, mk = AK._audio(S, T, amp, seed=m), AK._mask(S, T, seed=m + 1)
    ad, md = torch.from_numpy(a).cuda(), torch.from_numpy(mk).cuda()
    x, out, cm = _run_raw(ad, md, schedule, audio.STFT_MAG_MEAN)
    want_out, want_cm = audio.mask_istft(ad, md, cleaned_mag=True)
    assert tuple(x.shape) == (S, m + 1, 257) and tuple(out.shape) == (S, T)
    assert torch.equal(x, audio.stft_mag(ad))
    assert torch.equal(out, want_out)
    assert torch.equal(cm, want_cm)
    # NULL mask = zero mask = the round trip
    x0, rt, cm0 = _run_raw(ad, None, schedule, 0.0)
    xz, rtz, cmz = _run_raw(ad, torch.zeros_like(md), schedule, 0.0)
    assert torch.equal(rt, rtz) and torch.equal(cm0, cmz) and torch.equal(x0, xz)
    assert torch.equal(rt, audio.mask_istft(ad, None)) and torch.equal(cm0, x0)
    assert AK._maxdiff("round trip vs input", rt.cpu().numpy(), a.astype(np.float64)) <= ATOL_AUDIO * amp


@pytest.mark.gpu
def test_kernels_negative_factor():
    """1 + mask in [-1.5, -0.5], as test_mask_istft_negative_factor."""
    import torch
    from sparsernns_amd import audio
    m, schedule, S = 40, [3, 5, 16, 13, 3], 3
    a, mk = AK._audio(S, HOP * m, seed=21), AK._mask(S, HOP * m, -2.5, -1.5)
    ad, md = torch.from_numpy(a).cuda(), torch.from_numpy(mk).cuda()
    _, out, cm = _run_raw(ad, md, schedule, audio.STFT_MAG_MEAN)
    want_out, want_cm = audio.mask_istft(ad, md, cleaned_mag=True)
    assert torch.equal(out, want_out) and torch.equal(cm, want_cm) and (cm <= 0).all()
    z = ref_stft(a)
    polar = np.abs(z) * (1.0 + mk) * np.exp(1j * np.angle(z))
    assert AK._maxdiff("cleaned", out.cpu().numpy(), ref_istft(polar)) <= ATOL_AUDIO


@pytest.mark.gpu
def test_independence_and_determinism():
    import torch
    from sparsernns_amd import audio
    m, schedule, S = 40, [3, 5, 16, 13, 3], 3
    a, mk = AK._audio(S, HOP * m, seed=31), AK._mask(S, HOP * m, seed=32)
    ad, md = torch.from_numpy(a).cuda(), torch.from_numpy(mk).cuda()
    first = _run_raw(ad, md, schedule, audio.STFT_MAG_MEAN)
    alone = _run_raw(ad[1:2].contiguous(), md[1:2].contiguous(), schedule, audio.STFT_MAG_MEAN)
    again = _run_raw(ad, md, schedule, audio.STFT_MAG_MEAN)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = _run_raw(ad, md, schedule, audio.STFT_MAG_MEAN)
    s.synchronize()
    for f, al, ag, sd in zip(first, alone, again, side):
        assert torch.equal(f[1:2], al) and torch.equal(f, ag) and torch.equal(f, sd)


@pytest.mark.gpu
def test_ragged_length():
    """T = 777: the caller zero-fills the last hop, as scipy's padded=True does."""
    import torch
    from sparsernns_amd import audio
    T, S = 777, 3
    a, mk = AK._audio(S, T, seed=41), AK._mask(S, T, seed=42)
    ad, md = torch.from_numpy(a).cuda(), torch.from_numpy(mk).cuda()
    padded = torch.nn.functional.pad(ad, (0, 7 * HOP - T))
    x, out, cm = _run_raw(padded, md, [3, 4], audio.STFT_MAG_MEAN)
    want_out, want_cm = audio.mask_istft(ad, md, cleaned_mag=True)
    assert torch.equal(x, audio.stft_mag(ad)) and torch.equal(out, want_out) and torch.equal(cm, want_cm)


@pytest.mark.gpu
def test_all_zero_audio():
    import torch
    md = torch.from_numpy(AK._mask(3, HOP * 40)).cuda()
    for t in _run_raw(torch.zeros(3, HOP * 40, device="cuda"), md, [3, 5, 16, 13, 3], 0.0):
        assert torch.count_nonzero(t) == 0  # exactly 0: NaN counts as nonzero


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU: with the model
# ---------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(dim_scale):
    if dim_scale not in _MODELS:
        _MODELS[dim_scale] = AK._model(dim_scale)
    return _MODELS[dim_scale]


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", [[1] * 40, [3, 5, 16, 13, 3]], ids=["1x40", "3-5-16-13-3"])
@pytest.mark.parametrize("dim_scale", [0.5, 0.25])
def test_stream_denoiser_with_the_model(dim_scale, schedule):
    """Claims 1 and 2 (x and the audio are the batch kernels', bit for bit) and 3 (the masks are a fresh SessionPool's for the
    same rows in the same chunks); the first chunk's mask is the CPU oracle's forward of its FLOOR-quantised rows.  The SI-SNR
    against denoise_fused over the whole clip is printed, not asserted: every chunk chooses its own exponents."""
    import torch
    from sparsernns_amd import audio
    model, ib, ie = _model(dim_scale)
    S, m, amp = 2, 40, 0.02
    noisy = (amp * torch.randn(S, HOP * m, generator=torch.Generator().manual_seed(5))).cuda()
    d = audio.StreamDenoiser(model, S)
    res = _stream_clone(d, noisy, schedule)
    _check_counts(res, schedule)
    out, x, mask, cm = (torch.cat([r[i] for r in res], dim=1) for i in range(4))
    assert torch.equal(x, audio.stft_mag(noisy))
    want_out, want_cm = audio.mask_istft(noisy, mask, cleaned_mag=True)
    assert torch.equal(out, want_out) and torch.equal(cm, want_cm)
    pool = model.engine().pool(S)
    for r in res:
        if r[1].shape[1]:
            assert torch.equal(pool.push(r[1]), r[2])
    first = next(r for r in res if r[1].shape[1])
    x0 = first[1].cpu().numpy()
    for s in range(S):  # each session's chunk is its own compute_best batch
        _, mref = AK._oracle_mask(model, x0[s:s + 1], ib, ie)
        assert np.array_equal(first[2][s:s + 1].cpu().numpy(), mref)
    whole = audio.denoise_fused(model, ib, ie, noisy)[0]
    print("SI-SNR of the streamed audio against denoise_fused over the whole clip (dB):",
          audio.si_snr(whole, out).cpu().numpy())
    # after reset() the object reproduces its first run
    d.reset()
    again = _stream_clone(d, noisy, schedule)
    for r, g in zip(res, again):
        for t, u in zip(r, g):
            assert torch.equal(t, u)


def _stream_clone(d, a, schedule):
    """_stream, with every push's results copied before the next push reuses the buffers."""
    res, at = [], 0
    for c in schedule:
        res.append(tuple(t.clone() for t in d.push(a[:, at * HOP:(at + c) * HOP], details=True)))
        at += c
    res.append(tuple(t.clone() for t in d.finish(details=True)))
    return res


@pytest.mark.gpu
def test_no_allocation_in_steady_state():
    import torch
    from sparsernns_amd import audio
    model, _, _ = _model(0.5)
    S = 2
    d = audio.StreamDenoiser(model, S)
    hops = (0.02 * torch.randn(S, HOP, generator=torch.Generator().manual_seed(6))).cuda()
    for _ in range(4):   # the first pushes have shapes of their own (F = 0, O = 0)
        d.push(hops)
    d.push(hops)         # the warm-up push of the steady shape
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(20):
        out = d.push(hops)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert tuple(out.shape) == (S, HOP)
