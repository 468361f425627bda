"""The audio steps with the model's int16 boundary (csrc/audio_stft.hpp: s5fxp_stft_mag_i16, s5fxp_mask_istft_i16) and the loop
built on them (audio.stft_mag_i16, mask_istft_i16, denoise_fused(boundary="int16")).

Everything here is an exact statement: the int16 x is fxp_from_fp(FLOOR) of the very float the float kernel stores, and the
int16 mask enters as 1 + to_float(mask), so every result equals the float route's bit for bit.
"""
import numpy as np
import pytest

from oracle import fxp_oracle as O
from sparsernns_amd import synth


def _audio(B, T, seed=0):
    """Quiet noise (most |Z| below the 0.0007 offset: negative x), with a loud stretch in sequence 1 whose bins pass the rail of
    every configuration the tests use (|Z| up to ~40 against rails of 8 and below)."""
    rng = np.random.default_rng(seed)
    a = 1e-3 * rng.standard_normal((B, T))
    n = min(T, 400)
    a[1, :n] += 40.0 * np.cos(2 * np.pi * 0.05 * np.arange(n)) + 25.0
    return a.astype(np.float32)


CFGS = [(16, 12), (16, 15), (12, 9), (1, 0)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_audio_int16_entries_reject_bad_arguments_before_any_device_access():
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib
    E, U = _lib.S5FXP_EBADARG, _lib.S5FXP_EUNSUPPORTED
    ok = dict(audio=1, B=2, T=1024, xb=16, xe=12, x=1)
    for bad in (dict(audio=None), dict(x=None), dict(B=0), dict(xb=0), dict(xb=17), dict(xe=-1), dict(xe=32)):
        a = dict(ok, **bad)
        assert lib.s5fxp_stft_mag_i16(a["audio"], a["B"], a["T"], 0.0007, a["xb"], a["xe"], a["x"], None, None) == E, bad
    assert lib.s5fxp_stft_mag_i16(1, 2, 511, 0.0007, 16, 12, 1, None, None) == U
    ok = dict(audio=1, mask=1, me=12, B=2, T=1024, out=1)
    for bad in (dict(audio=None), dict(out=None), dict(B=0), dict(me=-1), dict(me=32)):
        a = dict(ok, **bad)
        assert lib.s5fxp_mask_istft_i16(a["audio"], a["mask"], a["me"], a["B"], a["T"], a["out"], None, None) == E, bad
    assert lib.s5fxp_mask_istft_i16(1, 1, 12, 2, 511, 1, None, None) == U


class _StubModel:
    """An int16-route 'model' that runs anywhere, with the float route defined through it."""
    fxp_qconfig = {"encoder": {"inp_bits": 16, "inp_exp": 12}}
    out_exp = 13

    def forward_int16(self, x, x_bits=None, x_exp=None):
        import torch
        assert x.dtype == torch.int16
        return ((x.to(torch.int32) * 3) % 20011 - 9000).to(torch.int16)

    def forward_float(self, x):
        import torch
        q = torch.from_numpy(O.from_fp(x.numpy(), 16, 12, True, O.FLOOR).data.astype(np.int16))
        return torch.ldexp(self.forward_int16(q).to(torch.float32), torch.tensor(-self.out_exp))


@pytest.mark.parametrize("T", [512, 777])
def test_cpu_tensors_take_the_torch_route(T):
    import torch
    from sparsernns_amd import audio
    a = torch.from_numpy(_audio(2, T, seed=T))
    xf = audio.stft_mag(a)
    for bits, exp in CFGS:
        x = audio.stft_mag_i16(a, bits, exp)
        assert x.dtype == torch.int16 and x.shape == xf.shape
        assert np.array_equal(x.numpy().astype(np.int32), O.from_fp(xf.numpy(), bits, exp, True, O.FLOOR).data)
    x, spec = audio.stft_mag_i16(a, 16, 12, spectrum=True)
    assert torch.equal(spec, audio.stft_mag(a, spectrum=True)[1])
    mask = torch.from_numpy(np.random.default_rng(1).integers(-32768, 32768, tuple(xf.shape)).astype(np.int16))
    for exp in (0, 13, 31):
        out, cm = audio.mask_istft_i16(a, mask, exp, cleaned_mag=True)
        mf = torch.ldexp(mask.to(torch.float32), torch.tensor(-exp))
        wout, wcm = audio.mask_istft(a, mf, cleaned_mag=True)
        assert torch.equal(out, wout) and torch.equal(cm, wcm)
    for bad in (lambda: audio.stft_mag_i16(a, 17, 12), lambda: audio.stft_mag_i16(a, 16, 32),
                lambda: audio.mask_istft_i16(a, mask, 32), lambda: audio.mask_istft_i16(a, mask.to(torch.int32), 12),
                lambda: audio.mask_istft_i16(a, mask[:, :-1], 12)):
        with pytest.raises(ValueError):
            bad()
    model = _StubModel()
    f = audio.denoise_fused(model, 16, 12, a)
    i = audio.denoise_fused(model, 16, 12, a, boundary="int16")
    assert torch.equal(f[0], i[0]) and torch.equal(f[1], i[1])
    assert i[2].dtype == i[3].dtype == torch.int16
    with pytest.raises(ValueError):
        audio.denoise_fused(model, 16, 12, a, boundary="int8")
    model.store_intermediates = True   # such a model runs op by op on FxpArrays: the int16 route says so instead of bypassing it
    with pytest.raises(ValueError):
        audio.denoise_fused(model, 16, 12, a, boundary="int16")


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [512, 513, 2085])
def test_stft_mag_i16_is_the_quantised_float_row(T):
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd.fxparray import RoundingMode, fxp_from_fp
    a = torch.from_numpy(_audio(2, T, seed=T)).cuda()
    xf, zf = audio.stft_mag(a, spectrum=True)
    for bits, exp in CFGS:
        x, z = audio.stft_mag_i16(a, bits, exp, spectrum=True)
        want = fxp_from_fp(xf, bits=bits, exp=exp, signed=True, round_mode=RoundingMode.FLOOR, warn_on_clip=False).data
        hi = (1 << (bits - 1)) - 1
        assert x.dtype == torch.int16 and x.is_contiguous() and tuple(x.shape) == (2, -(-T // 128) + 1, 257)
        # the case is what it claims to be: negative values, and values on both rails' side of the clip
        assert bool((want < 0).any()) and bool((want == hi).any())
        assert torch.equal(x.to(torch.int32), want), f"{int((x.to(torch.int32) != want).sum())} values differ at {(bits, exp)}"
        assert torch.equal(_bits(torch.view_as_real(z)), _bits(torch.view_as_real(zf)))
    # another offset, no spectrum
    x0 = audio.stft_mag_i16(a, 16, 12, sub=0.0)
    want = fxp_from_fp(audio.stft_mag(a, sub=0.0), bits=16, exp=12, signed=True, round_mode=RoundingMode.FLOOR, warn_on_clip=False).data
    assert torch.equal(x0.to(torch.int32), want)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [512, 513, 2085])
def test_mask_istft_i16_is_the_float_route(T):
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd.fxparray import FxpArray
    a = torch.from_numpy(_audio(2, T, seed=T + 1)).cuda()
    n_seg = -(-T // 128) + 1
    m = np.random.default_rng(T).integers(-32768, 32768, (2, n_seg, 257)).astype(np.int16)
    m[0, 0, :5] = (-32768, 32767, 0, 1, -1)
    m[1, -1, -5:] = (-32768, 32767, 0, 1, -1)
    mask = torch.from_numpy(m).cuda()
    for exp in (0, 12, 15, 31):
        mf = FxpArray(mask.to(torch.int32), 16, exp, True).to_float()
        out, cm = audio.mask_istft_i16(a, mask, exp, cleaned_mag=True)
        wout, wcm = audio.mask_istft(a, mf, cleaned_mag=True)
        assert torch.equal(_bits(out), _bits(wout)) and torch.equal(_bits(cm), _bits(wcm)), exp
        assert torch.equal(_bits(audio.mask_istft_i16(a, mask, exp)), _bits(wout))


_LOOP = {}


def _loop_model(name):
    if name not in _LOOP:
        from sparsernns_amd import _lib
        from sparsernns_amd.fxpmodel import build_regression_model
        md, qc, dims = synth.make_model(0.5, calib_L=128)
        kw = dict(engine_flags=_lib.MODEL_FORCE_GENERIC) if name == "generic" else {}
        _LOOP[name] = (build_regression_model(md, qc, dims["n_layers"], **kw), qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"])
    return _LOOP[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ds0.5", "generic"])
def test_denoise_fused_int16_boundary_gives_the_same_audio(name):
    import torch
    from sparsernns_amd import _lib, audio
    from sparsernns_amd.fxparray import FxpArray, RoundingMode, fxp_from_fp
    model, ib, ie = _loop_model(name)
    eng = model.engine()
    noisy = (0.02 * torch.randn(2, 2085, generator=torch.Generator().manual_seed(5))).cuda()
    cleaned, cm, x, mask = audio.denoise_fused(model, ib, ie, noisy)
    cleaned16, cm16, x16, mask16 = audio.denoise_fused(model, ib, ie, noisy, boundary="int16")
    assert int(eng.status[2].item()) == (_lib.PATH_GENERIC if name == "generic" else _lib.PATH_FUSED)
    assert x16.dtype == mask16.dtype == torch.int16
    assert torch.equal(x16.to(torch.int32), fxp_from_fp(x, bits=ib, exp=ie, signed=True, round_mode=RoundingMode.FLOOR).data)
    assert torch.equal(_bits(FxpArray(mask16.to(torch.int32), eng.out_bits, eng.out_exp, True).to_float()), _bits(mask))
    assert torch.equal(cleaned16, cleaned) and torch.equal(cm16, cm)
    clean = noisy * 0.5
    l, s = audio.validate_batch(model, ib, ie, noisy, clean)
    l16, s16 = audio.validate_batch(model, ib, ie, noisy, clean, boundary="int16")
    assert torch.equal(l, l16) and torch.equal(s, s16)
