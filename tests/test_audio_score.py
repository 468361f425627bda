"""The scored masked inverse (csrc/audio_score.hpp: s5fxp_mask_istft_score[_i16], k_score_finalize) and the loop built on it
(audio.score_fused, audio.validate_fused).

Reference on the GPU: a float64 evaluation of fxprun.py:79-88 on the device's own planes, which the unchanged entries produce --
cleaned audio and cleaned_mag from s5fxp_mask_istft, clean magnitude from s5fxp_stft_mag(clean, sub = 0).  The new kernel's
inputs to its sums are those float32 values bit for bit, so only the summation and the float32 rounding of the three results
separate the two:
  si_snr   1e-4 dB.  float32 spacing at 40 dB is 3.8e-6; double sums of <= 5000 exact products carry a relative error of about
           1e-13, which a 40 dB cancellation amplifies by 1e4.  A miscounted hop or tail moves the score by more than 1e-2 dB.
           The bound holds for |si_snr| <= 40 dB, which the tests assert of every case.
  mag_mse  1e-6 relative: float32 rounding (6e-8) plus the double summation.
  loss     lam * mag_mse + (100 - si_snr) recomputed from the returned float32 values, within 1e-5 (float32 spacing at 100
           is 7.6e-6).
Shapes: T = 512 (one tile, both cover edges), 777 (ragged tail), 1664 (one full tile whose last frame lies beyond it), 1700 (a
second tile of one hop), 5000 (four tiles and a tail); B = 1 and 3.

Measured on the MI355X over the twenty (case, lam) runs (si_snr 16.7 .. 18.0 dB): max |si_snr - ref| = 9.5e-7 dB,
max |mag_mse - ref| / ref = 5.1e-8, max |loss - recomputed| = 4.4e-6, max |loss - ref| = 3.7e-6.  validate_fused against
validate_batch (si_snr 3.39 and 0.79 dB): 1.2e-6 dB and 7.6e-6 in the loss."""
import ctypes as C
import functools

import numpy as np
import pytest

from sparsernns_amd import synth

SIZES = [512, 777, 1664, 1700, 5000]
CASES = [(B, T) for T in SIZES for B in (1, 3)]
LAMS = (0.001, 1000.0)


def _ids(c):
    return f"B{c[0]}-T{c[1]}"


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement (tests/test_audio_kernels.py pins the first two to scipy at 1e-12)
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


def ref_scores(cleaned, cleaned_mag, clean, clean_mag, lam):
    """fxprun.py:79-88 in float64 on given planes: (loss, si_snr, mag_mse), each (B)."""
    T = clean.shape[-1]
    si = ref_si_snr(np.asarray(cleaned, np.float64)[:, :T], np.asarray(clean, np.float64))
    mse = ((np.asarray(cleaned_mag, np.float64) - np.asarray(clean_mag, np.float64)) ** 2).mean(axis=(1, 2))
    return lam * mse + (100.0 - si), si, mse


@functools.lru_cache(maxsize=None)
def inputs(B, T):
    """clean: unit-variance noise band-limited to a quarter of the spectrum, plus a DC offset of 0.5 in the last sequence (it
    exercises the mean subtraction); noisy = clean + 0.1 * white noise; mask uniform in +-0.3."""
    rng = np.random.default_rng(1000 * B + T)
    spec = np.fft.rfft(rng.standard_normal((B, T)), axis=-1)
    spec[:, spec.shape[1] // 4:] = 0.0
    clean = np.fft.irfft(spec, n=T, axis=-1)
    clean /= clean.std(axis=-1, keepdims=True)
    clean[-1] += 0.5
    clean = clean.astype(np.float32)
    noisy = (clean + 0.1 * rng.standard_normal((B, T))).astype(np.float32)
    mask = rng.uniform(-0.3, 0.3, (B, -(-T // 128) + 1, 257)).astype(np.float32)
    return noisy, clean, mask


def restated_scores(noisy, clean, mask, lam):
    z = ref_stft(noisy)
    m = np.asarray(mask, np.float64)
    return ref_scores(ref_istft(z * (1.0 + m)), np.abs(z) * (1.0 + m), clean, np.abs(ref_stft(clean)), lam)


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("s5fxp_score_workspace_bytes", "s5fxp_mask_istft_score", "s5fxp_mask_istft_score_i16")


def test_symbols_and_version():
    from sparsernns_amd import _lib
    assert _lib.lib.s5fxp_version() >= 111
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name


def test_workspace_bytes():
    from sparsernns_amd import _lib
    w = _lib.lib.s5fxp_score_workspace_bytes
    assert [w(B, T) for B, T in ((0, 512), (-1, 5000), (1, 511), (3, 0), (1, -7))] == [0] * 5
    # six doubles per tile of 13 output hops
    assert w(1, 512) == 48 and w(1, 1664) == 48 and w(1, 1700) == 96 and w(3, 5000) == 3 * 4 * 48 and w(32, 480000) == 32 * 289 * 48
    sizes = [512, 513, 777, 1664, 1665, 1700, 5000, 480000]
    for B in (1, 2, 3, 32):
        by_t = [w(B, T) for T in sizes]
        assert all(a <= b for a, b in zip(by_t, by_t[1:])) and by_t[0] > 0
        assert all(w(B, T) < w(B + 1, T) for T in sizes)


def _check_arguments():
    """The codes come back for pointers that are not device memory at all: nothing was launched or dereferenced."""
    from sparsernns_amd import _lib
    L, bad, big = _lib.lib, C.c_void_p(64), 1 << 20
    f = lambda a=bad, c=bad, m=bad, B=1, T=512, ws=bad, wb=big, si=bad: \
        L.s5fxp_mask_istft_score(a, c, m, B, T, 0.001, None, None, ws, wb, si, None, None, None)
    g = lambda a=bad, c=bad, m=bad, e=14, B=1, T=512, ws=bad, wb=big, si=bad: \
        L.s5fxp_mask_istft_score_i16(a, c, m, e, B, T, 0.001, bad, bad, ws, wb, si, bad, bad, None)
    for fn in (f, g):
        assert fn(a=None) == _lib.S5FXP_EBADARG
        assert fn(c=None) == _lib.S5FXP_EBADARG
        assert fn(ws=None) == _lib.S5FXP_EBADARG
        assert fn(si=None) == _lib.S5FXP_EBADARG
        assert fn(B=0) == _lib.S5FXP_EBADARG and fn(B=-2) == _lib.S5FXP_EBADARG
        assert fn(T=511) == _lib.S5FXP_EUNSUPPORTED and fn(T=0, m=None) == _lib.S5FXP_EUNSUPPORTED
        assert fn(wb=47) == _lib.S5FXP_EWORKSPACE and fn(wb=0) == _lib.S5FXP_EWORKSPACE
        assert fn(B=3, T=5000, wb=L.s5fxp_score_workspace_bytes(3, 5000) - 1) == _lib.S5FXP_EWORKSPACE
    assert g(e=-1) == _lib.S5FXP_EBADARG and g(e=32) == _lib.S5FXP_EBADARG
    assert g(e=32, T=100) == _lib.S5FXP_EBADARG and f(B=0, T=100) == _lib.S5FXP_EBADARG  # bad arguments come first


def test_argument_validation_needs_no_device():
    _check_arguments()


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_inputs_stay_within_40_db(case):
    """The condition of the si_snr bound, on the float64 restatement of the whole chain."""
    _, si, _ = restated_scores(*inputs(*case), 0.001)
    print("si_snr (dB):", si)
    assert np.all(np.abs(si) <= 40.0)


class _StubModel:
    """A float-route 'model' that runs anywhere: forward_float(x) is a fixed smooth function of x."""
    fxp_qconfig = {"encoder": {"inp_bits": 16, "inp_exp": 12}}

    def forward_float(self, x):
        import torch
        return torch.tanh(40.0 * x) - 0.25


@pytest.mark.parametrize("lam", LAMS)
def test_cpu_score_fused(lam):
    import torch
    from sparsernns_amd import audio
    noisy, clean, mask = inputs(3, 1700)
    nt, ct, mt = (torch.tensor(a) for a in (noisy, clean, mask))
    want = restated_scores(noisy, clean, mask, lam)
    got = audio.score_fused(nt, ct, mt, lam=lam)
    assert len(got) == 3 and all(g.shape == (3,) and g.dtype == torch.float32 for g in got)
    for name, g, w in zip(("loss", "si_snr", "mag_mse"), got, want):
        d = float(np.abs(g.numpy().astype(np.float64) - w).max())
        print(f"{name}: max |diff| = {d:.3e}")
        assert d <= 1e-4
    # the planes on request, the int16 mask, no mask
    l2, s2, m2, out, cm = audio.score_fused(nt, ct, mt, lam=lam, cleaned=True, cleaned_mag=True)
    o_ref, cm_ref = audio.mask_istft(nt, mt, cleaned_mag=True)
    assert torch.equal(out, o_ref) and torch.equal(cm, cm_ref) and torch.equal(l2, got[0]) and torch.equal(s2, got[1])
    assert len(audio.score_fused(nt, ct, mt, cleaned_mag=True)) == 4
    mi = torch.round(mt * 2.0 ** 14).to(torch.int16)
    a = audio.score_fused(nt, ct, mi, lam=lam, mask_exp=14)
    b = audio.score_fused(nt, ct, mi.to(torch.float32) / 2.0 ** 14, lam=lam)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = audio.score_fused(nt, ct, None, lam=lam)
    b = audio.score_fused(nt, ct, torch.zeros_like(mt), lam=lam)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        audio.score_fused(nt, ct[:, :-1], mt)
    with pytest.raises(ValueError):
        audio.score_fused(nt, ct, mt[:, :-1])
    with pytest.raises(ValueError):
        audio.score_fused(nt, ct, mi)            # int16 without its exponent
    with pytest.raises(ValueError):
        audio.score_fused(nt, ct, mt, mask_exp=14)
    with pytest.raises(NotImplementedError):
        audio.score_fused(nt[:, :511], ct[:, :511], None)


def test_cpu_validate_fused():
    import torch
    from sparsernns_amd import audio
    rng = np.random.default_rng(8)
    T, model = 2000, _StubModel()
    clean = (0.05 * rng.standard_normal((3, T))).astype(np.float32)
    noisy = clean + (0.02 * rng.standard_normal((3, T))).astype(np.float32)
    nt, ct = torch.from_numpy(noisy), torch.from_numpy(clean)
    loss, score = audio.validate_fused(model, 16, 12, nt, ct)
    mask = model.forward_float(audio.stft_mag(nt)).numpy()
    ls, si, _ = restated_scores(noisy, clean, mask, 0.001)
    assert loss.shape == score.shape == (3,)
    assert np.abs(score.numpy() - si).max() <= 1e-4 and np.abs(loss.numpy() - ls).max() <= 1e-4
    lb, sb = audio.validate_batch(model, 16, 12, nt, ct)
    assert torch.equal(lb, loss) and torch.equal(sb, score)  # CPU tensors: validate_batch's arithmetic
    with pytest.raises(ValueError):
        audio.validate_fused(model, 16, 12, nt, ct, boundary="int8")


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_case(B, T):
    """The inputs on the device and the planes of the unchanged entries, computed once per case and never written."""
    import torch
    from sparsernns_amd import audio
    nd, cd, md = (torch.tensor(a).cuda() for a in inputs(B, T))
    out, cm = audio.mask_istft(nd, md, cleaned_mag=True)
    clean_mag = audio.stft_mag(cd, sub=0.0)
    planes = tuple(t.cpu().numpy() for t in (out, cm, cd, clean_mag))
    return nd, cd, md, out, cm, planes


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_scores(case):
    from sparsernns_amd import audio
    nd, cd, md, _, _, planes = device_case(*case)
    for lam in LAMS:
        ls, si, mse = ref_scores(*planes, lam)
        assert np.all(np.abs(si) <= 40.0), si
        loss, score, mag_mse = (t.cpu().numpy() for t in audio.score_fused(nd, cd, md, lam=lam))
        assert loss.shape == score.shape == mag_mse.shape == (case[0],) and loss.dtype == score.dtype == mag_mse.dtype == np.float32
        d_si = np.abs(score.astype(np.float64) - si).max()
        d_mse = (np.abs(mag_mse.astype(np.float64) - mse) / mse).max()
        again = np.float64(lam) * mag_mse.astype(np.float64) + (100.0 - score.astype(np.float64))
        d_loss = np.abs(loss.astype(np.float64) - again).max()
        print(f"lam {lam}: si_snr {si} dB, |si_snr - ref| = {d_si:.3e}, |mag_mse - ref| / ref = {d_mse:.3e}, "
              f"|loss - recomputed| = {d_loss:.3e}, |loss - ref| = {np.abs(loss.astype(np.float64) - ls).max():.3e}, "
              f"lam * mag_mse = {lam * mse}")
        assert d_si <= 1e-4
        assert d_mse <= 1e-6
        assert d_loss <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_planes(case):
    """out and cleaned_mag are s5fxp_mask_istft's; the scores do not depend on which planes are stored, nor on the call."""
    import torch
    from sparsernns_amd import audio
    nd, cd, md, out_ref, cm_ref, _ = device_case(*case)
    bare = audio.score_fused(nd, cd, md)
    loss, score, mse, out, cm = audio.score_fused(nd, cd, md, cleaned=True, cleaned_mag=True)
    assert torch.equal(out, out_ref) and torch.equal(cm, cm_ref)
    l3, s3, m3, out3 = audio.score_fused(nd, cd, md, cleaned=True)
    l4, s4, m4, cm4 = audio.score_fused(nd, cd, md, cleaned_mag=True)
    assert torch.equal(out3, out_ref) and torch.equal(cm4, cm_ref)
    for other in ((loss, score, mse), (l3, s3, m3), (l4, s4, m4), audio.score_fused(nd, cd, md)):
        assert all(torch.equal(a, b) for a, b in zip(bare, other))
    # one sequence alone = the same entry of the batch
    if case[0] > 1:
        one = audio.score_fused(nd[1:2], cd[1:2], md[1:2])
        assert all(torch.equal(a, b[1:2]) for a, b in zip(one, bare))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_int16_mask(case):
    """s5fxp_mask_istft_score_i16 at mask_exp 14 = the float entry on to_float(mask), bit for bit."""
    import torch
    from sparsernns_amd import audio
    nd, cd, md, _, _, _ = device_case(*case)
    mi = torch.round(md * 2.0 ** 14).to(torch.int16)
    mf = mi.to(torch.float32) / 2.0 ** 14
    a = audio.score_fused(nd, cd, mi, mask_exp=14, cleaned=True, cleaned_mag=True)
    b = audio.score_fused(nd, cd, mf, cleaned=True, cleaned_mag=True)
    assert len(a) == len(b) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))
    bare = audio.score_fused(nd, cd, mi, mask_exp=14)
    assert all(torch.equal(x, y) for x, y in zip(bare, b))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_null_mask(case):
    import torch
    from sparsernns_amd import audio
    nd, cd, md, _, _, _ = device_case(*case)
    a = audio.score_fused(nd, cd, None, cleaned=True, cleaned_mag=True)
    b = audio.score_fused(nd, cd, torch.zeros_like(md), cleaned=True, cleaned_mag=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(audio.score_fused(nd, cd, None), b))


@pytest.mark.gpu
def test_validate_fused():
    """The model loop on the synthetic dim_scale 0.25 model: both boundaries give the same bits, and validate_batch's numbers
    within the 1e-3 that tests/test_audio_kernels.py::test_validate_batch holds validate_batch to."""
    import torch
    from sparsernns_amd import audio
    from sparsernns_amd.fxpmodel import build_regression_model
    md, qc, dims = synth.make_model(0.25, calib_L=128)
    model = build_regression_model(md, qc, dims["n_layers"])
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    rng = np.random.default_rng(30)
    clean = (0.05 * rng.standard_normal((2, 5000))).astype(np.float32)
    noisy = clean + (0.02 * rng.standard_normal((2, 5000))).astype(np.float32)
    nd, cd = torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()
    loss, score = audio.validate_fused(model, ib, ie, nd, cd)
    loss16, score16 = audio.validate_fused(model, ib, ie, nd, cd, boundary="int16")
    assert tuple(loss.shape) == tuple(score.shape) == (2,)
    assert torch.equal(loss, loss16) and torch.equal(score, score16)
    lb, sb = audio.validate_batch(model, ib, ie, nd, cd)
    d_si, d_loss = float((score - sb).abs().max()), float((loss - lb).abs().max())
    print(f"si_snr {score.cpu().numpy()} dB: |si_snr - validate_batch| = {d_si:.3e}, |loss - validate_batch| = {d_loss:.3e}")
    assert d_si <= 1e-3 and d_loss <= 1e-3


@pytest.mark.gpu
def test_argument_validation_before_any_device_access():
    _check_arguments()
