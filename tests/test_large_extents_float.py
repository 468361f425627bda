"""The float model (FloatEngine) and its two scans at extents past 2^32 bytes per plane.  Nothing in the float model couples
the sequences of a batch, so a batch of k copies of R = 7 sequences must repeat the 7-sequence forward bit for bit; that small
forward is held to float64 by the helpers of tests/float_model_ref.py, as in test_float_model.py.  Histograms add up: every
row of the large run is exactly k times the small run's row.
"""
import functools
import time

import numpy as np
import pytest

import float_model_ref as FR
import large_extents as LX
from large_extents import L_REP, P31, P32, R

pytestmark = pytest.mark.gpu
DIM = 1.0


def _report(name, t0, **figures):
    print(f"[large] {name}: {time.perf_counter() - t0:.2f} s " + " ".join(f"{k}={v}" for k, v in figures.items()), flush=True)


@functools.lru_cache(maxsize=None)
def _model():
    from sparsernns_amd import synth
    return synth.make_model(DIM)


def _engine():
    from sparsernns_amd import floatmodel
    md, _, dims = _model()
    eng = floatmodel.FloatEngine(md, dims["n_layers"])
    assert eng.on_device
    return eng


@functools.lru_cache(maxsize=None)
def _x_small():
    from sparsernns_amd import synth
    x = synth.make_input(R, L_REP, _model()[2]["d_in"], seed=4100)
    return x


def _float_need(eng, B, L):
    from sparsernns_amd._lib import lib
    ws = lib.s5fxp_float_workspace_bytes(eng._h, B, L, 0)
    assert ws == 4 * (2 * B * L * eng.H + 4 * B * L * eng.P)
    return B * L * (eng.d_in + eng.d_out) * 4 + ws + LX.chunk_bytes(R * L * eng.d_out)


def test_small_forward_is_held_to_float64():
    """The reference of this file: the traced forward of the 7 sequences, every stage within the float32 chain bound of its
    float64 evaluation, and the hot forward bit for bit the traced one."""
    t0 = time.perf_counter()
    md, _, dims = _model()
    eng = _engine()
    x = _x_small()
    t = {k: v.cpu().numpy() for k, v in eng.forward_traced(x).items()}
    FR.check_stages(md, dims["n_layers"], x, t)
    FR.check_hot_equals_traced(eng, x, t)
    _report("float_small", t0, frames=R * L_REP)
    del eng, t
    LX.release()


def test_float_forward_past_2_32_bytes_per_plane():
    """forward_device at the smallest multiple of 7 sequences whose float (N, H) planes pass 2^32 bytes (the complex64 state
    planes are larger still): y and the observers bit for bit those of the 7 sequences."""
    import torch

    t0 = time.perf_counter()
    eng = _engine()
    B = R * (P32 // (4 * eng.H * L_REP * R) + 1)
    N = B * L_REP
    assert (B - R) * L_REP * eng.H * 4 <= P32 < N * eng.H * 4 and N * eng.P * 8 > P32 and N * eng.d_in * 4 > P32
    LX.memory_guard(_float_need(eng, B, L_REP), f"float forward of {N} frames")
    xs = torch.from_numpy(_x_small()).cuda()
    st_s, st = eng.new_stats(), eng.new_stats()
    ys = eng.forward_device(xs, st_s)
    y = eng.forward_device(LX.repeated(xs, B // R), st)
    torch.cuda.synchronize()
    LX.assert_repeats(y, ys, "float forward")
    assert torch.equal(st.view(torch.int32), st_s.view(torch.int32)), "observers differ"
    _report("float_forward", t0, B=B, frames=N, h_plane=N * eng.H * 4, state_plane=N * eng.P * 8)
    del y, ys, xs, eng
    LX.release()


def test_float_histograms_past_2_31_counts_per_row():
    """forward_device with hist_dev at a batch where the rows of the 257-wide tensors pass 2^31 counts: every row is exactly k
    times the 7-sequence run's row (fm_hist_rows_ok admits the shape; the 32-bit LDS counters do not wrap), and y and the
    observers are unchanged by the histogram."""
    import torch

    t0 = time.perf_counter()
    eng = _engine()
    B = R * (P31 // (eng.d_in * L_REP * R) + 1)
    N, k = B * L_REP, B // R
    assert N * eng.d_in > P31 and N * eng.H * 4 > P32
    LX.memory_guard(_float_need(eng, B, L_REP), f"float histogram forward of {N} frames")
    xs = torch.from_numpy(_x_small()).cuda()
    st_s, st, h_s, h = eng.new_stats(), eng.new_stats(), eng.new_hist(), eng.new_hist()
    ys = eng.forward_device(xs, st_s, hist_dev=h_s)
    y = eng.forward_device(LX.repeated(xs, k), st, hist_dev=h)
    torch.cuda.synchronize()
    LX.assert_repeats(y, ys, "float forward with histograms")
    assert torch.equal(st.view(torch.int32), st_s.view(torch.int32)), "observers differ"
    assert torch.equal(h, h_s * k), "a histogram row is not k times the small run's"
    rows = h.sum(dim=1).cpu().numpy()
    assert int(rows.max()) == N * eng.d_in > P31 and int(rows.min()) > 0
    _report("float_hist", t0, B=B, frames=N, largest_row=int(rows.max()), largest_bin=int(h.max()))
    del y, ys, xs, eng
    LX.release()


CLIP_LENS = (L_REP, 0, 1, L_REP + 77, 33, 2050)   # cycled; the fourth is clamped to Lmax


def test_float_clips_past_2_32_bytes():
    """forward_clips_device on n clips padded to 4099 frames, n * 4099 * 1028 > 2^32: lengths cycle through CLIP_LENS, contents
    through the 7 sequences (period 42).  y -- padding rows keep their sentinel -- equals the 42-clip launch, whose clips each
    equal forward_device on the clip alone; observers equal, histogram rows k-fold."""
    import torch

    t0 = time.perf_counter()
    eng = _engine()
    period, Lmax = R * len(CLIP_LENS), L_REP
    k = P32 // (period * Lmax * eng.H * 4) + 1   # the (n Lmax, H) planes of the workspace pass 2^32 bytes as well
    n = k * period
    assert n * Lmax * eng.d_out * 4 > P32 and n * Lmax * eng.H * 4 > P32
    LX.memory_guard(_float_need(eng, n, Lmax), f"{n} float clips")
    xs7 = torch.from_numpy(_x_small()).cuda()
    xs = xs7[torch.arange(period, device="cuda") % R].contiguous()
    lens_s = torch.tensor([CLIP_LENS[e % len(CLIP_LENS)] for e in range(period)], dtype=torch.int32, device="cuda")
    sent = -123.5
    ys = torch.full((period, Lmax, eng.d_out), sent, device="cuda")
    st_s, st, h_s, h = eng.new_stats(), eng.new_stats(), eng.new_hist(), eng.new_hist()
    eng.forward_clips_device(xs, lens_s, st_s, h_s, out=ys)
    for e in range(period):   # the small launch against the clip alone
        ln = min(int(lens_s[e]), Lmax)
        assert bool((ys[e, ln:] == sent).all()), f"clip {e}: padding written"
        if ln and e < 2 * len(CLIP_LENS):
            one = eng.forward_device(xs[e:e + 1, :ln].contiguous())
            assert torch.equal(one[0].view(torch.int32), ys[e, :ln].view(torch.int32)), f"clip {e} differs from its own forward"
    y = torch.full((n, Lmax, eng.d_out), sent, device="cuda")
    eng.forward_clips_device(LX.repeated(xs, k), LX.repeated(lens_s, k), st, h, out=y)
    torch.cuda.synchronize()
    LX.assert_repeats(y, ys, "float clips")
    assert torch.equal(st.view(torch.int32), st_s.view(torch.int32)) and torch.equal(h, h_s * k)
    _report("float_clips", t0, n=n, y_bytes=n * Lmax * eng.d_out * 4)
    del y, ys, xs, xs7, eng
    LX.release()


@pytest.mark.parametrize("which", ["assoc", "fq"])
def test_scans_past_2_32_bytes(which):
    """s5fxp_assoc_scan_c64 and s5fxp_fq_scan_c64 called directly at B * L * P * 8 > 2^32: the rows repeat with period 7, and
    the result (and the last state) equals the 7-row call bit for bit."""
    import torch
    from sparsernns_amd import synth
    from sparsernns_amd._lib import lib, check

    t0 = time.perf_counter()
    md, _, dims = _model()
    P, L = dims["P"], L_REP
    k = P32 // (R * L * P * 8) + 1
    B = k * R
    assert B * L * P * 8 > P32
    LX.memory_guard(2 * B * L * P * 8 + LX.COPIES_PER_CHUNK * R * L * P * 2, f"{which} scan of {B} rows")
    lam = torch.from_numpy(np.ascontiguousarray(synth.zoh(md["encoder"]["layers_0"]["mixer"])[0])).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    bu_s = torch.randn((R, L, P, 2), generator=g, device="cuda") * 0.01
    if which == "fq":   # inside the exact domain: values on the 2^-12 grid, far below 2^24 steps
        bu_s = torch.round(bu_s * 4096) / 4096
    stream = torch.cuda.current_stream().cuda_stream

    def run(bu):
        b = bu.shape[0]
        xs, last = torch.empty_like(bu), torch.empty((b, P, 2), device="cuda")
        if which == "assoc":
            check(lib.s5fxp_assoc_scan_c64(lam.data_ptr(), bu.data_ptr(), xs.data_ptr(), None, last.data_ptr(), b, L, P, 0, stream), which)
        else:
            check(lib.s5fxp_fq_scan_c64(lam.data_ptr(), bu.data_ptr(), xs.data_ptr(), None, last.data_ptr(), None, b, L, P, 12, 12,
                                        stream), which)
        return xs, last

    xs_s, last_s = run(bu_s)
    xs, last = run(LX.repeated(bu_s, k))
    torch.cuda.synchronize()
    assert float(xs_s.abs().max()) > 0 and bool(torch.isfinite(xs_s).all())
    LX.assert_repeats(xs, xs_s, f"{which} scan")
    LX.assert_repeats(last, last_s, f"{which} scan, last state")
    _report(f"scan_{which}", t0, B=B, bytes=B * L * P * 8)
    del xs, last
    LX.release()


def test_float_size_query_never_wraps_and_the_entries_refuse():
    """Host only.  s5fxp_float_workspace_bytes over B = 2^k up to INT_MAX at several L, with and without trace planes: the true
    size (Python integers) where it fits a size_t, otherwise 0 -- and then 0 for every larger B.  The forward and clip entries
    return S5FXP_EWORKSPACE for such a shape before anything is launched, whatever workspace_bytes claims."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib

    eng = _engine()
    int_max, size_max = 2 ** 31 - 1, 2 ** 64 - 1
    Bs = sorted({2 ** k for k in range(31)} | {2 ** k - 1 for k in range(20, 32)})
    zeros = 0
    for trace in (0, 1):
        for L in (1, L_REP, 4194044, int_max):
            was_zero = False
            for B in Bs:
                true = 4 * (2 * B * L * eng.H + (eng.n_layers if trace else 1) * 4 * B * L * eng.P)
                got = lib.s5fxp_float_workspace_bytes(eng._h, B, L, trace)
                assert got == (true if true <= size_max else 0) and not (was_zero and got), (trace, B, L, got, true)
                was_zero = was_zero or got == 0
            zeros += was_zero
    assert zeros >= 4   # the loop did reach sizes beyond a size_t
    buf = torch.full((1024,), -7.0, device="cuda")
    lens = torch.zeros(16, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    B, L = int_max, 4194044
    assert lib.s5fxp_float_workspace_bytes(eng._h, B, L, 0) == 0
    p = buf.data_ptr()
    assert lib.s5fxp_float_model_forward(eng._h, p, B, L, p, None, None, p, 1 << 63, stream) == _lib.S5FXP_EWORKSPACE
    assert lib.s5fxp_float_model_forward_hist(eng._h, p, B, L, p, None, None, None, p, 1 << 63, stream) == _lib.S5FXP_EWORKSPACE
    assert lib.s5fxp_float_model_clips(eng._h, p, B, L, lens.data_ptr(), p, None, None, p, 1 << 63, stream) == _lib.S5FXP_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all()), "something was launched"
    del eng
    LX.release()
