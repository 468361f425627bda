"""Shared pieces of the large-extent suites (test_large_extents*.py): tensors whose planes pass 2^31 / 2^32 bytes or 2^31
elements, checked against a reference that stays small.

The method is repetition.  Every tensor-wide quantity of the integer model is an extreme, never a sum, so a batch made of k
copies of R sequences gives k copies of the R-sequence output (tests/test_large_extents_oracle.py holds the C oracle to that).
The oracle runs on R x L frames; the device output is compared with it on the device, in chunks.  R = 7 and L = 4099 (prime,
no multiple of any tile): every plane's period has the factor 7, so an offset that wrapped by 2^31 or 2^32 bytes cannot land
on an identical copy -- 2^k is no multiple of a period with an odd factor.
"""
import gc

import numpy as np
import pytest

R = 7
L_REP = 4099
SCAN_DEPTH = 32   # s5fxp_api.hip: the time blocks the recurrence kernels keep in flight (S5_SCANP_ASM_DEPTH)
P31, P32, P30 = 1 << 31, 1 << 32, 1 << 30
# the integer models of the suites: calibrated with one bit of state headroom, so that the fast recurrence rungs stay in range
MODEL_CFG = {1.0: dict(dim_scale=1.0, calib_L=256, state_headroom_bits=1), 0.5: dict(dim_scale=0.5, calib_L=256, state_headroom_bits=1),
             "1.0h2": dict(dim_scale=1.0, calib_L=256, state_headroom_bits=2)}
_CACHE = {}


def model(ds):
    """(export, qconfig, dims) of the integer model at dim_scale ds."""
    if ("model", ds) not in _CACHE:
        from sparsernns_amd import synth
        from sparsernns_amd.fxpmodel import build_regression_model
        md, qc, dims = synth.make_model(**MODEL_CFG[ds])
        _CACHE[("model", ds)] = (build_regression_model(md, qc, dims["n_layers"]).export(), qc, dims)
    return _CACHE[("model", ds)]


def engine(ds, flags=0):
    """A fresh engine (its workspace is released with it: see release)."""
    from sparsernns_amd.engine import Engine
    return Engine(model(ds)[0], flags)


def small_run(ds, L=L_REP, seed=4099):
    """The R-sequence reference, computed once per (ds, L) and never modified: the float input, its integers at the encoder's
    input configuration, and the C oracle's output, bits and exponent."""
    key = ("small", ds, L, seed)
    if key not in _CACHE:
        from oracle import cref
        from oracle import fxp_oracle as O
        from sparsernns_amd import synth
        export, qc, dims = model(ds)
        xf = synth.make_input(R, L, dims["d_in"], seed=seed).astype(np.float32)
        fx = O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
        xi = np.ascontiguousarray(fx.data.astype(np.int32))
        ref, rb, re_, _ = cref.CModel(export).forward(xi, fx.bits, fx.exp)
        for a in (xf, xi, ref):
            a.setflags(write=False)
        _CACHE[key] = dict(xf=xf, xi=xi, x_bits=fx.bits, x_exp=fx.exp, ref=ref, bits=rb, exp=re_)
    return _CACHE[key]


def dev(a):
    """A device copy of a host array (the shared references are read-only: the copy is what torch gets)."""
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def time_blocks(L):
    """TB of ws_layout / fast_ws (s5fxp_api.hip, s5fxp_fast.hpp): 4-step blocks, padded to a multiple of SCAN_DEPTH."""
    return -(-(-(-L // 4)) // SCAN_DEPTH) * SCAN_DEPTH


def plane_sizes(B, L, dims, io_bytes=4, h_bytes=2):
    """name -> (elements, bytes) of every plane of one forward, in Python integers: x, y, the (N, H) planes of the workspace
    (five int16 ones on the fused path, int32 ones on the generic path) and one of the two state streams."""
    N = B * L
    words = (B * time_blocks(L) + SCAN_DEPTH) * dims["P"] * 8
    return {"x": (N * dims["d_in"], N * dims["d_in"] * io_bytes), "y": (N * dims["d_out"], N * dims["d_out"] * io_bytes),
            "h": (N * dims["H"], N * dims["H"] * h_bytes), "stream": (words, words * 4)}


def assert_exceeds(sizes, names, nbytes=None, elements=None):
    """The test's claim about its own shapes: every named plane is beyond the threshold.  A failure here is a test that shrank."""
    for n in names:
        el, by = sizes[n]
        if nbytes is not None:
            assert by > nbytes, f"plane {n}: {by} bytes do not exceed {nbytes}"
        if elements is not None:
            assert el > elements, f"plane {n}: {el} elements do not exceed {elements}"


def memory_guard(need_bytes, what):
    """Skips, with both figures, when `need_bytes` do not fit the free device memory with 10 % to spare."""
    import torch
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if need_bytes * 1.1 > free:
        pytest.skip(f"{what}: needs {need_bytes} bytes (+10 %), the device has {free} of {total} free")
    return free


def release():
    """After a test has dropped its engines and tensors: hand the memory back."""
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


COPIES_PER_CHUNK = 16
CHUNK_FLOOR = 1 << 27   # elements: a small reference is compared many copies at a time


def chunk_copies(ref_numel):
    return max(COPIES_PER_CHUNK, CHUNK_FLOOR // max(ref_numel, 1))


def chunk_bytes(ref_numel):
    """Device bytes one comparison chunk takes: the boolean result of chunk_copies copies."""
    return chunk_copies(ref_numel) * ref_numel


def repeated(small, k):
    """k copies of the device tensor `small` (R, ...) along dim 0, built on the device."""
    return small.repeat((k,) + (1,) * (small.ndim - 1))


def assert_repeats(y, ref, what):
    """y (k * R, ...) equals k copies of ref (R, ...), both on the device, bit for bit; compared in chunks of COPIES_PER_CHUNK
    (or more, of a small reference) copies, so that nothing large is allocated or copied to the host.  Floats are compared as their bits."""
    import torch
    assert y.dtype == ref.dtype and y.shape[0] % ref.shape[0] == 0 and y.shape[1:] == ref.shape[1:], (y.shape, ref.shape)
    if y.dtype == torch.float32:
        y, ref = y.view(torch.int32), ref.view(torch.int32)
    k = y.shape[0] // ref.shape[0]
    yk = y.view((k,) + tuple(ref.shape))
    step = chunk_copies(ref.numel())
    for c0 in range(0, k, step):
        eq = yk[c0:c0 + step] == ref[None]
        if not bool(eq.all()):
            per_copy = (~eq).reshape(eq.shape[0], -1).sum(dim=1)
            bad = int(torch.nonzero(per_copy)[0]) + c0
            idx = torch.nonzero(~eq[bad - c0])[0].tolist()
            raise AssertionError(f"{what}: copy {bad} of {k} differs from the {ref.shape[0]}-sequence reference in "
                                 f"{int(per_copy[bad - c0])} values, first at {idx} (element offset "
                                 f"{bad * ref.numel() + int(np.ravel_multi_index(idx, tuple(ref.shape)))})")
