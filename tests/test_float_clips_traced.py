"""The float clip forward with trace planes (s5fxp_float_model_clips_traced, FloatEngine.forward_clips_traced).

The reference is the device's OWN rectangular traced forward on each clip alone, ``forward_traced(x[e:e+1, :len_e], fq=...)``:
rows t < len_e of every plane -- h_enc, per layer u / y / g_in / g / h_out and Bu / xs, and out -- equal it bit for bit, and
what the buffers held in the rows from len_e on (a NaN pattern no kernel produces) is still there.  y and stats equal
``forward_clips_device``'s.  No tolerance appears in this file.  The clip list is tests/test_clips.py's: every edge of the
32-frame tile at Lmax = 100.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from sparsernns_amd import synth
from test_clips import EDGE_LENS

gpu = pytest.mark.gpu
LMAX = 100
SENT32 = 0x7FC0DEAD  # a NaN bit pattern no kernel produces
NAME = "s5fxp_float_model_clips_traced"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported_at_version_115():
    from sparsernns_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "s5fxp.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    assert re.search(r"\b%s\s*\(" % NAME, hdr) and NAME in _lib.EXPORTED_SYMBOLS and hasattr(raw, NAME) and hasattr(_lib.lib, NAME)
    assert _lib.lib.s5fxp_version() == 115


def test_null_arguments_are_refused_before_the_device_is_touched():
    from sparsernns_amd import _lib

    fake = 0x1000  # never dereferenced: the argument checks fail first
    call = _lib.lib.s5fxp_float_model_clips_traced
    ok = dict(m=fake, x=fake, n=1, L=1, lens=fake, y=fake, tr=fake, ws=fake)
    run = lambda **kw: (lambda a: call(a["m"], a["x"], a["n"], a["L"], a["lens"], a["y"], None, None, a["tr"], a["ws"], 1 << 20, None))({**ok, **kw})
    for kw in (dict(m=None), dict(x=None), dict(n=0), dict(L=0), dict(lens=None), dict(y=None), dict(tr=None), dict(ws=None)):
        assert run(**kw) == _lib.S5FXP_EBADARG, kw


def test_python_entry_needs_the_kernels(monkeypatch):
    import torch
    from sparsernns_amd import floatmodel

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    md, _, dims = synth.make_model(0.25)
    eng = floatmodel.FloatEngine(md, dims["n_layers"])
    assert not eng.on_device
    with pytest.raises(RuntimeError):
        eng.forward_clips_traced(torch.zeros(1, 4, 257), torch.tensor([4], dtype=torch.int32))


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _setup(dim):
    from sparsernns_amd import floatmodel

    md, qc, dims = synth.make_model(dim)
    eng = floatmodel.FloatEngine(md, dims["n_layers"])
    assert eng.on_device
    x = synth.make_input(len(EDGE_LENS), LMAX, dims["d_in"], seed=51).copy()
    for e, n in enumerate(EDGE_LENS):
        x[e, n:] = np.nan  # padding rows are never read
    return qc, dims, eng, x


def _spec(dim, kind):
    from sparsernns_amd import floatmodel

    qc, dims, _, _ = _setup(dim)
    if kind == "plain":
        return None
    return floatmodel.fq_spec(qc, dims["n_layers"], recurrence="step" if kind == "step" else "scan")


@gpu
@pytest.mark.parametrize("kind", ["plain", "fq", "step"])
@pytest.mark.parametrize("dim", [0.25, 0.5])
def test_rows_equal_the_rectangular_traced_forward_and_padding_is_never_written(dim, kind):
    import torch
    from sparsernns_amd._lib import lib

    qc, dims, eng, x = _setup(dim)
    fq = _spec(dim, kind)
    n = len(EDGE_LENS)
    xd = torch.from_numpy(x).cuda()
    lens = torch.tensor(EDGE_LENS, dtype=torch.int32, device="cuda")
    # poison everything the entry writes into: y, the trace buffer and the engine's traced workspace
    poison = lambda words: torch.full((words,), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    y = poison(n * LMAX * dims["d_out"]).view(n, LMAX, dims["d_out"])
    tb = poison(lib.s5fxp_float_trace_bytes(eng._h, n, LMAX) // 4)
    eng._workspace(n, LMAX, True).view(torch.int32).fill_(SENT32)
    got = eng.forward_clips_traced(xd, lens, fq=fq, out=y, trace_buf=tb)
    torch.cuda.synchronize()
    got = {k: (torch.view_as_real(v) if v.is_complex() else v).cpu().numpy() for k, v in got.items()}
    # y and stats of the untraced clip forward
    st = eng.new_stats()
    y0 = eng.forward_clips_device(xd, lens, st, fq=fq)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got["stats"]), bits(st.cpu().numpy())), (dim, kind, "stats")
    y0 = y0.cpu().numpy()
    planes = ["h_enc", "out"] + [f"l{i}.{k}" for i in range(dims["n_layers"]) for k in ("u", "Bu", "xs", "y", "g_in", "g", "h_out")]
    assert set(got) == set(planes) | {"stats"}
    for e, L in enumerate(EDGE_LENS):
        assert np.array_equal(bits(got["out"][e, :L]), bits(y0[e, :L])), (dim, kind, e, "y")
        want = None
        if L:
            want = eng.forward_traced(xd[e:e + 1, :L], fq=fq)
            torch.cuda.synchronize()
        for k in planes:
            g = got[k][e]
            assert np.all(bits(g[L:]) == SENT32), (dim, kind, e, k, "rows beyond len were written")
            if L:
                w = want[k]
                w = (torch.view_as_real(w) if w.is_complex() else w).cpu().numpy()[0]
                assert np.array_equal(bits(g[:L]), bits(w)), (dim, kind, e, k, int(np.count_nonzero(bits(g[:L]) != bits(w))))


@gpu
def test_arguments_on_a_real_handle():
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib

    qc, dims, eng, x = _setup(0.25)
    n, L = 2, 40
    xd = torch.zeros(n, L, 257, device="cuda")
    y = torch.zeros(n, L, 257, device="cuda")
    lens = torch.tensor([40, 7], dtype=torch.int32, device="cuda")
    need = lib.s5fxp_float_workspace_bytes(eng._h, n, L, 1)
    assert need > lib.s5fxp_float_workspace_bytes(eng._h, n, L, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    tr = torch.empty(lib.s5fxp_float_trace_bytes(eng._h, n, L), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = lambda trp=tr.data_ptr(), wsb=need, fq=None: lib.s5fxp_float_model_clips_traced(
        eng._h, xd.data_ptr(), n, L, lens.data_ptr(), y.data_ptr(), None, fq, trp, ws.data_ptr(), wsb, s)
    assert call(trp=None) == _lib.S5FXP_EBADARG
    assert call(wsb=lib.s5fxp_float_workspace_bytes(eng._h, n, L, 0)) == _lib.S5FXP_EWORKSPACE   # the untraced size is too small
    bad = (_lib.FloatFqSite * (4 + 10 * dims["n_layers"]))()
    bad[0].bits = 1
    assert call(fq=C.cast(bad, C.c_void_p)) == _lib.S5FXP_EBADARG
    assert call() == _lib.S5FXP_OK
    torch.cuda.synchronize()
