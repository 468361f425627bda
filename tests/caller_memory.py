"""Helpers of tests/test_caller_memory.py: the poison fills, guard bands round a buffer of exactly the queried size, and the
float model's C entries on buffers the test owns (``FloatEngine`` allocates y and the trace planes itself).
"""
import ctypes as C

import numpy as np

# every byte of a poisoned buffer: zero (the control); int16 32639, float32 3.39e38; int16 -32640, a tiny negative float;
# -1, NaN at both float widths and every flag set
FILLS = (0x00, 0x7F, 0x80, 0xFF)
SENTINEL = 0xA5      # the guard bands' byte: none of the fills
WS_GUARD = 64 << 10  # bytes either side of a workspace
GUARD = 4 << 10      # bytes either side of every other guarded buffer


def fill_id(fill):
    return f"fill{fill:02X}"


def poison(t, fill):
    """Every byte of the contiguous device tensor ``t`` becomes ``fill``; returns ``t``."""
    import torch
    assert t.is_contiguous()
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(fill)
    return t


def poison_at(t, index, fill):
    """Every byte of ``t[index]`` becomes ``fill``; ``index`` addresses leading dimensions of the contiguous tensor ``t`` only."""
    import torch
    assert t.is_contiguous() and t.dim() >= 2
    t.view(torch.uint8)[index] = fill
    return t


def poisoned(shape, dtype, fill):
    import torch
    return poison(torch.empty(shape, dtype=dtype, device="cuda"), fill)


def raw(a):
    """The bytes of a host array or device tensor, flat."""
    if not isinstance(a, np.ndarray):
        a = a.detach().contiguous().cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same_bytes(a, b):
    a, b = raw(a), raw(b)
    return a.shape == b.shape and np.array_equal(a, b)


def is_fill(a, fill):
    return bool((raw(a) == fill).all())


def same_results(a, b, path=""):
    """Two results (nested dicts / lists of host arrays, ints and None) agree in every byte; returns the first path that differs."""
    if isinstance(a, dict):
        assert set(a) == set(b), (path, sorted(a), sorted(b))
        for k in a:
            same_results(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            same_results(u, v, f"{path}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, (path, "one side has no such output")
    elif isinstance(a, (int, bool, str)):
        assert a == b, (path, a, b)
    else:
        assert same_bytes(a, b), (path, int(np.count_nonzero(raw(a) != raw(b))) if raw(a).shape == raw(b).shape else "shapes")


class Band:
    """``nbytes`` bytes on a 256-byte boundary in the middle of a larger buffer, ``guard`` sentinel bytes either side (and up to
    255 more in front, for the alignment).  ``mem`` is the slice a call gets; it holds ``fill`` in every byte."""

    def __init__(self, nbytes, fill, guard=GUARD):
        import torch
        self.nbytes, self.fill = int(nbytes), fill
        self.buf = torch.full((guard + 256 + self.nbytes + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.off = guard + (-(self.buf.data_ptr() + guard)) % 256
        self.mem = self.buf[self.off:self.off + self.nbytes]
        self.mem.fill_(fill)
        assert self.mem.data_ptr() % 256 == 0 and self.off >= guard and self.buf.numel() - self.off - self.nbytes >= guard

    def view(self, dtype, shape=None):
        t = self.mem.view(dtype)
        return t if shape is None else t.view(shape)

    def intact(self):
        h = self.buf.cpu().numpy()
        return bool((h[:self.off] == SENTINEL).all() and (h[self.off + self.nbytes:] == SENTINEL).all())

    def written(self):
        """At least one byte of the slice no longer holds the fill."""
        return not is_fill(self.mem, self.fill)


def band_like(shape, dtype, fill, guard=GUARD):
    """(band, its slice as a tensor of ``shape`` and ``dtype``)."""
    import torch
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    b = Band(n, fill, guard)
    return b, b.view(dtype, shape)


class Buffers:
    """The buffers one call writes.  ``buf(shape, dtype)`` gives a tensor with ``fill`` in every byte: a plain allocation, or with
    ``bands`` a slice of exactly that size between guard bands, which ``check`` then holds intact."""

    def __init__(self, fill, bands=False):
        self.fill, self.bands, self.guards = fill, bands, []

    def __call__(self, shape, dtype, guard=GUARD):
        if not self.bands:
            return poisoned(shape, dtype, self.fill)
        b, t = band_like(shape, dtype, self.fill, guard)
        self.guards.append(b)
        return t

    def workspace(self, nbytes):
        import torch
        return self((int(nbytes),), torch.uint8, WS_GUARD)

    def like(self, t, guard=GUARD):
        return self(tuple(t.shape), t.dtype, guard)

    def check(self, ws):
        """After the call: every guard byte intact, and at least one byte of the workspace slice ``ws`` written."""
        if self.bands:
            assert all(b.intact() for b in self.guards), [i for i, b in enumerate(self.guards) if not b.intact()]
            assert not is_fill(ws, self.fill), "no byte of the workspace slice was written"


# ----------------------------------------------------------------------------------------------------------------------
# the float model on the caller's buffers
# ----------------------------------------------------------------------------------------------------------------------
class FloatBuffers:
    """Everything one float forward writes, allocated here and poisoned: y, the trace planes, the workspace (the engine's cached
    tensor, or ``ws`` when given) -- and stats / hist, which the header makes the caller zero."""

    def __init__(self, eng, B, L, fill, trace, stats=True, hist=False, ws=None, y=None):
        import torch
        from sparsernns_amd import floatmodel
        from sparsernns_amd._lib import lib
        self.eng, self.B, self.L, self.fill, self.trace = eng, B, L, fill, trace
        self.need = lib.s5fxp_float_workspace_bytes(eng._h, B, L, int(trace))
        if ws is None:
            ws = eng._workspace(B, L, trace)
            self.cached = ws.data_ptr()
            if fill is not None:   # None: the call history tests leave what the last call left
                poison(ws, fill)
        self.ws = ws if ws.dtype == torch.float32 else ws.view(torch.float32)
        self.y = poisoned((B, L, eng.d_out), torch.float32, fill) if y is None else y
        self.tr = poisoned((lib.s5fxp_float_trace_bytes(eng._h, B, L) // 4,), torch.float32, fill) if trace else None
        self.stats = eng.new_stats() if stats else None
        self.hist = torch.zeros(len(eng.keys), floatmodel.HIST_BINS, dtype=torch.int64, device="cuda") if hist else None

    def call(self, x, lens=None, fq=None):
        """The C entry of the form: forward, _hist, _fq, _clips or _clips_fq."""
        import torch
        from sparsernns_amd._lib import check, lib
        p = lambda t: None if t is None else t.data_ptr()
        h, B, L = self.eng._h, self.B, self.L
        assert self.ws.numel() * self.ws.element_size() >= self.need
        tail = (self.ws.data_ptr(), self.need, torch.cuda.current_stream().cuda_stream)
        fqp = None if fq is None else np.ascontiguousarray(fq).ctypes.data
        if lens is not None and fq is not None:
            check(lib.s5fxp_float_model_clips_fq(h, x.data_ptr(), B, L, lens.data_ptr(), p(self.y), p(self.stats), fqp, *tail), "clips_fq")
        elif lens is not None:
            check(lib.s5fxp_float_model_clips(h, x.data_ptr(), B, L, lens.data_ptr(), p(self.y), p(self.stats), p(self.hist), *tail), "clips")
        elif fq is not None:
            check(lib.s5fxp_float_model_forward_fq(h, x.data_ptr(), B, L, p(self.y), p(self.stats), fqp, p(self.tr), *tail), "forward_fq")
        elif self.hist is not None:
            check(lib.s5fxp_float_model_forward_hist(h, x.data_ptr(), B, L, p(self.y), p(self.stats), p(self.hist), p(self.tr), *tail),
                  "forward_hist")
        else:
            check(lib.s5fxp_float_model_forward(h, x.data_ptr(), B, L, p(self.y), p(self.stats), p(self.tr), *tail), "forward")
        torch.cuda.synchronize()
        if hasattr(self, "cached"):   # the call used the tensor that was poisoned
            assert self.eng._workspace(B, L, self.trace).data_ptr() == self.cached == self.ws.data_ptr()

    def planes(self, x):
        """Host copies of what ``FloatEngine.forward_traced`` returns, read from these buffers (a traced call)."""
        import torch
        eng, B, L = self.eng, self.B, self.L
        NH, NP2 = B * L * eng.H, B * L * 2 * eng.P
        ws, tr = self.ws.view(-1), self.tr
        host = lambda t: t.cpu().numpy()
        out = dict(out=host(self.y), stats=host(self.stats), h_enc=host(ws[:NH].view(B, L, eng.H)), x=x)
        if self.hist is not None:
            out["hist"] = host(self.hist)
        for i in range(eng.n_layers):
            for j, name in enumerate(("u", "y", "g_in", "g", "h_out")):
                out[f"l{i}.{name}"] = host(tr[(5 * i + j) * NH:(5 * i + j + 1) * NH].view(B, L, eng.H))
            base = 2 * NH + 2 * i * NP2
            out[f"l{i}.Bu"] = host(torch.view_as_complex(ws[base:base + NP2].view(B, L, eng.P, 2).clone()))
            out[f"l{i}.xs"] = host(torch.view_as_complex(ws[base + NP2:base + 2 * NP2].view(B, L, eng.P, 2).clone()))
        return out

    def result(self):
        """What the header defines of an untraced call: y, stats, hist."""
        host = lambda t: None if t is None else t.cpu().numpy()
        return dict(y=host(self.y), stats=host(self.stats), hist=host(self.hist))
