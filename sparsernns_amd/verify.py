"""Stage-by-stage comparison of two forwards where their planes lie: in device memory.

Both engines leave every intermediate plane of a forward on the device: ``Engine.forward(traces=True)`` the eleven
``s5fxp_layer_trace`` planes of every layer, ``FloatEngine.forward_traced(fq=...)`` ``u / y / g_in / g / h_out / Bu / xs``.
``s5fxp_stage_err`` (include/s5fxp.h, csrc/stage_err.hpp) compares up to 4096 pairs of strided boxes of such planes in two
launches and leaves per pair one record of sums, counts and two exponent histograms.  This module is its driver:

* ``pair`` describes one pair from two tensors or views (no copy: pointer, extents and strides are the tensor's own);
* ``stage_errors`` is one call of the entry, ``stage_errors_host`` the same statement in NumPy float64 -- the reference of every
  test and the path taken for tensors that are not on a GPU;
* ``compare_engines`` runs the integer and the float model on one batch and reports every stage both sides have, for the whole
  batch, per sequence or per time bucket; ``compare_float`` does the same between the fake-quantised and the plain float model;
* ``clip_pair``, ``stage_errors_clips``, ``stage_errors_clips_host``, ``compare_clips`` and ``compare_float_clips`` are the same
  for a list of clips of different lengths: padded planes from ``Engine.clips_traced`` and
  ``FloatEngine.forward_clips_traced``, masked by the clips' lengths on the device (``s5fxp_stage_err_clips``).

The arithmetic, for every element: ``va = a * 2^-a_exp`` in float64 (exact for any int32) or the float32 ``a`` itself,
``vb = b``; an element whose ``a`` or ``b`` is not finite is counted in ``n_nonfinite`` and enters nothing else; with ``relu_a``
a negative ``va`` becomes 0; ``e = |va - vb|``; where ``vb != 0``, ``rel = e / |vb|``.  These are the figures of
``fxpreporter.compute_error``; the medians are bracketed by the two histograms instead of computed.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import StageErrRec, StagePair, TRACE_FIELDS, check, lib
from .floatmodel import HIST_BINS, HIST_EMIN, exp_hist

REC_WORDS = C.sizeof(StageErrRec) // 8
COUNTS = ("n", "n_nonfinite", "n_equal", "n_ref_nonzero")
SUMS = ("sum_abs", "sum_sq", "max_abs", "sum_ref_sq", "sum_rel", "max_rel")
DERIVED = ("abs_error_mean", "abs_error_std", "abs_error_max", "abs_error_med_lo", "abs_error_med_hi", "rel_error_mean",
           "rel_error_max", "rel_error_med_lo", "rel_error_med_hi", "sqnr_db", "equal_share")


class Pair:
    """One pair of boxes: the two tensors (kept alive), their common (nb, rows, cols) extents and both sides' strides."""

    def __init__(self, a: torch.Tensor, b: torch.Tensor, a_exp: int, relu_a: bool):
        self.a, self.b, self.a_exp, self.relu_a = a, b, int(a_exp), bool(relu_a)
        pad = 3 - a.dim()
        self.shape = (1,) * pad + tuple(int(s) for s in a.shape)
        self.a_stride = (0,) * pad + tuple(int(s) for s in a.stride())
        self.b_stride = (0,) * pad + tuple(int(s) for s in b.stride())
        self.kind = _lib.STAGE_I32 if a.dtype == torch.int32 else _lib.STAGE_F32
        self.n = self.shape[0] * self.shape[1] * self.shape[2]

    def fill(self, d: StagePair) -> None:
        d.a, d.b = self.a.data_ptr() if self.n else None, self.b.data_ptr() if self.n else None
        d.a_kind, d.a_exp, d.flags = self.kind, self.a_exp, _lib.STAGE_RELU_A if self.relu_a else 0
        d.nb, d.rows, d.cols = self.shape
        for k in range(3):
            d.a_stride[k], d.b_stride[k] = self.a_stride[k], self.b_stride[k]

    def host(self):
        """(a, b, a_exp, relu_a) with both sides copied to NumPy: what ``stage_errors_host`` computes on."""
        return self.a.detach().cpu().numpy(), self.b.detach().cpu().numpy(), self.a_exp, self.relu_a


def _tensor(v) -> torch.Tensor:
    return v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))


def pair(a, b, a_exp: Optional[int] = None, relu_a: bool = False) -> Pair:
    """The descriptor of one comparison: ``a`` int32 (value = a * 2^-a_exp) or float32, ``b`` float32, the reference side; two
    tensors or views of the same shape and up to three dimensions, on the same device.  Nothing is copied, so
    ``torch.view_as_real(Bu)[..., 0]``, ``plane[s]`` and ``plane[:, t0:t1]`` are boxes of the plane they view.
    ``relu_a``: compare ``max(a, 0)``."""
    a, b = _tensor(a), _tensor(b)
    if a.dtype not in (torch.int32, torch.float32):
        raise ValueError(f"a must be int32 or float32, got {a.dtype}")
    if b.dtype != torch.float32:
        raise ValueError(f"b must be float32, got {b.dtype}")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} must have the same shape")
    if a.dim() > 3:
        raise ValueError(f"at most three dimensions, got {tuple(a.shape)}")
    if a.device != b.device:
        raise ValueError(f"a is on {a.device}, b on {b.device}")
    if any(s >= 2 ** 31 for s in a.shape):
        raise ValueError(f"an extent of {tuple(a.shape)} does not fit 31 bits")
    if a.dtype == torch.int32:
        if a_exp is None or not 0 <= int(a_exp) <= 40:
            raise ValueError(f"an int32 a needs its exponent, 0..40, got {a_exp}")
    return Pair(a, b, 0 if a.dtype == torch.float32 else a_exp, relu_a)


# -- the record and what is derived from it -------------------------------------------------------------------------------
def _edge(k: int) -> float:
    """The least float64 whose float32 rounding is at least 2^k: a value belongs to the bin its float32 rounding falls in."""
    return 2.0 ** k * (1.0 - 2.0 ** -25)


def bin_edges(b: int):
    """[lo, hi) of histogram bin ``b`` in terms of the float64 value that was binned."""
    lo = 0.0 if b == 0 else _edge(b + HIST_EMIN)
    hi = math.inf if b == HIST_BINS - 1 else _edge(b + HIST_EMIN + 1)
    return lo, hi


def median_bracket(hist) -> tuple:
    """(lo, hi) with lo <= np.median(values) <= hi from the values' exponent histogram: the lower edge of the bin that holds
    the lower middle element and the upper edge of the bin that holds the upper one ((0, 0) without values)."""
    h = np.asarray(hist, dtype=np.int64)
    n = int(h.sum())
    if n == 0:
        return 0.0, 0.0
    cum = np.cumsum(h)
    b_lo = int(np.searchsorted(cum, (n - 1) // 2 + 1))
    b_hi = int(np.searchsorted(cum, n // 2 + 1))
    return bin_edges(b_lo)[0], bin_edges(b_hi)[1]


def derive(rec: dict) -> dict:
    """Adds the report's figures to a record (in place): the means divide by the compared elements, n - n_nonfinite (the
    relative ones by n_ref_nonzero).  ``abs_error_std`` is sqrt(sum_sq / n - mean^2), meaningless below the cancellation of
    that formula, 4 n 2^-53 * sum_sq / n in the variance."""
    nf, nz = rec["n"] - rec["n_nonfinite"], rec["n_ref_nonzero"]
    mean = rec["sum_abs"] / nf if nf else 0.0
    rec["abs_error_mean"], rec["abs_error_max"] = mean, rec["max_abs"]
    rec["abs_error_std"] = math.sqrt(max(rec["sum_sq"] / nf - mean * mean, 0.0)) if nf else 0.0
    rec["rel_error_mean"], rec["rel_error_max"] = (rec["sum_rel"] / nz if nz else 0.0), rec["max_rel"]
    rec["abs_error_med_lo"], rec["abs_error_med_hi"] = median_bracket(rec["hist_abs"])
    rec["rel_error_med_lo"], rec["rel_error_med_hi"] = median_bracket(rec["hist_rel"])
    if rec["sum_sq"] > 0.0:
        rec["sqnr_db"] = 10.0 * math.log10(rec["sum_ref_sq"] / rec["sum_sq"]) if rec["sum_ref_sq"] > 0.0 else -math.inf
    else:
        rec["sqnr_db"] = math.inf
    rec["equal_share"] = rec["n_equal"] / nf if nf else 0.0
    return rec


def _host_record(a, b, a_exp: int, relu_a: bool) -> dict:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype not in (np.int32, np.float32) or b.dtype != np.float32 or a.shape != b.shape:
        raise ValueError(f"expected int32 / float32 a and float32 b of one shape, got {a.dtype} {a.shape}, {b.dtype} {b.shape}")
    va = a.astype(np.float64) * 2.0 ** -int(a_exp) if a.dtype == np.int32 else a.astype(np.float64)
    return _value_record(va, b.astype(np.float64), relu_a)


def _value_record(va: np.ndarray, vb: np.ndarray, relu_a: bool) -> dict:
    """The record of the float64 values ``va`` (a NaN or an infinity: not compared) against ``vb``."""
    n = int(va.size)
    fin = np.isfinite(va) & np.isfinite(vb)
    if relu_a:
        va = np.where(va < 0, 0.0, va)
    va, vb = va[fin], vb[fin]
    e = np.abs(va - vb)
    nz = vb != 0
    rel = e[nz] / np.abs(vb[nz])
    with np.errstate(over="ignore"):
        ha, hr = exp_hist(e.astype(np.float32)), exp_hist(rel.astype(np.float32))
    return dict(n=n, n_nonfinite=int(n - e.size), n_equal=int(np.count_nonzero(e == 0)), n_ref_nonzero=int(rel.size),
                sum_abs=float(e.sum()), sum_sq=float((e * e).sum()), max_abs=float(e.max()) if e.size else 0.0,
                sum_ref_sq=float((vb * vb).sum()), sum_rel=float(rel.sum()), max_rel=float(rel.max()) if rel.size else 0.0,
                hist_abs=ha, hist_rel=hr)


def stage_errors_host(pairs_or_arrays: Iterable) -> List[dict]:
    """The statement of ``s5fxp_stage_err`` in NumPy float64: per item -- a ``Pair`` or a tuple ``(a, b[, a_exp[, relu_a]])`` of
    arrays -- the record's fields and the derived figures, as ``stage_errors`` returns them."""
    out = []
    for item in pairs_or_arrays:
        if isinstance(item, Pair):
            a, b, a_exp, relu = item.host()
        else:
            item = tuple(item)
            a, b = np.asarray(item[0]), np.asarray(item[1])
            a_exp = item[2] if len(item) > 2 and item[2] is not None else 0
            relu = bool(item[3]) if len(item) > 3 else False
        out.append(derive(_host_record(a, b, a_exp, relu)))
    return out


class StageCall:
    """One prepared call of ``s5fxp_stage_err``: descriptors, record buffer and workspace.  ``enqueue`` is the entry
    (stream-ordered, no sync), ``records`` reads the records back."""
    DESC, ENTRY, WS_BYTES = StagePair, "s5fxp_stage_err", "s5fxp_stage_err_workspace_bytes"

    def __init__(self, pairs: Sequence[Pair]):
        self.pairs = list(pairs)
        n = len(self.pairs)
        if not 1 <= n <= _lib.STAGE_MAX_PAIRS:
            raise ValueError(f"one call takes 1..{_lib.STAGE_MAX_PAIRS} pairs, got {n}")
        self.device = self.pairs[0].a.device
        if self.device.type != "cuda" or any(p.a.device != self.device for p in self.pairs):
            raise ValueError("every pair of one call must lie on the same GPU")
        self.desc = (self.DESC * n)()
        for p, d in zip(self.pairs, self.desc):
            p.fill(d)
        self.rec = torch.empty(n * REC_WORDS, dtype=torch.int64, device=self.device)
        self.ws = torch.empty(getattr(lib, self.WS_BYTES)(n), dtype=torch.uint8, device=self.device)

    def enqueue(self) -> None:
        with torch.cuda.device(self.device):
            check(getattr(lib, self.ENTRY)(self.desc, len(self.pairs), self.rec.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                           torch.cuda.current_stream().cuda_stream), self.ENTRY)

    def records(self) -> List[dict]:
        words = self.rec.cpu().numpy().reshape(len(self.pairs), REC_WORDS)
        u, f = words.view(np.uint64), words.view(np.float64)
        out = []
        for i in range(len(self.pairs)):
            r = {k: int(u[i, j]) for j, k in enumerate(COUNTS)}
            r.update({k: float(f[i, 4 + j]) for j, k in enumerate(SUMS)})
            r["hist_abs"] = u[i, 10:10 + HIST_BINS].astype(np.int64)
            r["hist_rel"] = u[i, 10 + HIST_BINS:10 + 2 * HIST_BINS].astype(np.int64)
            out.append(derive(r))
        return out


def stage_errors(pairs: Iterable[Pair]) -> List[dict]:
    """Per pair the record's fields (``n``, ``n_nonfinite``, ``n_equal``, ``n_ref_nonzero``, ``sum_abs``, ``sum_sq``, ``max_abs``,
    ``sum_ref_sq``, ``sum_rel``, ``max_rel``, ``hist_abs``, ``hist_rel``) and the derived figures (``DERIVED``): one call of
    ``s5fxp_stage_err`` for up to 4096 pairs (more are taken 4096 at a time).  Pairs that are not on a GPU take
    ``stage_errors_host``."""
    pairs = list(pairs)
    if not pairs:
        return []
    if pairs[0].a.device.type != "cuda":
        return stage_errors_host(pairs)
    out: List[dict] = []
    for i in range(0, len(pairs), _lib.STAGE_MAX_PAIRS):
        call = StageCall(pairs[i:i + _lib.STAGE_MAX_PAIRS])
        call.enqueue()
        out += call.records()
    return out


# -- clips of different lengths: padded boxes, masked by lens on the device ---------------------------------
class StagePairClips(C.Structure):
    """s5fxp_stage_pair_clips: a ``StagePair`` box of padded planes plus the clips' lengths (120 bytes)."""
    _fields_ = [("box", StagePair), ("lens", C.c_void_p), ("a_exp_dev", C.c_void_p), ("a_exp_stride", C.c_int64),
                ("row0", C.c_int32), ("reserved", C.c_int32)]


class ClipPair(Pair):
    """One pair of padded boxes (nb = clips, rows, cols): ``Pair`` plus ``lens`` (nb int32, the same device), the frame index
    ``row0`` of the box's row 0 inside its clip and, optionally, the clips' exponents where a forward left them."""

    def __init__(self, a, b, lens, a_exp, relu_a, row0, a_exp_dev, a_exp_stride):
        super().__init__(a, b, a_exp, relu_a)
        self.lens, self.row0, self.a_exp_dev, self.a_exp_stride = lens, int(row0), a_exp_dev, int(a_exp_stride)

    def fill(self, d: StagePairClips) -> None:
        super().fill(d.box)
        d.lens = self.lens.data_ptr() if self.n else None
        d.a_exp_dev = self.a_exp_dev.data_ptr() if self.a_exp_dev is not None else None
        d.a_exp_stride, d.row0, d.reserved = self.a_exp_stride, self.row0, 0

    def host(self):
        """(a, b, lens, a_exp or the per-clip exponents, relu_a, row0) in NumPy: what ``stage_errors_clips_host`` computes on."""
        exps = self.a_exp
        if self.a_exp_dev is not None and self.kind == _lib.STAGE_I32:
            words = self.a_exp_dev.detach().cpu().numpy().reshape(-1)
            exps = [int(words[b * self.a_exp_stride]) for b in range(self.shape[0])]
        return (self.a.detach().cpu().numpy(), self.b.detach().cpu().numpy(), self.lens.detach().cpu().numpy(), exps, self.relu_a,
                self.row0)


def clip_pair(a, b, lens, a_exp: Optional[int] = None, relu_a: bool = False, row0: int = 0, a_exp_dev=None,
              a_exp_stride: int = 0) -> ClipPair:
    """The descriptor of one ragged comparison: ``a`` and ``b`` as in ``pair``, three-dimensional boxes (clips, rows, cols) of
    PADDED planes; ``lens`` (clips,) int32 on the same device.  Element (e, r, c) is compared iff ``row0 + r < lens[e]``; the
    others are never read.  ``a_exp_dev`` / ``a_exp_stride``: an int32 tensor on the same device whose word
    ``e * a_exp_stride`` (counted from its first element) is clip e's exponent -- ``status.view(-1)[8 + 8 * l + k:]`` with
    stride ``STATUS_WORDS`` for the compute_best exponents a clip launch left; then ``a_exp`` is not needed.  One clip of a box:
    ``clip_pair(a[e:e + 1], b[e:e + 1], lens[e:e + 1], ...)``; a time bucket: ``clip_pair(a[:, t0:t1], b[:, t0:t1], lens,
    row0=t0)``."""
    a, b, lens = _tensor(a), _tensor(b), _tensor(lens)
    if a.dim() != 3:
        raise ValueError(f"a clip pair is a (clips, rows, cols) box, got {tuple(a.shape)}")
    if lens.dtype != torch.int32 or tuple(lens.shape) != (int(a.shape[0]),) or lens.device != a.device or (lens.numel() > 1 and lens.stride(0) != 1):
        raise ValueError(f"lens must be a contiguous int32 ({int(a.shape[0])},) tensor on {a.device}")
    if row0 < 0 or row0 >= 2 ** 31:
        raise ValueError(f"row0 must be 0 .. 2^31 - 1, got {row0}")
    if a_exp_dev is not None:
        a_exp_dev = _tensor(a_exp_dev)
        if a_exp_dev.dtype != torch.int32 or a_exp_dev.device != a.device or not a_exp_dev.is_contiguous():
            raise ValueError(f"a_exp_dev must be a contiguous int32 tensor on {a.device}")
        reach = (int(a.shape[0]) - 1) * int(a_exp_stride)
        if int(a.shape[0]) and not 0 <= reach < a_exp_dev.numel():
            raise ValueError(f"a_exp_dev has {a_exp_dev.numel()} words, clip {int(a.shape[0]) - 1} reads word {reach}")
        if a_exp is None:
            a_exp = 0
    p = pair(a, b, a_exp, relu_a)
    return ClipPair(p.a, p.b, lens, p.a_exp, p.relu_a, row0, a_exp_dev, a_exp_stride)


def _host_record_clips(a, b, lens, exps, relu_a: bool, row0: int) -> dict:
    a, b, lens = np.asarray(a), np.asarray(b), np.asarray(lens)
    if a.dtype not in (np.int32, np.float32) or b.dtype != np.float32 or a.shape != b.shape or a.ndim != 3 or lens.shape != a.shape[:1]:
        raise ValueError(f"expected (clips, rows, cols) int32 / float32 a, float32 b and (clips,) lens, got {a.dtype} {a.shape}, "
                         f"{b.dtype} {b.shape}, {lens.shape}")
    exps = [int(exps)] * a.shape[0] if np.ndim(exps) == 0 else [int(e) for e in exps]
    va, vb = [], []
    for e in range(a.shape[0]):  # gather the rows inside, scale clip by clip
        m = min(max(int(lens[e]) - row0, 0), a.shape[1])
        if a.dtype == np.int32:
            v = a[e, :m].astype(np.float64) * 2.0 ** -exps[e] if 0 <= exps[e] <= 40 else np.full((m, a.shape[2]), np.nan)
        else:
            v = a[e, :m].astype(np.float64)
        va.append(v.reshape(-1))
        vb.append(b[e, :m].astype(np.float64).reshape(-1))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0)
    return _value_record(cat(va), cat(vb), relu_a)


def stage_errors_clips_host(pairs_or_arrays: Iterable) -> List[dict]:
    """The statement of ``s5fxp_stage_err_clips`` in NumPy float64: per item -- a ``ClipPair`` or a tuple ``(a, b, lens[, a_exp
    [, relu_a[, row0]]])`` of arrays, ``a_exp`` one exponent or one per clip -- the rows inside are gathered (``row0 + r <
    lens[e]``), scaled clip by clip (an exponent outside 0..40 makes the clip's elements not comparable: ``n_nonfinite``), and
    ``stage_errors_host``'s arithmetic gives the record and the derived figures."""
    out = []
    for item in pairs_or_arrays:
        if isinstance(item, ClipPair):
            a, b, lens, exps, relu, row0 = item.host()
        else:
            item = tuple(item)
            a, b, lens = item[0], item[1], item[2]
            exps = item[3] if len(item) > 3 and item[3] is not None else 0
            relu = bool(item[4]) if len(item) > 4 else False
            row0 = int(item[5]) if len(item) > 5 else 0
        out.append(derive(_host_record_clips(a, b, lens, exps, relu, row0)))
    return out


class StageCallClips(StageCall):
    """One prepared call of ``s5fxp_stage_err_clips``."""
    DESC, ENTRY, WS_BYTES = StagePairClips, "s5fxp_stage_err_clips", "s5fxp_stage_err_clips_workspace_bytes"


def stage_errors_clips(pairs: Iterable[ClipPair], read: bool = True):
    """``stage_errors`` for ``ClipPair``s: one call of ``s5fxp_stage_err_clips`` for up to 4096 pairs (more are taken 4096 at a
    time); pairs that are not on a GPU take ``stage_errors_clips_host``.  ``read=False`` only enqueues and returns the prepared
    calls, whose ``records()`` read them later (the pairs' tensors are kept alive by the calls)."""
    pairs = list(pairs)
    if not pairs:
        return []
    if pairs[0].a.device.type != "cuda":
        return stage_errors_clips_host(pairs)
    calls = [StageCallClips(pairs[i:i + _lib.STAGE_MAX_PAIRS]) for i in range(0, len(pairs), _lib.STAGE_MAX_PAIRS)]
    for c in calls:
        c.enqueue()
    return [r for c in calls for r in c.records()] if read else calls


# -- the two engines, stage by stage --------------------------------------------------------------------------------------
def trace_exponents(engine, fxp_qconfig: dict) -> List[Dict[str, int]]:
    """Per layer the exponent of every ``TRACE_FIELDS`` plane of the forward ``engine`` has just run.  The static ones come
    from ``fxp_qconfig`` (``u``, ``Bu_*``, ``xs_*`` = x_*, ``ys`` = y from the SSM's activations; ``out2`` = out2.out_exp;
    ``out2_sigmoid`` = out2.out_bits - 2, fxpmodel.py:1097-1103; ``post_GLU`` = multgate.res_exp), ``pre_s5`` and ``residadd``
    are compute_best results, read from the engine's status words: the last BatchNorm op the layer has, and the residual
    add."""
    dyn = engine.layer_exponents()
    out = []
    for i in range(engine.n_layers):
        b = fxp_qconfig["blocks"]
        b = b.get(f"layers_{i}", b)
        act = b["ssm"]["activations"]
        norm = engine._layers[i].norm
        last = "norm_output_scaled_bias" if norm.bias else "norm_output_scaled" if norm.scale else "norm_output_raw"
        e = dict(pre_s5=dyn[i][last], u=act["u"]["exp"], Bu_re=act["Bu_re"]["exp"], Bu_im=act["Bu_im"]["exp"],
                 xs_re=act["x_re"]["exp"], xs_im=act["x_im"]["exp"], ys=act["y"]["exp"], out2=b["out2"]["out_exp"],
                 out2_sigmoid=b["out2"]["out_bits"] - 2, post_GLU=b["multgate"]["res_exp"], residadd=dyn[i]["residadd"])
        out.append({k: int(e[k]) for k in TRACE_FIELDS})
    return out


def _split(rows, by: str, buckets: int):
    """The pairs of ``rows`` = [(name, a, b, a_exp, relu_a)] for one ``by`` mode, with the keys that say which part each is."""
    if by not in ("stage", "sequence", "time"):
        raise ValueError(f'by must be "stage", "sequence" or "time", got {by!r}')
    if by == "time" and buckets < 1:
        raise ValueError(f"buckets must be positive, got {buckets}")
    pairs, keys = [], []
    for name, a, b, a_exp, relu in rows:
        B, L = int(a.shape[0]), int(a.shape[1])
        if by == "stage":
            pairs.append(pair(a, b, a_exp, relu))
            keys.append(dict(name=name))
        elif by == "sequence":
            for s in range(B):
                pairs.append(pair(a[s], b[s], a_exp, relu))
                keys.append(dict(name=name, sequence=s))
        else:
            w = -(-L // buckets)
            for k, t0 in enumerate(range(0, L, w)):
                t1 = min(t0 + w, L)
                pairs.append(pair(a[:, t0:t1], b[:, t0:t1], a_exp, relu))
                keys.append(dict(name=name, bucket=k, t0=t0, t1=t1))
    return pairs, keys


def engine_rows(engine, fengine, x_float, fxp_qconfig: dict, fq=None) -> list:
    """Runs both traced forwards on ``x_float`` (B,L,d_in) and returns the rows ``compare_engines`` compares,
    [(name, a, b, a_exp, relu_a)]: the planes stay on the device."""
    from .fxparray import RoundingMode, fxp_from_fp
    xd = fengine._to_device(x_float)
    if xd.dim() != 3:
        raise ValueError(f"x must be (B, L, {engine.d_in}), got {tuple(xd.shape)}")
    xd = xd.contiguous()
    fx = fxp_from_fp(xd, bits=engine.inp_bits, exp=engine.inp_exp, signed=True, round_mode=RoundingMode.FLOOR, warn_on_clip=False)
    y, tr = engine.forward(fx, traces=True)
    exps = trace_exponents(engine, fxp_qconfig)
    ft = fengine.forward_traced(xd, fq=fq)
    rows = [("inputs", fx.data, xd, fx.exp, False)]
    for i in range(engine.n_layers):
        t, e, p = tr[i], exps[i], f"encoder.layers_{i}."
        f = lambda k: ft[f"l{i}.{k}"]
        bu, xs = torch.view_as_real(f("Bu")), torch.view_as_real(f("xs"))
        rows += [(p + "norm", t["pre_s5"], f("u"), e["pre_s5"], False),
                 (p + "u", t["u"], f("u"), e["u"], False),
                 (p + "mixer.Bu (real)", t["Bu_re"], bu[..., 0], e["Bu_re"], False),
                 (p + "mixer.Bu (imag)", t["Bu_im"], bu[..., 1], e["Bu_im"], False),
                 (p + "mixer.xs (real)", t["xs_re"], xs[..., 0], e["xs_re"], False),
                 (p + "mixer.xs (imag)", t["xs_im"], xs[..., 1], e["xs_im"], False),
                 (p + "mixer.yt", t["ys"], f("y"), e["ys"], False),
                 (p + "mixer.out2", t["out2"], f("g_in"), e["out2"], False),
                 (p + "mixer.out2_sigmoid", t["out2_sigmoid"], f("g"), e["out2_sigmoid"], False),
                 (p + "mixer.output", t["residadd"], f("h_out"), e["residadd"], True)]
    rows.append(("decoder", y.data, ft["out"], y.exp, False))
    return rows


def compare_engines(engine, fengine, x_float, fxp_qconfig: dict, fq=None, by: str = "stage", buckets: int = 8) -> List[dict]:
    """The integer model (``engine``, an ``Engine``) against the float model (``fengine``, a ``FloatEngine`` on the device) on
    one batch ``x_float`` (B,L,d_in): both traced forwards run, and one call of ``s5fxp_stage_err`` compares, named as
    ``fxpreporter.verification_report`` names them,

      ``inputs``; per layer ``norm`` (pre_s5 <-> u), ``u`` (u <-> u), ``mixer.Bu`` and ``mixer.xs`` real and imaginary (raw
      states on both sides), ``mixer.yt`` (ys <-> y), ``mixer.out2`` (out2 <-> g_in), ``mixer.out2_sigmoid`` (<-> g),
      ``mixer.output`` (relu(residadd) <-> h_out); ``decoder``.

    The report's ``post_glu``, ``residadd`` and encoder rows are left out: the float side stores no plane for the first two
    and the integer trace none for the encoder's output; ``mixer.output`` (and the next layer's ``norm``) covers them.
    ``by="sequence"`` gives every row once per sequence (key ``sequence``), ``by="time"`` once per bucket of
    ceil(L / buckets) frames over all sequences (keys ``bucket``, ``t0``, ``t1``).  ``fq`` (``floatmodel.fq_spec``) goes to the
    float side: the same call then measures the integer model against the fake-quantised float model, and ``equal_share`` is
    the share of elements on which the two agree exactly.  Each returned dict holds ``name``, the record and ``DERIVED``."""
    pairs, keys = _split(engine_rows(engine, fengine, x_float, fxp_qconfig, fq), by, buckets)
    return [dict(k, **r) for k, r in zip(keys, stage_errors(pairs))]


def float_rows(fengine, x_float, fq) -> list:
    """The rows ``compare_float`` compares: every plane of the fake-quantised forward against the plain forward's."""
    xd = fengine._to_device(x_float).contiguous()
    plain, quant = fengine.forward_traced(xd), fengine.forward_traced(xd, fq=fq)
    rows = [("h_enc", quant["h_enc"], plain["h_enc"], 0, False)]
    for i in range(fengine.n_layers):
        for k in ("u", "Bu", "xs", "y", "g_in", "g", "h_out"):
            a, b = quant[f"l{i}.{k}"], plain[f"l{i}.{k}"]
            if a.is_complex():
                a, b = torch.view_as_real(a), torch.view_as_real(b)
                rows += [(f"l{i}.{k} (real)", a[..., 0], b[..., 0], 0, False), (f"l{i}.{k} (imag)", a[..., 1], b[..., 1], 0, False)]
            else:
                rows.append((f"l{i}.{k}", a, b, 0, False))
    rows.append(("out", quant["out"], plain["out"], 0, False))
    return rows


def compare_float(fengine, x_float, fq, by: str = "stage", buckets: int = 8) -> List[dict]:
    """The fake-quantised float forward (``fq``) against the plain one, plane for plane (``h_enc``, per layer ``u``, ``Bu``,
    ``xs``, ``y``, ``g_in``, ``g``, ``h_out``, then ``out``), both float32: the per-stage companion of
    ``floatmodel.sensitivity``, which stops at the output.  ``by`` and ``buckets`` as in ``compare_engines``."""
    pairs, keys = _split(float_rows(fengine, x_float, fq), by, buckets)
    return [dict(k, **r) for k, r in zip(keys, stage_errors(pairs))]


# -- the two engines on clips of different lengths ---------------------------------------------------------
_DYN_WORD = dict(norm_input_minus_mean=0, norm_output_raw=1, norm_output_scaled=2, norm_output_scaled_bias=3, residadd=4)


def _padded_clips(fengine, clips):
    """(x (n,Lmax,d_in) float32 on the device, lens (n,) int32 on the device) from a list of (L_e, d_in) float arrays, or from
    ``(x_padded, lens_dev)`` as ``audio.stft_mag_clips`` returns them."""
    if isinstance(clips, tuple) and len(clips) == 2 and isinstance(clips[1], torch.Tensor) and clips[1].dtype == torch.int32 \
            and clips[1].dim() == 1:
        x, lens = fengine._to_device(clips[0]).contiguous(), clips[1].to(fengine.device).contiguous()
        if x.dim() != 3 or x.shape[0] != lens.shape[0]:
            raise ValueError(f"expected x (n, Lmax, d_in) and lens (n,), got {tuple(x.shape)} and {tuple(lens.shape)}")
        return x, lens
    clips = [fengine._to_device(c) for c in clips]
    if not clips or any(c.dim() != 2 or c.shape[1] != clips[0].shape[1] for c in clips):
        raise ValueError("clips must be a non-empty list of (L_e, d_in) arrays")
    ls = [int(c.shape[0]) for c in clips]
    x = torch.zeros(len(clips), max(max(ls), 1), int(clips[0].shape[1]), dtype=torch.float32, device=fengine.device)
    for e, c in enumerate(clips):
        x[e, :ls[e]] = c
    return x, torch.tensor(ls, dtype=torch.int32, device=fengine.device)


def _split_clips(rows, lens, by: str, buckets: int):
    """The ``ClipPair``s of ``rows`` = [(name, a, b, a_exp, relu_a)] for one ``by`` mode; ``a_exp`` is an int or ``(words, stride)``:
    an int32 device tensor whose word ``e * stride`` is clip e's exponent."""
    if by not in ("stage", "clip", "time"):
        raise ValueError(f'by must be "stage", "clip" or "time", got {by!r}')
    if by == "time" and buckets < 1:
        raise ValueError(f"buckets must be positive, got {buckets}")
    pairs, keys = [], []
    for name, a, b, a_exp, relu in rows:
        n, L = int(a.shape[0]), int(a.shape[1])
        dev, stride = a_exp if isinstance(a_exp, tuple) else (None, 0)
        static = None if dev is not None else a_exp
        if by == "stage":
            pairs.append(clip_pair(a, b, lens, static, relu, 0, dev, stride))
            keys.append(dict(name=name))
        elif by == "clip":
            for e in range(n):
                pairs.append(clip_pair(a[e:e + 1], b[e:e + 1], lens[e:e + 1], static, relu, 0, None if dev is None else dev[e * stride:], stride))
                keys.append(dict(name=name, clip=e))
        else:
            w = -(-L // buckets)
            for k, t0 in enumerate(range(0, L, w)):
                t1 = min(t0 + w, L)
                pairs.append(clip_pair(a[:, t0:t1], b[:, t0:t1], lens, static, relu, t0, dev, stride))
                keys.append(dict(name=name, bucket=k, t0=t0, t1=t1))
    return pairs, keys


def clip_rows(engine, fengine, x, lens, fxp_qconfig: dict, fq=None):
    """Runs both traced clip forwards on the padded ``x`` (n,Lmax,d_in) float32 / ``lens`` and returns ``(rows, status)``: the
    rows ``compare_clips`` compares, [(name, a, b, a_exp, relu_a)] with padded planes that stay on the device, and the clips'
    status words (n, STATUS_WORDS) on the device.  ``pre_s5`` and ``residadd`` carry ``(words, stride)`` in place of an
    exponent: where the launch left every clip's compute_best exponent.  Enqueue only, no sync."""
    from .fxparray import RoundingMode, fxp_from_fp
    n = int(x.shape[0])
    fx = fxp_from_fp(x, bits=engine.inp_bits, exp=engine.inp_exp, signed=True, round_mode=RoundingMode.FLOOR, warn_on_clip=False)
    y, tr = engine.clips_traced(fx.data.contiguous(), lens, x_bits=fx.bits, x_exp=fx.exp)
    status = engine.lane_status(0, n)[:n * _lib.STATUS_WORDS]
    ft = fengine.forward_clips_traced(x, lens, fq=fq)
    rows = [("inputs", fx.data, x, fx.exp, False)]
    for i in range(engine.n_layers):
        b = fxp_qconfig["blocks"]
        b = b.get(f"layers_{i}", b)
        act = b["ssm"]["activations"]
        norm = engine._layers[i].norm
        last = "norm_output_scaled_bias" if norm.bias else "norm_output_scaled" if norm.scale else "norm_output_raw"
        word = lambda k: (status[8 + 8 * i + _DYN_WORD[k]:], _lib.STATUS_WORDS)
        t, p = tr[i], f"encoder.layers_{i}."
        f = lambda k: ft[f"l{i}.{k}"]
        bu, xs = torch.view_as_real(f("Bu")), torch.view_as_real(f("xs"))
        rows += [(p + "norm", t["pre_s5"], f("u"), word(last), False),
                 (p + "u", t["u"], f("u"), int(act["u"]["exp"]), False),
                 (p + "mixer.Bu (real)", t["Bu_re"], bu[..., 0], int(act["Bu_re"]["exp"]), False),
                 (p + "mixer.Bu (imag)", t["Bu_im"], bu[..., 1], int(act["Bu_im"]["exp"]), False),
                 (p + "mixer.xs (real)", t["xs_re"], xs[..., 0], int(act["x_re"]["exp"]), False),
                 (p + "mixer.xs (imag)", t["xs_im"], xs[..., 1], int(act["x_im"]["exp"]), False),
                 (p + "mixer.yt", t["ys"], f("y"), int(act["y"]["exp"]), False),
                 (p + "mixer.out2", t["out2"], f("g_in"), int(b["out2"]["out_exp"]), False),
                 (p + "mixer.out2_sigmoid", t["out2_sigmoid"], f("g"), int(b["out2"]["out_bits"]) - 2, False),
                 (p + "mixer.output", t["residadd"], f("h_out"), word("residadd"), True)]
    rows.append(("decoder", y, ft["out"], engine.out_exp, False))
    return rows, status.view(n, _lib.STATUS_WORDS)


def lens_without_wide(status: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """A copy of ``lens`` with a zero for every clip whose status words (n, STATUS_WORDS) carry ``ST_WIDE_INPUT``: such a clip
    has stopped before its first layer and left its y and trace rows untouched, so no comparison may read them.  Computed on
    the device, no sync."""
    wide = (status[:, 0] & _lib.ST_WIDE_INPUT) != 0
    return torch.where(wide, torch.zeros_like(lens), lens)


def _read_clip_records(calls) -> List[dict]:
    return calls if calls and isinstance(calls[0], dict) else [r for c in calls for r in c.records()]


def compare_clips(engine, fengine, clips, fxp_qconfig: dict, fq=None, by: str = "stage", buckets: int = 8) -> List[dict]:
    """``compare_engines`` for clips of different lengths: ``clips`` is a list of (L_e, d_in) float arrays, or ``(x_padded,
    lens_dev)`` as ``audio.stft_mag_clips`` returns them.  Every clip is its own reference batch (its own compute_best
    exponents), yet the whole comparison is one integer launch (``Engine.clips_traced``), the float model's 2 + 3 n_layers
    launches (``FloatEngine.forward_clips_traced``) and the two launches of ``s5fxp_stage_err_clips``, whatever the number of
    clips: the lengths, and the exponents of ``pre_s5`` and ``residadd``, are read from the clips' status words on the device.
    The status words come to the host once, after everything is enqueued: ``NEGSHIFT`` / ``NEGEXP`` raise as in
    ``Engine.forward_clips``; a clip with ``ST_WIDE_INPUT`` (no integer result) is left out -- on the device, by a zeroed entry
    in a copy of ``lens`` -- and its index is listed under the key ``skipped`` of every row.
    The rows and names are ``compare_engines``'s.  ``by="stage"``: one row per stage over all clips; ``by="clip"``: every row
    once per clip (key ``clip``), equal to ``compare_engines`` on that clip alone; ``by="time"``: once per bucket of
    ceil(Lmax / buckets) frames over all clips that reach it (keys ``bucket``, ``t0``, ``t1``)."""
    x, lens = _padded_clips(fengine, clips)
    rows, status = clip_rows(engine, fengine, x, lens, fxp_qconfig, fq)
    pairs, keys = _split_clips(rows, lens_without_wide(status, lens), by, buckets)
    calls = stage_errors_clips(pairs, read=False)
    st = status.cpu().numpy()  # the one read of the status words
    bad = int(np.bitwise_or.reduce(st[:, 0] & ~_lib.ST_WIDE_INPUT))
    if bad & _lib.ST_NEGSHIFT:
        raise ValueError("invalid result_exp: a data-dependent shift came out negative (fxparray.py:619-621)")
    if bad & _lib.ST_NEGEXP:
        raise ValueError("a compute_best exponent came out negative")
    skipped = [int(e) for e in np.nonzero(st[:, 0] & _lib.ST_WIDE_INPUT)[0]]
    return [dict(k, skipped=skipped, **r) for k, r in zip(keys, _read_clip_records(calls))]


def float_clip_rows(fengine, x, lens, fq) -> list:
    """The rows ``compare_float_clips`` compares: every padded plane of the fake-quantised clip forward against the plain one's."""
    plain, quant = fengine.forward_clips_traced(x, lens), fengine.forward_clips_traced(x, lens, fq=fq)
    rows = [("h_enc", quant["h_enc"], plain["h_enc"], 0, False)]
    for i in range(fengine.n_layers):
        for k in ("u", "Bu", "xs", "y", "g_in", "g", "h_out"):
            a, b = quant[f"l{i}.{k}"], plain[f"l{i}.{k}"]
            if a.is_complex():
                a, b = torch.view_as_real(a), torch.view_as_real(b)
                rows += [(f"l{i}.{k} (real)", a[..., 0], b[..., 0], 0, False), (f"l{i}.{k} (imag)", a[..., 1], b[..., 1], 0, False)]
            else:
                rows.append((f"l{i}.{k}", a, b, 0, False))
    rows.append(("out", quant["out"], plain["out"], 0, False))
    return rows


def compare_float_clips(fengine, clips, fq, by: str = "stage", buckets: int = 8) -> List[dict]:
    """``compare_float`` for clips of different lengths (``clips`` as in ``compare_clips``): the fake-quantised clip forward
    against the plain one, plane for plane, masked by the lengths on the device.  ``by``: "stage", "clip" or "time"."""
    x, lens = _padded_clips(fengine, clips)
    pairs, keys = _split_clips(float_clip_rows(fengine, x, lens, fq), lens, by, buckets)
    return [dict(k, **r) for k, r in zip(keys, stage_errors_clips(pairs))]


# -- tables ---------------------------------------------------------------------------------------------------------------
TABLE_COLUMNS = ("n", "abs_error_mean", "abs_error_std", "abs_error_max", "abs_error_med_lo", "abs_error_med_hi", "rel_error_mean",
                 "rel_error_max", "rel_error_med_lo", "rel_error_med_hi", "sqnr_db", "equal_share")


def _where(r: dict) -> str:
    if "sequence" in r:
        return f"seq {r['sequence']}"
    if "clip" in r:
        return f"clip {r['clip']}"
    if "t0" in r:
        return f"t {r['t0']}..{r['t1'] - 1}"
    return ""


def table_markdown(rows: List[dict], title: str = "integer vs float, stage by stage, whole batch", header: Optional[dict] = None) -> str:
    out = [f"# {title}", ""] + [f"- {k}: {v}" for k, v in (header or {}).items()]
    out += ["", "| stage | part | " + " | ".join(TABLE_COLUMNS) + " |", "|---|---|" + "---|" * len(TABLE_COLUMNS)]
    for r in rows:
        out.append(f"| {r['name']} | {_where(r)} | " + " | ".join(f"{r[c]:.4g}" for c in TABLE_COLUMNS) + " |")
    return "\n".join(out) + "\n"


def _plain(v):
    if isinstance(v, np.ndarray):
        return [int(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return str(v)
    return v


def save_table(rows: List[dict], folder: str, stem: str = "stages_device", title: Optional[str] = None, header: Optional[dict] = None) -> None:
    """``stem``.md and ``stem``.json under ``folder``."""
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, stem + ".md"), "w") as f:
        f.write(table_markdown(rows, header=header, **({"title": title} if title else {})))
    with open(os.path.join(folder, stem + ".json"), "w") as f:
        json.dump(dict(header=header or {}, results=[{k: _plain(v) for k, v in r.items()} for r in rows]), f, indent=1)
