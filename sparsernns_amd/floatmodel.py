"""The FLOAT model on the device: ``synth.float_forward`` (``calibrate_bn=False``) as HIP kernels, with calibration observers.

``FloatEngine`` wraps ``s5fxp_float_model_*`` (include/s5fxp.h, csrc/float_model.hpp): encoder, per layer
B projection -> ``s5fxp_assoc_scan_c64`` -> gate, decoder -- 2 + 3 * n_layers launches, every contraction on the exact f32
MFMA.  The 4 + 10 * n_layers absmax observers that ``synth.derive_qconfig`` needs are gathered by the same kernels into one
device array (``STAT_KEYS`` gives its order), so a calibration set streams through in batches without a host pass.

The same kernels can gather, per observer, a histogram over the float32 exponent field (``exp_hist``): every
threshold of a fixed-point configuration is a power of two, so the histogram answers exactly which share of a calibration
set saturates or falls below one LSB (``range_report``), and lets the calibration ignore a stated share of outliers
(``clip_absmax``, ``calibrate_clipped``).

Clips of different lengths go through in the same launches (``forward_clips``, ``forward_clips_device``): every
clip gets what its own forward gives, and padding frames are never read, written or observed, so a calibration set that is
ragged is calibrated on its real frames only (``calibrate`` / ``calibrate_clipped`` take ``(x, lens)`` pairs).

Chosen observed tensors can be fake-quantised inside the forward (``fake_quant``, ``fq_spec``, ``fq=`` on every forward;
DESIGN.md §4u): a site that is on rounds its tensor to the grid of its quantiser right after the observer saw it, so
``sensitivity`` can say which of the 34 quantisers costs the output its SQNR, one at a time and all together.

The two things those sites cannot see are modelled too.  ``fq_spec(..., recurrence="step")`` puts a layer's
state sites into mode ``FQ_STEP``: its recurrence then floors four exact products and ``Bu`` at every step, as the integer
recurrence does (``s5fxp_fq_scan_c64``; ``fq_scan`` is the exact statement and the reference of every test).
``quantised_modeldict`` replaces chosen weight groups by the integer model's dequantised values, and ``sensitivity`` takes
``recurrence=`` and ``weights=`` to add those rows to its table.

Results agree with ``synth.float_forward`` to float32 rounding (the summation order differs), not bit for bit.  Without a
GPU, or for a shape the kernels refuse, ``FloatEngine`` runs ``synth.float_forward`` itself and says so: ``on_device`` is False.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, synth
from ._lib import check, lib

F32 = np.float32


def stat_keys(n_layers: int) -> List[str]:
    """The observers in the order ``synth.float_forward`` records them -- the layout of the device array."""
    keys = ["encoder.inp", "encoder.out"]
    for i in range(n_layers):
        keys += [f"l{i}.{k}" for k in ("u", "Bu_re", "Bu_im", "x_re", "x_im", "y", "out2.inp", "out2.out", "gate.l", "gate.r")]
    return keys + ["decoder.inp", "decoder.out"]


STAT_KEYS = stat_keys(3)  # the N-DNS recipe's three layers; stat_keys(n) for any other depth
TRACE_PLANES = ("u", "y", "g_in", "g", "h_out")  # per layer, (N,H) each: the trace buffer's order


HIST_BINS = 64   # S5FXP_FLOAT_HIST_BINS
HIST_EMIN = -40  # S5FXP_FLOAT_HIST_EMIN: bin b in 1..62 holds 2^(b + HIST_EMIN) <= |v| < 2^(b + HIST_EMIN + 1)
HIST_KMIN, HIST_KMAX = HIST_EMIN + 1, HIST_EMIN + HIST_BINS - 1  # the thresholds 2^k a histogram answers exactly: -39 .. 23


def exp_hist(v) -> np.ndarray:
    """int64[64]: the histogram of ``v`` (taken as float32) over the exponent field E = (bits >> 23) & 0xff, bin
    clamp(E - 87, 0, 63).  Bin 0 holds everything below 2^-39 (zero, subnormals), bin 63 |v| >= 2^23, infinities and NaN."""
    bits = np.ascontiguousarray(np.asarray(v, dtype=F32)).view(np.uint32)
    E = ((bits >> 23) & 0xff).astype(np.int64)
    return np.bincount(np.clip(E - (127 + HIST_EMIN), 0, HIST_BINS - 1).ravel(), minlength=HIST_BINS).astype(np.int64)


def tail_count(row, k: int) -> int:
    """T(k) = #{|v| >= 2^k}, exact for HIST_KMIN <= k <= HIST_KMAX."""
    if not HIST_KMIN <= k <= HIST_KMAX:
        raise ValueError(f"the histogram answers thresholds 2^{HIST_KMIN} .. 2^{HIST_KMAX}, not 2^{k}")
    return int(np.asarray(row)[k - HIST_EMIN:].sum())


FQ_SITE = np.dtype([("bits", np.int8), ("exp", np.int8), ("mode", np.uint8), ("saturate", np.uint8)])  # s5fxp_float_fq_site
FQ_MODES = ("floor", "nearest")  # S5FXP_FQ_FLOOR, S5FXP_FQ_NEAREST
FQ_BITS, FQ_EXPS = (2, 24), (-24, 40)  # the fields the entries accept; bits 0 switches a site off
STATE_SITES = ("x_re", "x_im")  # never saturate: the integer model wraps its state (fxpmodel.py:147-172)


def fake_quant(v, bits: int, exp: int, mode: str = "floor", saturate: bool = True) -> np.ndarray:
    """The quantiser of the fake-quantised forward, float32 -> float32:
    q(v) = clamp(R(v * 2^exp), -2^(bits-1), 2^(bits-1) - 1) * 2^-exp, R = floor (the integer model's shifts and input
    conversion) or round-half-to-even (``mode="nearest"``); without ``saturate`` the clamp is left out; NaN stays NaN.
    Computed in float64 and cast: for bits 2..24 and exp -24..40 both products and the rounded integer are exact in float32
    (as long as v * 2^exp is a normal number), so this is the function the kernels compute with four float32 operations.
    The reference of every fake-quantisation test."""
    if mode not in FQ_MODES:
        raise ValueError(f"mode must be one of {FQ_MODES}, got {mode!r}")
    a = np.asarray(v, dtype=F32).astype(np.float64) * 2.0 ** int(exp)
    r = np.floor(a) if mode == "floor" else np.rint(a)
    if saturate:
        r = np.clip(r, -2.0 ** (int(bits) - 1), 2.0 ** (int(bits) - 1) - 1)  # np.clip hands a NaN through
    return (r * 2.0 ** -int(exp)).astype(F32)


FQ_STEP = 2  # S5FXP_FQ_STEP: on a layer's two state sites, the recurrence itself rounds at every step (``fq_scan``)
FQ_STEP_XMAX = 2.0 ** 24  # the domain of ``fq_scan``: every |x| * 2^exp stays below it


def fq_scan(lam, bu, exp_re: int, exp_im: int, x0=None, lens=None, domain: str = "ignore"):
    """The recurrence with the integer model's per-step rounding, the reference of every step-mode test:
    with F(v, e) = floor(v * 2^e) * 2^-e of the EXACT real v, sequentially over time

        xr' = (F(ar xr, exp_re) - F(ai xi, exp_re)) + F(br, exp_re)
        xi' = (F(ar xi, exp_im) + F(ai xr, exp_im)) + F(bi, exp_im)

    ``lam`` (P) and ``bu`` (B,L,P) complex64 (taken as float32 pairs), ``x0`` (B,P) or None (zeros), ``lens`` (B) or None:
    sequence b runs clamp(lens[b], 0, L) steps, its rows behind them are zero -> (xs (B,L,P), x_last (B,P)) complex64,
    x_last the state after a sequence's last step.  Evaluated in float64, where the product of two float32 is exact.
    Inside the DOMAIN -- every |x| * 2^exp below 2^24, every product, br and bi times 2^exp a normal float32 or zero -- every
    sum is exact, so this is one exactly defined float32 function: on grid values it is ``oracle.fxp_oracle.scan`` integer
    for integer (equal exponent pairs, no int32 wrap), and ``s5fxp_fq_scan_c64`` computes it bit for bit.  ``domain``:
    "ignore"; "report" -> (xs, x_last, stayed_inside); "raise" -> ValueError when the run left it.  A NaN in ``bu`` makes
    that state NaN from there on and does not count as leaving the domain."""
    if domain not in ("ignore", "report", "raise"):
        raise ValueError(f'domain must be "ignore", "report" or "raise", got {domain!r}')
    lam, bu = _c64(lam), _c64(bu)
    if bu.ndim != 3 or lam.shape != bu.shape[2:]:
        raise ValueError(f"lam must be (P) and bu (B,L,P), got {lam.shape} and {bu.shape}")
    B, L, P = bu.shape
    ar, ai = lam.real.astype(np.float64), lam.imag.astype(np.float64)
    sr, si = 2.0 ** int(exp_re), 2.0 ** int(exp_im)
    xr, xi = np.zeros((B, P)), np.zeros((B, P))
    if x0 is not None:
        x0 = _c64(x0).reshape(B, P)
        xr, xi = x0.real.astype(np.float64), x0.imag.astype(np.float64)
    n = np.full(B, L) if lens is None else np.clip(np.asarray(lens, dtype=np.int64).reshape(B), 0, L)
    tiny = float(np.finfo(F32).tiny)
    inside = bool((np.abs(xr) * sr < FQ_STEP_XMAX).all() and (np.abs(xi) * si < FQ_STEP_XMAX).all()) if x0 is not None else True

    def F(v, s):
        nonlocal inside
        t = v * s
        a = np.abs(t[live])
        if inside and ((a != 0) & (a < tiny)).any():
            inside = False
        return np.floor(t) / s

    xs = np.zeros((B, L, P), dtype=np.complex64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(int(n.max()) if B else 0):
            live = n > t
            br, bi = bu[:, t].real.astype(np.float64), bu[:, t].imag.astype(np.float64)
            nr = (F(ar * xr, sr) - F(ai * xi, sr)) + F(br, sr)
            ni = (F(ar * xi, si) + F(ai * xr, si)) + F(bi, si)
            xr, xi = np.where(live[:, None], nr, xr), np.where(live[:, None], ni, xi)
            if inside and ((np.abs(xr[live]) * sr >= FQ_STEP_XMAX).any() or (np.abs(xi[live]) * si >= FQ_STEP_XMAX).any()):
                inside = False
            xs[live, t] = (xr + 1j * xi)[live]
    x_last = (xr + 1j * xi).astype(np.complex64)
    if domain == "raise" and not inside:
        raise ValueError("fq_scan: the run left the domain (|x| * 2^exp >= 2^24, or a subnormal v * 2^exp)")
    return (xs, x_last, inside) if domain == "report" else (xs, x_last)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=F32))


def _c64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.complex64))


class _Desc:
    """``s5fxp_float_model_desc`` over a modeldict, with the host arrays it points to kept alive."""

    def __init__(self, modeldict: dict, n_layers: int):
        enc = modeldict["encoder"]
        self.keep: list = []
        self.layers = (_lib.FloatLayerDesc * n_layers)()
        for i in range(n_layers):
            layer = enc[f"layers_{i}"]
            nm = layer["norm"]
            lam_bar, B_bar, Cc = synth.zoh(layer["mixer"])
            d = self.layers[i]
            d.mean, d.var = self._p(_f32(nm["mean"])), self._p(_f32(nm["var"]))
            d.scale = self._p(_f32(nm["scale"])) if "scale" in nm else None
            d.bias = self._p(_f32(nm["bias"])) if "bias" in nm else None
            d.lambda_bar, d.B_bar, d.C = self._p(_c64(lam_bar)), self._p(_c64(B_bar)), self._p(_c64(Cc))
            d.D = self._p(_f32(layer["mixer"]["D"]))
            d.w2, d.b2 = self._p(_f32(layer["out2"]["kernel"])), self._p(_f32(layer["out2"]["bias"]))
        ew, dw = _f32(enc["encoder"]["kernel"]), _f32(modeldict["decoder"]["kernel"])
        P = int(np.asarray(enc["layers_0"]["mixer"]["Lambda_re"]).shape[0])
        self.d_in, self.H, self.P, self.d_out = int(ew.shape[0]), int(ew.shape[1]), P, int(dw.shape[1])
        self.desc = _lib.FloatModelDesc(n_layers=n_layers, d_in=self.d_in, H=self.H, P=P, d_out=self.d_out,
                                        enc_w=self._p(ew), enc_b=self._p(_f32(enc["encoder"]["bias"])), layers=self.layers,
                                        dec_w=self._p(dw), dec_b=self._p(_f32(modeldict["decoder"]["bias"])))

    def _p(self, arr: np.ndarray):
        self.keep.append(arr)
        return arr.view(F32).ctypes.data_as(_lib.F32P)


def supported(modeldict: dict, n_layers: int) -> bool:
    """True when the kernels serve this shape (the four recipe shapes at 257 columns)."""
    return lib.s5fxp_float_model_blob_bytes(C.byref(_Desc(modeldict, n_layers).desc)) > 0


def pack_blob(modeldict: dict, n_layers: int) -> np.ndarray:
    """The packed parameter blob as ``s5fxp_float_model_create`` uploads it, as host float32 (no GPU needed)."""
    d = _Desc(modeldict, n_layers)
    nbytes = lib.s5fxp_float_model_blob_bytes(C.byref(d.desc))
    if nbytes == 0:
        raise NotImplementedError(f"the float kernels do not serve d_in={d.d_in} H={d.H} P={d.P} d_out={d.d_out}")
    blob = np.empty(nbytes // 4, dtype=F32)
    check(lib.s5fxp_float_model_pack(C.byref(d.desc), blob.ctypes.data, nbytes), "s5fxp_float_model_pack")
    return blob


class FloatEngine:
    """The float forward of one modeldict.  ``forward`` mirrors ``synth.float_forward`` in keys and dtypes."""

    def __init__(self, modeldict: dict, n_layers: int, device: Optional[torch.device] = None):
        self.modeldict, self.n_layers = modeldict, int(n_layers)
        self.keys = stat_keys(self.n_layers)
        d = _Desc(modeldict, self.n_layers)
        self.d_in, self.H, self.P, self.d_out = d.d_in, d.H, d.P, d.d_out
        self._h = None
        self.on_device = bool(torch.cuda.is_available()) and lib.s5fxp_float_model_blob_bytes(C.byref(d.desc)) > 0
        if not self.on_device:
            self.device = torch.device("cpu")
            return
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        nbytes = lib.s5fxp_float_model_blob_bytes(C.byref(d.desc))
        self.blob = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.s5fxp_float_model_create(C.byref(d.desc), self.blob.data_ptr(), nbytes,
                                               torch.cuda.current_stream().cuda_stream, C.byref(handle)), "s5fxp_float_model_create")
        self._h = handle
        self._ws: Dict[bool, torch.Tensor] = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib.s5fxp_float_model_destroy(h)
            self._h = None

    # -- device side ---------------------------------------------------------------------------
    def new_stats(self) -> torch.Tensor:
        """A zeroed observer array: 4 + 10 * n_layers float32 on the engine's device."""
        return torch.zeros(len(self.keys), dtype=torch.float32, device=self.device)

    def stats_dict(self, stats_dev: torch.Tensor) -> Dict[str, float]:
        return {k: float(v) for k, v in zip(self.keys, stats_dev.cpu().numpy())}

    def new_hist(self) -> torch.Tensor:
        """A zeroed histogram array: (4 + 10 * n_layers, 64) int64 on the engine's device, rows in ``keys`` order."""
        return torch.zeros(len(self.keys), HIST_BINS, dtype=torch.int64, device=self.device)

    def hist_dict(self, hist_dev: torch.Tensor) -> Dict[str, np.ndarray]:
        return {k: row.copy() for k, row in zip(self.keys, hist_dev.cpu().numpy())}

    def _fq_arg(self, fq, hist) -> Optional[np.ndarray]:
        if fq is not None and hist is not None:
            raise ValueError("fake quantisation together with the histogram is not offered: pass fq or hist, not both")
        return _check_fq(fq, self.keys)

    def _workspace(self, B: int, L: int, trace: bool) -> torch.Tensor:
        n = lib.s5fxp_float_workspace_bytes(self._h, B, L, int(trace)) // 4
        ws = self._ws.get(trace)
        if ws is None or ws.numel() < n:
            ws = self._ws[trace] = torch.empty(n, dtype=torch.float32, device=self.device)
        return ws

    def _device_forward(self, clips: bool, x, lens, stats_dev, hist_dev, out, trace: bool, fq, trace_buf=None):
        """The one device forward behind ``forward_device``, ``forward_clips_device`` and ``forward_clips_traced``: the checks of
        every argument, the buffers and the C entry that serves the form -> (y, trace buffer or None, workspace).  ``trace_buf``:
        the trace buffer to write into instead of a fresh one."""
        if not self.on_device:
            raise RuntimeError(f"FloatEngine.{'forward_clips_device' if clips else 'forward_device'} needs the kernels (on_device is False)")
        fq = self._fq_arg(fq, hist_dev)
        if x.dim() != 3 or x.shape[2] != self.d_in or x.dtype != torch.float32 or x.device != self.device:
            raise ValueError(f"x must be float32 ({'n, Lmax' if clips else 'B, L'}, {self.d_in}) on {self.device}, "
                             f"got {x.dtype} {tuple(x.shape)} on {x.device}")
        B, L = int(x.shape[0]), int(x.shape[1])
        if clips and (not isinstance(lens, torch.Tensor) or lens.dtype != torch.int32 or tuple(lens.shape) != (B,)
                      or lens.device != self.device):
            raise ValueError(f"lens must be an int32 ({B},) tensor on {self.device}")
        if stats_dev is not None and (stats_dev.dtype != torch.float32 or stats_dev.numel() != len(self.keys)
                                      or stats_dev.device != self.device or not stats_dev.is_contiguous()):
            raise ValueError(f"stats must be {len(self.keys)} contiguous float32 on {self.device}")
        if hist_dev is not None and (hist_dev.dtype != torch.int64 or hist_dev.numel() != len(self.keys) * HIST_BINS
                                     or hist_dev.device != self.device or not hist_dev.is_contiguous()):
            raise ValueError(f"hist must be {len(self.keys)} x {HIST_BINS} contiguous int64 on {self.device}")
        shape = (B, L, self.d_out)
        if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.device
                                or not out.is_contiguous()):
            raise ValueError(f"out must be contiguous float32 {shape} on {self.device}")
        x = x.contiguous()
        lens = lens.contiguous() if clips else None  # both held until the launches are enqueued
        y = out if out is not None else torch.empty(shape, dtype=torch.float32, device=self.device)
        ws = self._workspace(B, L, trace)
        nt = lib.s5fxp_float_trace_bytes(self._h, B, L) // 4
        if trace_buf is not None and (not trace or trace_buf.dtype != torch.float32 or trace_buf.numel() != nt
                                      or trace_buf.device != self.device or not trace_buf.is_contiguous()):
            raise ValueError(f"trace_buf must be {nt} contiguous float32 on {self.device}, of a traced forward")
        tr = trace_buf if trace_buf is not None else torch.empty(nt, dtype=torch.float32, device=self.device) if trace else None
        h, xp, yp, trp = self._h, x.data_ptr(), y.data_ptr(), None if tr is None else tr.data_ptr()
        st, hp = None if stats_dev is None else stats_dev.data_ptr(), None if hist_dev is None else hist_dev.data_ptr()
        with torch.cuda.device(self.device):
            tail = (ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
            if clips and trace:  # with or without fq (forward_clips_traced: no histogram is offered)
                check(lib.s5fxp_float_model_clips_traced(h, xp, B, L, lens.data_ptr(), yp, st, None if fq is None else fq.ctypes.data,
                                                         trp, *tail), "s5fxp_float_model_clips_traced")
            elif clips and fq is not None:
                check(lib.s5fxp_float_model_clips_fq(h, xp, B, L, lens.data_ptr(), yp, st, fq.ctypes.data, *tail), "s5fxp_float_model_clips_fq")
            elif clips:
                check(lib.s5fxp_float_model_clips(h, xp, B, L, lens.data_ptr(), yp, st, hp, *tail), "s5fxp_float_model_clips")
            elif fq is not None:
                check(lib.s5fxp_float_model_forward_fq(h, xp, B, L, yp, st, fq.ctypes.data, trp, *tail), "s5fxp_float_model_forward_fq")
            elif hist_dev is not None:
                check(lib.s5fxp_float_model_forward_hist(h, xp, B, L, yp, st, hp, trp, *tail), "s5fxp_float_model_forward_hist")
            else:
                check(lib.s5fxp_float_model_forward(h, xp, B, L, yp, st, trp, *tail), "s5fxp_float_model_forward")
        return y, tr, ws

    def forward_device(self, x: torch.Tensor, stats_dev: Optional[torch.Tensor] = None, trace: bool = False,
                       hist_dev: Optional[torch.Tensor] = None, fq=None):
        """x (B,L,257) float32 on the device -> y (B,L,257); ``stats_dev`` (``new_stats``) is raised in place, ``hist_dev``
        (``new_hist``) is added to in place.  With ``trace`` also (trace buffer, workspace): the planes of ``forward_traced``
        as flat tensors.  ``fq`` (``fq_spec``) fake-quantises the observed tensors whose site is on, each right
        after it entered its observer (``s5fxp_float_model_forward_fq``); not together with ``hist_dev``.  Stream-ordered, no
        sync."""
        y, tr, ws = self._device_forward(False, x, None, stats_dev, hist_dev, None, trace, fq)
        return (y, tr, ws) if trace else y

    def forward_clips_device(self, x: torch.Tensor, lens, stats_dev: Optional[torch.Tensor] = None,
                             hist_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, fq=None) -> torch.Tensor:
        """n clips of different lengths in the launches of ONE forward (``s5fxp_float_model_clips``): x
        (n,Lmax,257) float32 on the device, padded; lens (n,) int32 on the device, as ``audio.stft_mag_clips`` writes it, clip e
        having len_e = clamp(lens[e], 0, Lmax) frames -> y (n,Lmax,257).  y[e, :len_e], ``stats_dev`` and ``hist_dev`` get bit for
        bit what ``forward_device(x[e:e+1, :len_e], ...)`` gives clip after clip: padding rows are never read, never written and
        never observed.  ``out``: the tensor to write into; otherwise y is fresh and its padding unspecified.  ``fq`` as in
        ``forward_device`` (``s5fxp_float_model_clips_fq``).  Stream-ordered, no sync."""
        return self._device_forward(True, x, lens, stats_dev, hist_dev, out, False, fq)[0]

    def _merge(self, st, hd, stats: Optional[dict], hist: Optional[dict]) -> None:
        """One forward's device arrays into the caller's dicts: ``stats`` by maximum, ``hist`` by addition."""
        if hist is not None:
            for k, row in self.hist_dict(hd).items():
                hist[k] = hist.get(k, 0) + row
        if stats is not None:
            for k, v in self.stats_dict(st).items():
                stats[k] = max(stats.get(k, 0.0), v)

    def forward_clips(self, clips, stats: Optional[dict] = None, hist: Optional[dict] = None, fq=None) -> list:
        """A list of (len_e, 257) float32 clips, NumPy arrays or tensors -> the list of the model's outputs, each of its clip's
        kind: per clip what ``forward(clip[None])[0]`` returns, ``stats`` and ``hist`` updated as by those calls.  On the
        device the clips are padded once and take ``forward_clips_device``; otherwise ``synth.float_forward`` runs clip by
        clip.  ``fq`` as in ``forward``."""
        fq = self._fq_arg(fq, hist)
        clips = list(clips)
        for c in clips:
            if len(c.shape) != 2 or c.shape[1] != self.d_in:
                raise ValueError(f"every clip must be (len, {self.d_in}), got {tuple(c.shape)}")
        if not self.on_device:
            return [self.forward(c[None], stats=stats, hist=hist, fq=fq)[0] for c in clips]
        if not clips:
            return []
        ls = [int(c.shape[0]) for c in clips]
        x = torch.zeros(len(clips), max(max(ls), 1), self.d_in, dtype=torch.float32, device=self.device)
        for e, c in enumerate(clips):
            x[e, :ls[e]] = self._to_device(c)
        st = self.new_stats() if stats is not None else None
        hd = self.new_hist() if hist is not None else None
        y = self.forward_clips_device(x, torch.tensor(ls, dtype=torch.int32, device=self.device), st, hd, fq=fq)
        self._merge(st, hd, stats, hist)
        return [y[e, :ls[e]].to(c.device) if isinstance(c, torch.Tensor) else y[e, :ls[e]].cpu().numpy() for e, c in enumerate(clips)]

    def forward_traced(self, x, hist: bool = False, fq=None) -> dict:
        """Every plane of one forward, as device tensors: ``h_enc`` (B,L,H), ``out`` (B,L,257), ``stats`` (the observer array
        of this forward alone), with ``hist`` also ``hist`` (its histogram array), and per layer ``l{i}.u / y / g_in / g / h_out`` (B,L,H) float32 and ``l{i}.Bu / xs`` (B,L,P)
        complex64 (``xs`` raw, before the complex ReLU).  Under ``fq`` the planes hold what downstream consumed: ``u``, ``y``,
        ``g_in``, ``g``, ``Bu`` and ``out`` are post-quantiser, ``xs`` stays raw (its site acts where the gate kernel reads it)."""
        if fq is not None and hist:
            raise ValueError("fake quantisation together with the histogram is not offered: pass fq or hist, not both")
        xd = self._to_device(x)
        B, L = int(xd.shape[0]), int(xd.shape[1])
        st = self.new_stats()
        hd = self.new_hist() if hist else None
        y, tr, ws = self.forward_device(xd, st, trace=True, hist_dev=hd, fq=fq)
        out = self._planes(y, st, tr, ws)
        if hist:
            out["hist"] = hd
        return out

    def _planes(self, y, st, tr, ws) -> dict:
        """The dict of ``forward_traced`` from a traced forward's output, observers, trace buffer and workspace; the planes that
        live in the workspace are copied, the others are views of the trace buffer."""
        B, L = int(y.shape[0]), int(y.shape[1])
        NH, NP2 = B * L * self.H, B * L * 2 * self.P
        out = dict(out=y, stats=st, h_enc=ws[:NH].view(B, L, self.H).clone())
        for i in range(self.n_layers):
            for j, name in enumerate(TRACE_PLANES):
                out[f"l{i}.{name}"] = tr[(5 * i + j) * NH:(5 * i + j + 1) * NH].view(B, L, self.H)
            base = 2 * NH + 2 * i * NP2
            out[f"l{i}.Bu"] = torch.view_as_complex(ws[base:base + NP2].view(B, L, self.P, 2).clone())
            out[f"l{i}.xs"] = torch.view_as_complex(ws[base + NP2:base + 2 * NP2].view(B, L, self.P, 2).clone())
        return out

    def forward_clips_traced(self, x: torch.Tensor, lens: torch.Tensor, fq=None, out: Optional[torch.Tensor] = None,
                             trace_buf: Optional[torch.Tensor] = None) -> dict:
        """``forward_traced`` for n clips of different lengths (``s5fxp_float_model_clips_traced``): x
        (n,Lmax,257) float32 on the device, padded; lens (n,) int32 on the device.  The keys are ``forward_traced``'s and every
        plane is padded like x: rows t < len_e of clip e are bit for bit those of ``forward_traced(x[e:e+1, :len_e], fq=fq)``,
        rows from len_e on are never written and hold whatever the buffers held.  ``out`` / ``trace_buf``
        (``s5fxp_float_trace_bytes`` / 4 float32): the tensors to write into, fresh otherwise.  No histogram.  Stream-ordered,
        no sync."""
        st = self.new_stats() if self.on_device else None
        y, tr, ws = self._device_forward(True, x, lens, st, None, out, True, fq, trace_buf)
        return self._planes(y, st, tr, ws)

    def _to_device(self, x) -> torch.Tensor:
        if isinstance(x, torch.Tensor):
            return x.to(device=self.device, dtype=torch.float32)
        return torch.from_numpy(_f32(x)).to(self.device)

    # -- the mirror of synth.float_forward -----------------------------------------------------
    def forward(self, x, stats: Optional[dict] = None, activations: Optional[dict] = None, hist: Optional[dict] = None,
                fq=None):
        """x (B,L,257) float32, NumPy array or tensor -> the model's output of the same kind.  ``stats`` is updated by maximum
        and ``hist`` by addition (int64[64] rows) under ``synth.float_forward``'s keys; ``activations`` receives sequence 0 under the reference's keys (``pre_C`` = the
        rectified states).  ``fq`` (``fq_spec``) fake-quantises the observed tensors whose site is on; not
        together with ``hist``."""
        fq = self._fq_arg(fq, hist)
        as_tensor = isinstance(x, torch.Tensor)
        if not self.on_device:
            xn = x.detach().cpu().numpy().astype(F32) if as_tensor else np.asarray(x, dtype=F32)
            y = synth.float_forward(self.modeldict, xn, self.n_layers, stats=stats, activations=activations, hist=hist, fq=fq)
            return torch.from_numpy(y) if as_tensor else y
        xd = self._to_device(x)
        hd = None
        if activations is not None:
            t = self.forward_traced(xd, hist=hist is not None, fq=fq)
            y, st, hd = t["out"], t["stats"], t.get("hist")
            self._fill_activations(t, activations)
        else:
            st = self.new_stats() if stats is not None else None
            hd = self.new_hist() if hist is not None else None
            y = self.forward_device(xd, st, hist_dev=hd, fq=fq)
        self._merge(st, hd, stats, hist)
        return y.to(x.device) if as_tensor else y.cpu().numpy()

    def _fill_activations(self, t: dict, activations: dict) -> None:
        from .ssm import complex_relu
        enc = activations.setdefault("encoder", {})
        h = t["h_enc"]
        for i in range(self.n_layers):
            act = enc.setdefault(f"layers_{i}", {})
            _, B_bar, _ = synth.zoh(self.modeldict["encoder"][f"layers_{i}"]["mixer"])
            y, g = t[f"l{i}.y"][0], t[f"l{i}.g"][0]
            n = lambda v: v.cpu().numpy()
            act.update(input=n(h[0]), pre_s5=n(t[f"l{i}.u"][0]), pre_C=n(complex_relu(t[f"l{i}.xs"][0])), pre_GLU=n(y),
                       post_GLU=n(torch.clamp_min(y, 0) * g), __call__=n(t[f"l{i}.h_out"][0]))
            act["mixer"] = dict(B_bar=B_bar.astype(np.complex64), __call__=n(y))
            act["out2"] = dict(__call__=n(t[f"l{i}.g_in"][0]))
            h = t[f"l{i}.h_out"]
        activations["__call__"] = t["out"][0].cpu().numpy()


def _clip_pair(item):
    """(x, lens) when a calibration item is a pair of a padded (n,Lmax,257) batch and its n clip lengths, else None."""
    if isinstance(item, (tuple, list)) and len(item) == 2 and getattr(item[0], "ndim", 0) == 3:
        return item[0], item[1]
    return None


def _real_clips(x, lens) -> list:
    """The host-side reading of an (x, lens) pair: the clips' real frames, x[e, :clamp(lens[e], 0, Lmax)], empty clips dropped."""
    Lmax = int(x.shape[1])
    lens = [min(max(int(v), 0), Lmax) for v in torch.as_tensor(lens).tolist()]
    if len(lens) != int(x.shape[0]):
        raise ValueError(f"{int(x.shape[0])} clips but {len(lens)} lengths")
    return [x[e, :n] for e, n in enumerate(lens) if n]


def _observe(eng: "FloatEngine", item, st, hd, stats: Optional[dict], hist: Optional[dict]) -> None:
    """One calibration item through the engine: a pair takes the clip entry, so that its padding is never observed; a plain
    (B,L,257) batch the rectangular one.  Device arrays ``st`` / ``hd`` on the device, the dicts off it."""
    pair = _clip_pair(item)
    if eng.on_device:
        if pair is None:
            eng.forward_device(eng._to_device(item), st, hist_dev=hd)
        else:
            lens = torch.as_tensor(pair[1]).to(device=eng.device, dtype=torch.int32)
            eng.forward_clips_device(eng._to_device(pair[0]), lens, st, hd)
    elif pair is None:
        eng.forward(item, stats=stats, hist=hist)
    else:
        eng.forward_clips(_real_clips(*pair), stats=stats, hist=hist)


def _derive_qconfig(modeldict: dict, absmax: dict, n_layers: int, quantization: str, state_headroom_bits: int) -> dict:
    """The fixed-point configuration from the observers, as ``synth.make_model`` derives it after its dry run."""
    qc = synth.derive_qconfig(modeldict, absmax, n_layers, synth.PRECISIONS[quantization])
    for k in ("x_re", "x_im"):
        qc["blocks"]["ssm"]["activations"][k]["exp"] -= state_headroom_bits
    synth.cap_result_exponents(qc)
    synth._assert_exps_nonnegative(qc)
    return qc


def calibrate(modeldict: dict, batches: Iterable, n_layers: int, quantization: str = "w8a16",
              state_headroom_bits: int = 0, engine: Optional[FloatEngine] = None) -> Tuple[dict, dict]:
    """Streams ``batches`` (each (B,L,257) float32) through the float model and derives the fixed-point configuration from
    the observers, exactly as ``synth.make_model`` does after its dry run -> (stats, fxp_qconfig).  On a GPU the observers
    stay in one device array across the batches and are read back once.  An item may also be a pair (x, lens) of clips of
    different lengths, x padded to (n,Lmax,257) and lens n integers (tensor, array or list): it takes the clip entry
    (``forward_clips_device``), so no padding frame is observed.  Both kinds may be mixed."""
    eng = engine if engine is not None else FloatEngine(modeldict, n_layers)
    stats: dict = {}
    if eng.on_device:
        st = eng.new_stats()
        for x in batches:
            _observe(eng, x, st, None, None, None)
        stats = eng.stats_dict(st)
    else:
        for x in batches:
            _observe(eng, x, None, None, stats, None)
    if not stats:
        raise ValueError("calibrate needs at least one batch")
    return stats, _derive_qconfig(modeldict, stats, n_layers, quantization, state_headroom_bits)


def clip_absmax(stats: dict, hist: dict, clip_fraction: float, keep=("x_re", "x_im")) -> dict:
    """The observers a calibration that may ignore ``clip_fraction`` of every tensor's values works from.  Per key, with
    n = sum(hist) and T(k) = #{|v| >= 2^k}: k* = min{k in [-39, 23] : T(k) <= floor(clip_fraction * n)}, and the effective
    absmax is min(absmax, nextafter(float32(2^k*), 0)) -- the largest value that still needs only k* integer bits; without
    such a k it is absmax.  Keys whose last component is in ``keep`` pass through: the reference never clips the SSM state,
    it wraps (fxpmodel.py:147-172), so the state's exponent stays on its absmax.  ``clip_fraction`` = 0 changes nothing, by
    construction: T(k) = 0 means absmax < 2^k already."""
    if not 0.0 <= clip_fraction < 1.0:
        raise ValueError(f"clip_fraction must be in [0, 1), got {clip_fraction}")
    out = {}
    for key, absmax in stats.items():
        out[key] = absmax
        if key.split(".")[-1] in keep:
            continue
        row = np.asarray(hist[key], dtype=np.int64)
        allow = int(math.floor(clip_fraction * int(row.sum())))
        tails = np.cumsum(row[::-1])[::-1]  # tails[b] = count in the bins b ..
        for k in range(HIST_KMIN, HIST_KMAX + 1):
            if int(tails[k - HIST_EMIN]) <= allow:
                out[key] = min(absmax, float(np.nextafter(F32(2.0 ** k), F32(0))))
                break
    return out


def calibrate_clipped(modeldict: dict, batches: Iterable, n_layers: int, clip_fraction: float, quantization: str = "w8a16",
                      state_headroom_bits: int = 0, keep=("x_re", "x_im"),
                      engine: Optional[FloatEngine] = None) -> Tuple[dict, dict, dict, dict]:
    """``calibrate`` with the histograms carried next to the observers -> (stats, hist, effective, fxp_qconfig): the
    configuration is derived from ``effective = clip_absmax(stats, hist, clip_fraction, keep)``.  On a GPU both arrays stay
    on the device across the batches and are read back once.  Items may be pairs (x, lens) as in ``calibrate``: the histograms
    then hold no padding, so neither ``range_report``'s denominators nor the allowance floor(clip_fraction * n) grow by it."""
    eng = engine if engine is not None else FloatEngine(modeldict, n_layers)
    stats: dict = {}
    hist: dict = {}
    if eng.on_device:
        st, hd = eng.new_stats(), eng.new_hist()
        n = 0
        for x in batches:
            _observe(eng, x, st, hd, None, None)
            n += 1
        if n:
            stats, hist = eng.stats_dict(st), eng.hist_dict(hd)
    else:
        for x in batches:
            _observe(eng, x, None, None, stats, hist)
    if not stats:
        raise ValueError("calibrate_clipped needs at least one batch")
    effective = clip_absmax(stats, hist, clip_fraction, keep)
    return stats, hist, effective, _derive_qconfig(modeldict, effective, n_layers, quantization, state_headroom_bits)


def quantiser_of(key: str, fxp_qconfig: dict) -> Tuple[int, int]:
    """(bits, exp) of the entry of ``fxp_qconfig`` that quantises the tensor observed under ``key``."""
    parts = key.split(".")
    if parts[0] in ("encoder", "decoder"):
        d = fxp_qconfig[parts[0]]
        return int(d[f"{parts[1]}_bits"]), int(d[f"{parts[1]}_exp"])
    b = fxp_qconfig["blocks"]
    if parts[1] == "out2":
        return int(b["out2"][f"{parts[2]}_bits"]), int(b["out2"][f"{parts[2]}_exp"])
    if parts[1] == "gate":
        return int(b["multgate"][f"{parts[2]}_bits"]), int(b["multgate"][f"{parts[2]}_exp"])
    a = b["ssm"]["activations"][parts[1]]
    return int(a["bits"]), int(a["exp"])


def _site_error(key: str, bits: int, exp: int, mode: int, saturate: int) -> Optional[str]:
    """Why ``s5fxp_float_model_forward_fq`` would refuse this site, or None."""
    if bits == 0:
        return None
    if not FQ_BITS[0] <= bits <= FQ_BITS[1]:
        return f"{key}: bits {bits} outside {FQ_BITS[0]}..{FQ_BITS[1]}"
    if not FQ_EXPS[0] <= exp <= FQ_EXPS[1]:
        return f"{key}: exp {exp} outside {FQ_EXPS[0]}..{FQ_EXPS[1]}"
    if mode not in (0, 1, FQ_STEP):
        return f"{key}: unknown mode {mode}"
    if mode == FQ_STEP and key.split(".")[-1] not in STATE_SITES:
        return f"{key}: step mode is for the state sites {STATE_SITES} only"
    if saturate not in (0, 1) or (saturate and key.split(".")[-1] in STATE_SITES):
        return f"{key}: saturate {saturate} (the state sites never saturate)"
    return None


def fq_spec(fxp_qconfig: dict, n_layers: int, sites=None, mode: str = "floor", recurrence: str = "scan") -> np.ndarray:
    """The fake-quantisation spec of a forward: one ``FQ_SITE`` entry (bits, exp, mode, saturate) per observer, in
    ``stat_keys`` order, (bits, exp) taken from ``quantiser_of``.  ``sites``: the keys to switch on (None: all of them);
    every other entry is zero, i.e. off.  The state sites ``x_re`` / ``x_im`` never saturate, every other site does.
    ``recurrence="step"`` puts every state site that is on into mode ``FQ_STEP``: that layer's recurrence
    rounds at every step (``fq_scan``) in place of quantising the scan's output; both state sites of a layer must then be on.
    ``ValueError`` for an unknown key or mode and for a quantiser the entry would refuse, naming the key."""
    if mode not in FQ_MODES:
        raise ValueError(f"mode must be one of {FQ_MODES}, got {mode!r}")
    if recurrence not in ("scan", "step"):
        raise ValueError(f'recurrence must be "scan" or "step", got {recurrence!r}')
    keys = stat_keys(n_layers)
    on = set(keys) if sites is None else set(sites)
    unknown = sorted(on - set(keys))
    if unknown:
        raise ValueError(f"unknown observer keys {unknown}")
    spec = np.zeros(len(keys), dtype=FQ_SITE)
    for j, key in enumerate(keys):
        if key not in on:
            continue
        bits, exp = quantiser_of(key, fxp_qconfig)
        sat = int(key.split(".")[-1] not in STATE_SITES)
        err = _site_error(key, bits, exp, FQ_MODES.index(mode), sat)
        if err or bits == 0:
            raise ValueError(f"fq_spec: {err or key + ': bits 0'}")
        spec[j] = (bits, exp, FQ_STEP if recurrence == "step" and not sat else FQ_MODES.index(mode), sat)
    err = _step_pair_error(keys, spec)
    if err:
        raise ValueError(f"fq_spec: {err}")
    return spec


def _step_pair_error(keys, fq) -> Optional[str]:
    """Why the entries would refuse the step sites of ``fq`` as a whole, or None: a layer's two state sites step together."""
    step = {k for k, s in zip(keys, fq) if int(s["bits"]) and int(s["mode"]) == FQ_STEP}
    for k in sorted(step):
        other = k[:-2] + ("im" if k.endswith("re") else "re")
        if other not in step:
            return f"{k}: step mode on one state site of a layer only ({other} is not in step mode)"
    return None


def step_layers(fq, n_layers: int) -> List[int]:
    """The layers whose state sites ``fq`` puts into step mode."""
    if fq is None:
        return []
    keys = stat_keys(n_layers)
    return [i for i in range(n_layers) if int(fq[keys.index(f"l{i}.x_re")]["bits"]) and int(fq[keys.index(f"l{i}.x_re")]["mode"]) == FQ_STEP]


def _check_fq(fq, keys) -> Optional[np.ndarray]:
    """``fq`` as the contiguous FQ_SITE array the entries read, checked as they check it (ValueError names the key)."""
    if fq is None:
        return None
    fq = np.ascontiguousarray(fq)
    if fq.dtype != FQ_SITE or fq.shape != (len(keys),):
        raise ValueError(f"fq must be an FQ_SITE array of {len(keys)} entries (fq_spec), got {fq.dtype} {fq.shape}")
    for key, s in zip(keys, fq):
        err = _site_error(key, int(s["bits"]), int(s["exp"]), int(s["mode"]), int(s["saturate"]))
        if err:
            raise ValueError(f"fq: {err}")
    err = _step_pair_error(keys, fq)
    if err:
        raise ValueError(f"fq: {err}")
    return fq


WEIGHT_GROUPS = ("ssm.A", "ssm.B", "ssm.C", "ssm.D", "encoder", "out2", "decoder")


def quantised_modeldict(modeldict: dict, fxp_qconfig: dict, n_layers: int, groups=None) -> dict:
    """``modeldict`` with the chosen weight groups (``WEIGHT_GROUPS``; None: all) replaced by the integer model's dequantised
    values, ``host_from_fp(v, bits, exp) * 2^-exp`` -- the call ``FxpSSM.setup`` / ``FxpDense.setup`` make, on the same float32
    inputs -- as a new modeldict that ``FloatEngine``, ``pack_blob``, ``synth.float_forward``, ``calibrate`` and ``sensitivity``
    accept.  ``ssm.A`` / ``ssm.B`` / ``ssm.C`` are quantised AFTER the ZOH discretisation (the reference's
    complex64 ``discretize_zoh``) and travel in the mixer dict under ``synth.ZOH_KEY``, which ``synth.zoh`` returns in place
    of recomputing; ``encoder``, ``out2`` and ``decoder`` are a dense layer's kernel and bias.  The input is not modified, a
    group left out stays bit-identical, and the BatchNorm constants are never touched (the blob holds 1 / sqrt(var + eps)
    computed by the packer, and the integer BatchNorm's data-dependent exponents are not modelled)."""
    import copy
    from .fxpmodel import discretize_zoh, host_from_fp

    groups = set(WEIGHT_GROUPS if groups is None else groups)
    unknown = sorted(groups - set(WEIGHT_GROUPS))
    if unknown:
        raise ValueError(f"unknown weight groups {unknown}; the groups are {WEIGHT_GROUPS}")
    out = copy.deepcopy(modeldict)

    def deq(v, bits, exp):
        return (host_from_fp(v, int(bits), int(exp)).astype(F32) / F32(2.0 ** int(exp))).astype(F32)

    def dense(d, q):
        d["kernel"] = deq(d["kernel"], q["w_bits"], q["w_exp"])
        d["bias"] = deq(d["bias"], q["b_bits"], q["b_exp"])

    if "encoder" in groups:
        dense(out["encoder"]["encoder"], fxp_qconfig["encoder"])
    if "decoder" in groups:
        dense(out["decoder"], fxp_qconfig["decoder"])
    for i in range(n_layers):
        layer = out["encoder"][f"layers_{i}"]
        blocks = fxp_qconfig["blocks"]
        blocks = blocks.get(f"layers_{i}", blocks)  # separate exponents per layer (FxpSequenceLayer.setup)
        w, md = blocks["ssm"]["weights"], layer["mixer"]
        if "out2" in groups:
            dense(layer["out2"], blocks["out2"])
        if "ssm.D" in groups:
            md["D"] = deq(md["D"], w["D"]["bits"], w["D"]["exp"])
        if groups & {"ssm.A", "ssm.B", "ssm.C"}:
            step = np.exp(np.asarray(md["log_step"], dtype=F32)[:, 0]).astype(F32)  # FxpSSM.setup at step_rescale 1
            lam_bar, B_bar = discretize_zoh(md["Lambda_re"] + 1j * md["Lambda_im"], md["B"][..., 0] + 1j * md["B"][..., 1], step)
            Cc = (md["C"][..., 0] + 1j * md["C"][..., 1]).astype(np.complex64)
            hook = dict(md.get(synth.ZOH_KEY, {}))
            for g, key, v, k in (("ssm.A", "lam_bar", lam_bar, "A"), ("ssm.B", "B_bar", B_bar, "B"), ("ssm.C", "C", Cc, "C")):
                if g in groups:
                    hook[key] = np.empty(v.shape, dtype=np.complex64)
                    hook[key].real = deq(v.real, w[f"{k}_re"]["bits"], w[f"{k}_re"]["exp"])
                    hook[key].imag = deq(v.imag, w[f"{k}_im"]["bits"], w[f"{k}_im"]["exp"])
            md[synth.ZOH_KEY] = hook
    return out


def _real_frames(eng: "FloatEngine", item, fq, st=None) -> torch.Tensor:
    """The model's output on the real frames of one calibration item, flat float64, on the engine's device.  ``st``: the
    observers to raise -- a device array (``new_stats``) when the engine is on the device, a dict otherwise."""
    pair = _clip_pair(item)
    if pair is None:
        if eng.on_device:
            return eng.forward_device(eng._to_device(item), st, fq=fq).double().flatten()
        xn = item.detach().cpu().numpy() if isinstance(item, torch.Tensor) else item
        return torch.from_numpy(eng.forward(np.asarray(xn, dtype=F32), stats=st, fq=fq)).double().flatten()
    if eng.on_device:
        Lmax = int(pair[0].shape[1])
        lens = torch.as_tensor(pair[1]).to(device=eng.device, dtype=torch.int32)
        y = eng.forward_clips_device(eng._to_device(pair[0]), lens, st, fq=fq)
        real = torch.arange(Lmax, device=eng.device)[None, :] < lens.clamp(0, Lmax)[:, None]
        return y[real].double().flatten()  # y's padding is unspecified: select, do not multiply
    ys = eng.forward_clips(_real_clips(*pair), stats=st, fq=fq)
    return torch.cat([torch.as_tensor(y).double().flatten() for y in ys]) if ys else torch.zeros(0, dtype=torch.float64)


def sensitivity(modeldict: dict, batches: Iterable, fxp_qconfig: dict, n_layers: int, groups=None, mode: str = "floor",
                engine: Optional[FloatEngine] = None, recurrence: str = "scan", weights: Optional[dict] = None) -> Dict[str, float]:
    """Which quantiser costs the accuracy: the output SQNR of the float model with one group of sites fake-quantised at a
    time -> {group: sqnr_db} plus ``"all"`` (every group on at once).  ``groups`` maps a name to the observer keys it
    switches on; the default is one group per key.  ``batches`` as for ``calibrate``: (B,L,257) batches, or pairs (x, lens)
    that take the clip entry, of which only the real frames count.  Per batch one plain forward, one forward per group and
    one with all groups run on the same input; sqnr_db = 10 log10(sum y^2 / sum (y_fq - y)^2), both sums accumulated in
    float64 over all batches (on the device when the engine is); a zero difference gives inf.

    The two things the sites alone do not hold.  ``recurrence="step"`` adds the row ``"recurrence"``: the
    state sites of every layer alone, in step mode, so the rounding inside the integer recurrence is fed back through the
    pole.  ``weights=fxp_qconfig`` adds one row per weight group (``WEIGHT_GROUPS``): the plain activations on
    ``quantised_modeldict(modeldict, weights, n_layers, [group])``, one more engine each.  ``"all"`` is then every site of
    ``groups``, in step mode when asked for, on the model with all weight groups quantised; every row is measured against
    the plain forward of ``modeldict``.  A step-mode run whose ``x_re`` / ``x_im`` observers show that it left the domain of
    ``fq_scan`` (|x| * 2^exp >= 2^24) is named in the list under ``"left_domain"``, a key that is absent otherwise."""
    eng = engine if engine is not None else FloatEngine(modeldict, n_layers)
    keys = stat_keys(n_layers)
    groups = {k: [k] for k in keys} if groups is None else {str(g): list(ks) for g, ks in dict(groups).items()}
    reserved = {"all", "left_domain"} | ({"recurrence"} if recurrence == "step" else set()) | (set(WEIGHT_GROUPS) if weights else set())
    if reserved & set(groups):
        raise ValueError(f"{sorted(reserved & set(groups))} name rows of the result; call a group something else")
    if recurrence not in ("scan", "step"):
        raise ValueError(f'recurrence must be "scan" or "step", got {recurrence!r}')
    states = [f"l{i}.{k}" for i in range(n_layers) for k in STATE_SITES]
    runs = {g: (eng, fq_spec(fxp_qconfig, n_layers, ks, mode)) for g, ks in groups.items()}  # row -> (engine, spec)
    if recurrence == "step":
        runs["recurrence"] = (eng, fq_spec(fxp_qconfig, n_layers, states, mode, recurrence="step"))
    all_keys = [k for ks in groups.values() for k in ks]
    all_eng = eng
    if weights is not None:
        for g in WEIGHT_GROUPS:
            runs[g] = (FloatEngine(quantised_modeldict(modeldict, weights, n_layers, [g]), n_layers), None)
        all_eng = FloatEngine(quantised_modeldict(modeldict, weights, n_layers), n_layers)
    if recurrence == "step" and set(states) <= set(all_keys):
        runs["all"] = (all_eng, fq_spec(fxp_qconfig, n_layers, all_keys, mode, recurrence="step"))
    elif recurrence == "step":  # the groups leave state sites out: "all" holds the groups and the stepping recurrence
        spec = fq_spec(fxp_qconfig, n_layers, all_keys, mode)
        step = runs["recurrence"][1]
        for j, k in enumerate(keys):
            if k in states:
                spec[j] = step[j]
        runs["all"] = (all_eng, spec)
    else:
        runs["all"] = (all_eng, fq_spec(fxp_qconfig, n_layers, all_keys, mode))
    stepping = {g: (e.new_stats() if e.on_device else {}) for g, (e, spec) in runs.items() if step_layers(spec, n_layers)}
    num, den, n = None, {}, 0
    for item in batches:
        y = _real_frames(eng, item, None)
        e = (y * y).sum()
        num = e if num is None else num + e
        for g, (run_eng, spec) in runs.items():
            d = _real_frames(run_eng, item, spec, stepping.get(g)).to(y.device) - y
            e = (d * d).sum()
            den[g] = e if g not in den else den[g] + e
        n += 1
    if not n:
        raise ValueError("sensitivity needs at least one batch")
    num = float(num)
    out = {}
    for g in runs:
        d = float(den[g])
        out[g] = math.inf if d == 0.0 else 10.0 * math.log10(num / d) if num > 0.0 else -math.inf
    left = []
    for g, st in stepping.items():
        seen = runs[g][0].stats_dict(st) if isinstance(st, torch.Tensor) else st
        spec = runs[g][1]
        if any(seen.get(k, 0.0) * 2.0 ** int(spec[keys.index(k)]["exp"]) >= FQ_STEP_XMAX for k in states if int(spec[keys.index(k)]["bits"])):
            left.append(g)
    if left:
        out["left_domain"] = left
    return out


def range_report(hist: dict, fxp_qconfig: dict, n_layers: int) -> Dict[str, dict]:
    """Per observed tensor, what its quantiser (``quantiser_of``: bits, exp) does to the calibration set:
    ``total`` values seen, ``saturates`` = T(bits - 1 - exp) / total, the share with |v| >= 2^(bits - 1 - exp), and
    ``below_lsb`` = 1 - T(-exp) / total, the share with |v| < 2^-exp.  Exact but for one case: a value equal to
    -2^(bits - 1 - exp) is representable and is counted as saturating.  ``ValueError`` for a threshold outside 2^-39 .. 2^23."""
    out = {}
    for key in stat_keys(n_layers):
        bits, exp = quantiser_of(key, fxp_qconfig)
        row = np.asarray(hist[key], dtype=np.int64)
        total = int(row.sum())
        sat, lsb = tail_count(row, bits - 1 - exp), tail_count(row, -exp)
        out[key] = dict(total=total, saturates=sat / total if total else 0.0, below_lsb=1.0 - lsb / total if total else 0.0)
    return out
