"""Fused forward of the fixed-point S5 model: Python driver of ``s5fxp_model_forward`` (int32 in and out),
``s5fxp_model_forward_f32`` (float32 in and out, the reference's validation step, sparseRNNs/fxprun.py:63-88) and
``s5fxp_model_forward_i16`` (int16 in and out: the same integers in half the bytes).

``Engine`` takes the INTEGER model in the reference's ``export()`` layout
(sparseRNNs/fxpmodel.py:1441-1458 and the nested exports it gathers), hands it to the C ABI,
and owns the device buffers (parameter blob, workspace, status words) as torch tensors.
The forward itself is a sequence of HIP kernel launches on the current stream with no host
synchronisation inside; data-dependent exponents stay in device memory.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import (DenseDesc, LayerDesc, LayerTrace, ModelDesc, NormDesc, SSMDesc, TRACE_FIELDS, check, lib)
from .fxparray import FxpArray

I32P = _lib.I32P


class Engine:
    def __init__(self, export: dict, flags: int = 0, device: Optional[torch.device] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("sparsernns_amd.Engine needs a ROCm GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self._keep: list = []
        self._export, self._flags, self._generic = export, flags, None
        P, Q = export["params"], export["qconfig"]
        self.n_layers = len([k for k in P["encoder"] if k.startswith("layers_")])
        self._layers = (LayerDesc * max(self.n_layers, 1))()
        for i in range(self.n_layers):
            self._fill_layer(self._layers[i], P["encoder"][f"layers_{i}"], Q["encoder"][f"layers_{i}"])
        self._desc = ModelDesc()
        self._desc.n_layers = self.n_layers
        self._desc.encoder = self._dense(P["encoder"]["encoder"], Q["encoder"]["encoder"])
        self._desc.layers = C.cast(self._layers, C.POINTER(LayerDesc))
        self._desc.decoder = self._dense(P["decoder"], Q["decoder"])
        self.d_in, self.H = self._desc.encoder.K, self._desc.encoder.M
        self.P = self._layers[0].ssm.P if self.n_layers else 0
        self.d_out = self._desc.decoder.M
        self.inp_bits, self.inp_exp = self._desc.encoder.inp_bits, self._desc.encoder.inp_exp
        nbytes = lib.s5fxp_model_blob_bytes(C.byref(self._desc))
        if nbytes == 0:
            # let create() report the precise reason
            nbytes = 256
        with torch.cuda.device(self.device):
            self.blob = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            handle = C.c_void_p()
            check(lib.s5fxp_model_create(C.byref(self._desc), self.blob.data_ptr(), nbytes, flags,
                                         torch.cuda.current_stream().cuda_stream, C.byref(handle)), "s5fxp_model_create")
        self._h = handle
        self.out_bits, self.out_exp = lib.s5fxp_model_out_bits(self._h), lib.s5fxp_model_out_exp(self._h)
        # a lane = the per-forward mutable state (status words + workspace); forwards on different lanes may be
        # in flight at the same time on different streams (InflightRunner).  Lane 0 is the default.
        self._status = {0: torch.zeros(_lib.STATUS_WORDS, dtype=torch.int32, device=self.device)}
        # The ladder of recurrence kernels an optimistic forward climbs when ST_REDO comes back: 0 pair kernel (tightest bound
        # on |state|), 1 quad kernel with int16 streams (16 bits), 2 exact 32-bit kernels.  `level` is where forwards start;
        # a rung that failed twice is not tried again for this model.
        self.level = 0
        self._redos = [0, 0]
        self._wsl: Dict[int, tuple] = {}
        self._groups: Dict[int, int] = {}   # groups of the last forward enqueued on a lane
        self._cb_keep = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib.s5fxp_model_destroy(h)
            self._h = None

    # -- descriptor construction ---------------------------------------------------------------
    def _ptr(self, a) -> I32P:
        arr = np.ascontiguousarray(np.asarray(a).astype(np.int64).astype(np.int32))
        self._keep.append(arr)
        return arr.ctypes.data_as(I32P)

    def _dense(self, p: dict, q: dict) -> DenseDesc:
        d = DenseDesc()
        d.K, d.M = p["weight"].shape
        d.weight, d.bias = self._ptr(p["weight"]), self._ptr(p["bias"])
        d.w_bits, d.w_exp = int(q["weight_bits"]), int(q["weight_exp"])
        d.b_bits, d.b_exp = int(q["bias_bits"]), int(q["bias_exp"])
        d.inp_bits, d.inp_exp = int(q["inp_bits"]), int(q["inp_exp"])
        d.out_bits, d.out_exp = int(q["out_bits"]), int(q["out_exp"])
        return d

    def _fill_layer(self, L: LayerDesc, lp: dict, lq: dict) -> None:
        L.out2 = self._dense(lp["out2"], lq["out2"])
        m, mq = lp["mixer"], lq["mixer"]
        s: SSMDesc = L.ssm
        s.P, s.H = m["B_real"].shape
        for f, k in (("A_re", "A_real"), ("A_im", "A_imag"), ("B_re", "B_real"), ("B_im", "B_imag"),
                     ("C_re", "C_real"), ("C_im", "C_imag"), ("D", "D")):
            setattr(s, f, self._ptr(m[k]))
            setattr(s, f + "_bits", int(mq[f"{k}_bits"]))
            setattr(s, f + "_exp", int(mq[f"{k}_exp"]))
        for k in ("u", "Bu_re", "Bu_im", "x_re", "x_im", "y"):
            setattr(s, k + "_bits", int(mq[f"{k}_bits"]))
            setattr(s, k + "_exp", int(mq[f"{k}_exp"]))
        n, nq = lp["norm"], lq["norm"]
        bn: NormDesc = L.norm
        bn.minus_mean = self._ptr(-np.asarray(n["mean"], dtype=np.int64))  # export() stores +mean (:949)
        bn.invsq_var = self._ptr(n["invsq_var"])
        bn.mean_bits, bn.mean_exp = int(nq["mean_bits"]), int(nq["mean_exp"])
        bn.invsq_var_bits, bn.invsq_var_exp = int(nq["invsq_var_bits"]), int(nq["invsq_var_exp"])
        if "scale" in n:
            bn.scale, bn.scale_bits, bn.scale_exp = self._ptr(n["scale"]), int(nq["scale_bits"]), int(nq["scale_exp"])
        if "bias" in n:
            bn.bias, bn.bias_bits, bn.bias_exp = self._ptr(n["bias"]), int(nq["bias_bits"]), int(nq["bias_exp"])
        for k in ("l_bits", "l_exp", "r_bits", "r_exp", "res_bits", "res_exp"):
            setattr(L, k, int(lq["multgate"][k]))
        sg = lq["sigmoid"]
        if int(sg.get("x_extra", 3)) != 3 or int(sg.get("n_exp", 3)) != 3:
            raise NotImplementedError("only the reference's 8-entry sigmoid LUT is implemented")
        L.sig_x_exp, L.sig_y_exp = int(sg["x_exp"]), int(sg["y_exp"])
        from .fxpmodel import sigmoid_lut
        lut = sigmoid_lut(L.sig_x_exp, L.sig_y_exp)
        for j in range(8):
            L.lut[j] = int(lut[j])

    # -- forward ---------------------------------------------------------------------------------
    LEVEL_FLAGS = (_lib.FWD_DEFER_REDO, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, _lib.FWD_EXACT)

    @property
    def redo_seen(self) -> int:  # kept for callers of the two-rung form: 2 = "go straight to the exact kernels"
        return 2 if self.level >= 2 else 0

    @redo_seen.setter
    def redo_seen(self, v: int) -> None:
        if v >= 2:
            self.level = 2

    def note_redo(self, level: int) -> int:
        """An optimistic forward at `level` came back with ST_REDO: returns the rung to repeat it on."""
        if level < 2:
            self._redos[level] += 1
            if self._redos[level] >= 2 and self.level <= level:
                self.level = level + 1
        return min(level + 1, 2)

    def run_ladder(self, launch: Callable[[int], None], check: Callable[[], np.ndarray]) -> None:
        """launch(flags) enqueues the forward, check() returns the status words (after synchronising)."""
        level = self.level
        while True:
            launch(self.LEVEL_FLAGS[level])
            st = check()
            if not (st[0] & _lib.ST_REDO) or level >= 2:
                return
            level = self.note_redo(level)

    @property
    def status(self) -> torch.Tensor:
        return self._status[0]

    def lane_status(self, lane: int, groups: int = 1) -> torch.Tensor:
        """The status words of `lane`: STATUS_WORDS per group, group after group (a plain forward is one group)."""
        st = self._status.get(lane)
        if st is None or st.numel() < groups * _lib.STATUS_WORDS:
            st = self._status[lane] = torch.zeros(groups * _lib.STATUS_WORDS, dtype=torch.int32, device=self.device)
        return st

    # the three model boundaries: dtype of x and y -> (workspace query, forward entry, its name)
    _IO = {torch.int32: (lib.s5fxp_workspace_bytes, lib.s5fxp_model_forward, "s5fxp_model_forward"),
           torch.float32: (lib.s5fxp_workspace_bytes_f32, lib.s5fxp_model_forward_f32, "s5fxp_model_forward_f32"),
           torch.int16: (lib.s5fxp_workspace_bytes_i16, lib.s5fxp_model_forward_i16, "s5fxp_model_forward_i16")}
    # ... and their forms at stated exponents (``enqueue(..., exps=)``)
    _IO_AT = {torch.int32: (lib.s5fxp_model_forward_at, "s5fxp_model_forward_at"),
              torch.float32: (lib.s5fxp_model_forward_at_f32, "s5fxp_model_forward_at_f32"),
              torch.int16: (lib.s5fxp_model_forward_at_i16, "s5fxp_model_forward_at_i16")}

    def workspace(self, B: int, L: int, lane: int = 0, groups: int = 1, io: torch.dtype = torch.int32) -> torch.Tensor:
        """The lane's workspace for forwards of this shape and I/O type (`io`: torch.int32, float32 or int16)."""
        key, ws = self._wsl.get(lane, (None, None))
        if key != (B, L, groups, io):
            per = self._IO[io][0](self._h, B, L)
            ws = torch.empty(groups * per, dtype=torch.uint8, device=self.device)
            self._wsl[lane] = ((B, L, groups, io), ws)
        return ws

    def enqueue(self, x: torch.Tensor, x_bits: int, x_exp: int, y: torch.Tensor, B: int, L: int,
                traces: Optional[List[Dict[str, torch.Tensor]]] = None, allreduce: Optional[Callable] = None,
                scan_events: Optional[list] = None, flags: int = 0, lane: int = 0,
                state_in: Optional[torch.Tensor] = None, state_out: Optional[torch.Tensor] = None, groups: int = 1,
                gate_events: Optional[list] = None, exps=None) -> None:
        """Launches one forward on the current stream; nothing is synchronised.

        exps: an (n_layers, 5) array of stated exponents (``exp_max`` has the layout, ``calibrate_exps`` makes one from data)
        runs ``s5fxp_model_forward_at[_f32|_i16]``: every sequence gets the rows ``clips(..., exps=)`` gives it alone, and with
        state_in / state_out a signal cut into several calls gives the rows of one call.  No traces; `allreduce` is never
        called.  None: the forward as it always was.

        groups = G > 1: x and y hold G * B sequences, G independent reference batches of B sequences each (what G calls
        would compute: own exponents, status words and carry per group) enqueued as ONE set of kernel launches
        (include/s5fxp.h, s5fxp_forward_opts::groups).

        flags: _lib.FWD_DEFER_REDO drops the (normally idle) gated exact re-run launches -- the caller must then
        read the status words and repeat with _lib.FWD_EXACT when ST_REDO is set (``forward`` does).

        x and y are both int32 (``s5fxp_model_forward``) or both float32 (``s5fxp_model_forward_f32``: x_bits / x_exp are then
        the quantisation target of the float input, and y receives to_float of the output) or both int16
        (``s5fxp_model_forward_i16``: the int forward on the sign-extended x, y narrowed; x_bits <= 16 and a model whose
        output has at most 16 bits).  int16 tensors need no more than their own 2-byte alignment: views into larger buffers
        are fine as long as they are contiguous."""
        if x.dtype != y.dtype or x.dtype not in self._IO:
            raise ValueError(f"x and y must both be int32, both float32 or both int16, got {x.dtype} and {y.dtype}")
        io = x.dtype
        if exps is not None and traces is not None:
            raise NotImplementedError("a forward at stated exponents takes no traces")
        if groups > 1 and (traces is not None or allreduce is not None):
            raise ValueError("a grouped forward takes neither traces nor a cross-rank hook: run the groups one by one")
        ws = self.workspace(B, L, lane, groups, io)
        self._groups[lane] = groups
        tr = None
        if traces is not None:
            tr = (LayerTrace * self.n_layers)()
            for i, d in enumerate(traces):
                for k in TRACE_FIELDS:
                    if k in d:
                        setattr(tr[i], k, d[k].data_ptr())
        opts = _lib.ForwardOpts()
        if allreduce is not None:
            ws_base = ws.data_ptr()

            def _cb(ctx, dev_ptr, n, stream):  # noqa: ANN001
                try:
                    # the maxima live in the workspace: hand the hook a float32 view of exactly those n words
                    off = int(dev_ptr) - ws_base
                    allreduce(ws[off:off + 4 * int(n)].view(torch.float32))
                    return 0
                except Exception:  # pragma: no cover - surfaced as EHIP by the C side
                    import traceback
                    traceback.print_exc()
                    return 1
            opts.allreduce = _lib.ALLREDUCE_FN(_cb)
        if scan_events is not None:
            assert len(scan_events) == 2 * self.n_layers
            arr = (C.c_void_p * len(scan_events))(*[(e.cuda_event if e is not None else None) for e in scan_events])
            opts.scan_events = C.cast(arr, C.POINTER(C.c_void_p))
            self._ev_keep = arr
        if gate_events is not None:
            assert len(gate_events) == 2 * self.n_layers
            arr2 = (C.c_void_p * len(gate_events))(*[(e.cuda_event if e is not None else None) for e in gate_events])
            opts.gate_events = C.cast(arr2, C.POINTER(C.c_void_p))
            self._ev_keep2 = arr2
        opts.flags = int(flags)
        opts.groups = int(groups)
        want = (self.n_layers, 2, B, self.P) if groups == 1 else (groups, self.n_layers, 2, B, self.P)
        for name, t in (("state_in", state_in), ("state_out", state_out)):
            if t is not None:
                if t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous() or not t.is_cuda:
                    raise ValueError(f"{name} must be a contiguous int32 device tensor of shape {want}")
                setattr(opts, name, t.data_ptr())
        self._cb_keep = opts
        _, entry, name = self._IO[io]
        tail = ()
        if exps is not None:
            self.check_exps(exps)        # host only: ValueError / NotImplementedError, as the pool and the clip route raise them
            entry, name = self._IO_AT[io]
            eh = self._exps_host(exps)   # the entry reads the host array before it returns: kept alive until then
            tail = (eh.ctypes.data,)
        check(entry(self._h, x.data_ptr(), x_bits, x_exp, B, L, y.data_ptr(), ws.data_ptr(), ws.numel(),
                    self.lane_status(lane, groups).data_ptr(), C.cast(tr, C.POINTER(LayerTrace)) if tr is not None else None,
                    C.byref(opts), *tail, torch.cuda.current_stream().cuda_stream), name)

    def check_status(self, lane: int = 0) -> np.ndarray:
        """Reads the status words back (one sync) and raises what the reference would have raised.  After a grouped
        forward word [0] of the returned array carries the error bits of ALL groups (the per-group words follow at
        multiples of STATUS_WORDS)."""
        groups = self._groups.get(lane, 1)
        # sliced on the device: a lane that once served a launch of many clips keeps its longer tensor
        st = self.lane_status(lane, groups)[:groups * _lib.STATUS_WORDS].cpu().numpy().copy()
        for g in range(1, groups):
            st[0] |= st[g * _lib.STATUS_WORDS]
        if st[0] & _lib.ST_NEGSHIFT:
            raise ValueError("invalid result_exp: a data-dependent shift came out negative (fxparray.py:619-621)")
        if st[0] & _lib.ST_NEGEXP:
            raise ValueError("a compute_best exponent came out negative")
        if st[0] & _lib.ST_WIDE_INPUT:
            raise OverflowError("input FxpArray holds values beyond 24 bits; rebuild the engine with "
                                "flags=MODEL_FORCE_GENERIC")
        return st

    def layer_exponents(self) -> List[Dict[str, int]]:
        st = self.status.cpu().numpy()
        names = ("norm_input_minus_mean", "norm_output_raw", "norm_output_scaled", "norm_output_scaled_bias", "residadd")
        return [{n: int(st[8 + 8 * i + j]) for j, n in enumerate(names)} for i in range(self.n_layers)]

    # -- the three model boundaries: one runner per family, the public methods prepare x and wrap y -----------------------
    def _boundary_input(self, x, dtype: torch.dtype, x_bits: Optional[int], x_exp: Optional[int]):
        """x as a contiguous `dtype` tensor on the engine's device; x_bits / x_exp default to the encoder's input configuration."""
        data = torch.as_tensor(x)
        if data.dtype != dtype:
            name = str(dtype).split(".")[-1]
            raise ValueError(f"expected a{'n' if name[0] == 'i' else ''} {name} tensor, got {data.dtype}")
        return (data.to(self.device).contiguous(), self.inp_bits if x_bits is None else int(x_bits),
                self.inp_exp if x_exp is None else int(x_exp))

    def _rows(self, data: torch.Tensor):
        """(B, L) of x (B,L,d_in) or (L,d_in)."""
        if data.shape[-1] != self.d_in:
            raise ValueError(f"expected last dim {self.d_in}, got {tuple(data.shape)}")
        return (1, data.shape[0]) if data.ndim == 2 else (data.shape[0], data.shape[1])

    def _trace_planes(self, data: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The trace tensors of one layer for the rows of `data`."""
        return {k: torch.empty(tuple(data.shape[:-1]) + (self.P if k in ("Bu_re", "Bu_im", "xs_re", "xs_im") else self.H,),
                               dtype=torch.int32, device=data.device) for k in TRACE_FIELDS}

    def _forward(self, data: torch.Tensor, xb: int, xe: int, out_dtype: torch.dtype, traces: bool, allreduce: Optional[Callable],
                 check_status: bool, exps=None):
        """Returns (y, the traces or None); an empty input gives an empty y without touching the device."""
        B, L = self._rows(data)
        y = torch.empty(tuple(data.shape[:-1]) + (self.d_out,), dtype=out_dtype, device=data.device)
        if B * L == 0:
            return y, ([] if traces else None)
        tr = [self._trace_planes(data) for _ in range(self.n_layers)] if traces else None
        if not check_status or allreduce:
            # self-contained: the gated exact re-run is part of the one enqueue (never the ladder with a multi-rank hook: ranks
            # must enqueue the same work)
            self.enqueue(data, xb, xe, y, B, L, tr, allreduce, exps=exps)
            if check_status:
                self.check_status()
        else:
            # the status words are read anyway: run optimistically and repeat with the exact kernels if a state left the fast
            # recurrence's range
            self.run_ladder(lambda fl: self.enqueue(data, xb, xe, y, B, L, tr, flags=fl, exps=exps), self.check_status)
        return y, tr

    def _forward_batches(self, data: torch.Tensor, xb: int, xe: int, out_dtype: torch.dtype, batch: int, exps=None) -> torch.Tensor:
        if data.ndim != 3 or data.shape[-1] != self.d_in or data.shape[0] % batch:
            raise ValueError(f"expected (G * {batch}, L, {self.d_in}), got {tuple(data.shape)}")
        G, L = data.shape[0] // batch, data.shape[1]
        y = torch.empty(tuple(data.shape[:-1]) + (self.d_out,), dtype=out_dtype, device=data.device)
        if G * batch * L:
            self.run_ladder(lambda fl: self.enqueue(data, xb, xe, y, batch, L, flags=fl, groups=G, exps=exps), self.check_status)
        return y

    def _forward_chunk(self, data: torch.Tensor, xb: int, xe: int, out_dtype: torch.dtype, state: Optional[torch.Tensor], exps=None):
        B, L = self._rows(data)
        if B * L == 0:
            raise ValueError("empty chunk")
        y = torch.empty(tuple(data.shape[:-1]) + (self.d_out,), dtype=out_dtype, device=data.device)
        new_state = torch.empty((self.n_layers, 2, B, self.P), dtype=torch.int32, device=data.device)
        # `state` is never written: a chunk that comes back with ST_REDO is repeated from it on the next rung
        self.run_ladder(lambda fl: self.enqueue(data, xb, xe, y, B, L, flags=fl, state_in=state, state_out=new_state, exps=exps),
                        self.check_status)
        return y, new_state

    def _fxp(self, y: torch.Tensor) -> FxpArray:
        return FxpArray(y, self.out_bits, self.out_exp, True)

    def forward(self, x: FxpArray, traces: bool = False, allreduce: Optional[Callable] = None, check_status: bool = True, exps=None):
        """x: FxpArray (B,L,d_in) or (L,d_in).  Returns an FxpArray (and the traces when asked).  exps: stated exponents
        (``enqueue``) -- here and in every ``forward_*`` method below; None is the forward on its own exponents."""
        y, tr = self._forward(x.data.contiguous(), x.bits, x.exp, torch.int32, traces, allreduce, check_status, exps)
        return (self._fxp(y), tr) if traces else self._fxp(y)

    def forward_float(self, x: torch.Tensor, x_bits: Optional[int] = None, x_exp: Optional[int] = None,
                      check_status: bool = True, allreduce: Optional[Callable] = None, exps=None) -> torch.Tensor:
        """The reference's validation step (sparseRNNs/fxprun.py:63-88) in one call: x float32 (B,L,d_in) or (L,d_in) ->
        float32 (.., d_out), bit for bit ``forward(fxp_from_fp(x, x_bits, x_exp, FLOOR)).to_float()``.  x_bits / x_exp default
        to the encoder's input configuration.  The conversions run inside the encoder and decoder kernels on the fused path.
        check_status / allreduce as in ``forward``."""
        return self._forward(*self._boundary_input(x, torch.float32, x_bits, x_exp), torch.float32, False, allreduce, check_status, exps)[0]

    def forward_batches_float(self, x: torch.Tensor, batch: int, x_bits: Optional[int] = None,
                              x_exp: Optional[int] = None, exps=None) -> torch.Tensor:
        """``forward_batches`` float32 in and out: x (G * batch, L, d_in) -> (G * batch, L, d_out), one set of launches."""
        return self._forward_batches(*self._boundary_input(x, torch.float32, x_bits, x_exp), torch.float32, batch, exps)

    def forward_chunk_float(self, x: torch.Tensor, state: Optional[torch.Tensor] = None, x_bits: Optional[int] = None,
                            x_exp: Optional[int] = None, exps=None):
        """``forward_chunk`` float32 in and out: returns (y float32, new_state); `state` is not modified."""
        return self._forward_chunk(*self._boundary_input(x, torch.float32, x_bits, x_exp), torch.float32, state, exps)

    # -- int16 in, int16 out ----------------------------------------------------------------------
    def forward_int16(self, x, x_bits: Optional[int] = None, x_exp: Optional[int] = None, check_status: bool = True,
                      allreduce: Optional[Callable] = None, exps=None) -> torch.Tensor:
        """``forward`` with int16 tensors at the model boundary: x int16 (B,L,d_in) or (L,d_in) at (x_bits, x_exp) -- default: the
        encoder's input configuration -- -> int16 (.., d_out) at (out_bits, out_exp), the very integers ``forward`` returns
        for the same values as int32.  On the fused path the encoder reads and the decoder writes int16; a model whose output
        is wider than 16 bits raises NotImplementedError.  check_status / allreduce as in ``forward``."""
        return self._forward(*self._boundary_input(x, torch.int16, x_bits, x_exp), torch.int16, False, allreduce, check_status, exps)[0]

    def forward_batches_int16(self, x, batch: int, x_bits: Optional[int] = None, x_exp: Optional[int] = None, exps=None) -> torch.Tensor:
        """``forward_batches`` int16 in and out: x (G * batch, L, d_in) -> (G * batch, L, d_out), one set of launches."""
        return self._forward_batches(*self._boundary_input(x, torch.int16, x_bits, x_exp), torch.int16, batch, exps)

    def forward_chunk_int16(self, x, state: Optional[torch.Tensor] = None, x_bits: Optional[int] = None,
                            x_exp: Optional[int] = None, exps=None):
        """``forward_chunk`` int16 in and out: returns (y int16, new_state); `state` is not modified."""
        return self._forward_chunk(*self._boundary_input(x, torch.int16, x_bits, x_exp), torch.int16, state, exps)

    def layer_forward(self, layer: int, x: FxpArray, traces: bool = False):
        """One ``FxpSequenceLayer.forward`` (sparseRNNs/fxpmodel.py:1110-1161) through ``s5fxp_layer_forward``: x is the
        layer's input (B,L,H) or (L,H) with its own bits / exponent; returns the layer's output FxpArray (its exponent is the
        one the residual compute_best add chose on the device), and the layer's traces when asked."""
        data = x.data.contiguous()
        if data.shape[-1] != self.H:
            raise ValueError(f"expected last dim {self.H}, got {tuple(data.shape)}")
        B, L = (1, data.shape[0]) if data.ndim == 2 else (data.shape[0], data.shape[1])
        y = torch.empty_like(data)
        ws = self.workspace(B, L)
        self._groups[0] = 1
        tr, d = None, None
        if traces:
            tr, d = (LayerTrace * 1)(), self._trace_planes(data)
            for k in TRACE_FIELDS:
                setattr(tr[0], k, d[k].data_ptr())
        e = torch.zeros(1, dtype=torch.int32, device=data.device)
        check(lib.s5fxp_layer_forward(self._h, layer, data.data_ptr(), x.bits, x.exp, B, L, y.data_ptr(), e.data_ptr(), ws.data_ptr(),
                                      ws.numel(), self.lane_status(0).data_ptr(),
                                      C.cast(tr, C.POINTER(LayerTrace)) if tr is not None else None, None,
                                      torch.cuda.current_stream().cuda_stream), "s5fxp_layer_forward")
        self.check_status()
        out = FxpArray(y, lib.s5fxp_model_layer_out_bits(self._h, layer), int(e.item()), True)
        return (out, d) if traces else out

    def forward_batches(self, x: FxpArray, batch: int, exps=None) -> FxpArray:
        """x: (G * batch, L, d_in) -- G independent reference batches of `batch` sequences each (the reference's
        run_validation loop over a loader, sparseRNNs/fxprun.py:53-88, several batches per call).  Returns what G calls of
        ``forward`` would, as one (G * batch, L, d_out) FxpArray, from ONE set of kernel launches."""
        return self._fxp(self._forward_batches(x.data.contiguous(), x.bits, x.exp, torch.int32, batch, exps))

    # -- streaming ------------------------------------------------------------------------------
    def zero_state(self, B: int) -> torch.Tensor:
        """The carry a sequence starts with: (n_layers, 2, B, P) int32 zeros (re plane, im plane per layer)."""
        return torch.zeros((self.n_layers, 2, B, self.P), dtype=torch.int32, device=self.device)

    def forward_chunk(self, x: FxpArray, state: Optional[torch.Tensor] = None, exps=None):
        """One chunk of a stream: x (B,L,d_in) or (L,d_in); `state` from zero_state() or the previous call (None: zeros).
        Returns (y, new_state).  What comes out is what the reference computes for THIS chunk when its recurrences
        (sparseRNNs/fxpmodel.py:147-172, the carry is an explicit argument of the step function) start from `state`;
        every chunk is its own compute_best batch -- or, with `exps`, runs at those stated exponents, and then the chunks of a
        signal give the rows of one forward of the whole signal however it is cut.  `state` is not modified."""
        y, new_state = self._forward_chunk(x.data.contiguous(), x.bits, x.exp, torch.int32, state, exps)
        return self._fxp(y), new_state

    def stream(self, B: int = 1) -> "StreamingSession":
        return StreamingSession(self, B)

    # -- one-launch streaming step -------------------------------------------------------------
    def step_ok(self, B: int, L: int) -> bool:
        """True when ``step`` serves this model at (B, L): a model on the fused path and B * L <= 32 rows per group."""
        return lib.s5fxp_model_step_ok(self._h, int(B), int(L)) == 1

    def step(self, x, state: Optional[torch.Tensor], y: Optional[torch.Tensor] = None, B: int = 1, L: int = 1, groups: int = 1,
             x_bits: Optional[int] = None, x_exp: Optional[int] = None, state_out: Optional[torch.Tensor] = None,
             lane=0, exps=None) -> torch.Tensor:
        """One short chunk of `groups` independent streams as ONE kernel launch (``s5fxp_model_step``): enqueue only --
        nothing is synchronised, and nothing is allocated when `y` is given.

        x: (groups, B, L, d_in) int32 (or an FxpArray of that shape) or float32 (``s5fxp_model_step_f32``; x_bits / x_exp
        default to the encoder's input configuration); y: (groups, B, L, d_out) of the same dtype.  state: the carry
        (groups, n_layers, 2, B, P) int32, read and -- unless `state_out` names another tensor -- replaced in place; None
        starts from zeros and keeps no carry.  Every group is its own compute_best batch, exactly ``enqueue(...,
        groups=groups)``.  The status words (``lane_status(lane, groups)``, ``check_status(lane)``) are the caller's to
        read: ST_WIDE_INPUT means the results are invalid (serve the chunk through ``enqueue`` on a generic engine).

        exps: an (n_layers, 5) array of stated exponents (``exp_max`` has the layout) runs ``s5fxp_model_step_at[_f32]``: no
        group chooses exponents, so a stream's outputs no longer depend on how it is cut into steps."""
        if isinstance(x, FxpArray):
            x_bits, x_exp, x = x.bits, x.exp, x.data
        f32 = x.dtype == torch.float32
        if not f32 and x.dtype != torch.int32:
            raise ValueError(f"x must be int32 or float32, got {x.dtype}")
        want_x = (groups, B, L, self.d_in)
        if x.numel() != groups * B * L * self.d_in or not x.is_contiguous() or not x.is_cuda:
            raise ValueError(f"x must be a contiguous device tensor of shape {want_x}, got {tuple(x.shape)}")
        xb = (self.inp_bits if f32 else 32) if x_bits is None else int(x_bits)
        xe = self.inp_exp if x_exp is None else int(x_exp)
        if y is None:
            y = torch.empty((groups, B, L, self.d_out), dtype=x.dtype, device=x.device)
        elif y.dtype != x.dtype or y.numel() != groups * B * L * self.d_out or not y.is_contiguous():
            raise ValueError(f"y must be a contiguous {x.dtype} tensor of {groups * B * L * self.d_out} elements")
        want = (groups, self.n_layers, 2, B, self.P)
        for name, t in (("state", state), ("state_out", state_out)):
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous() or not t.is_cuda):
                raise ValueError(f"{name} must be a contiguous int32 device tensor of shape {want}")
        so = state_out if state_out is not None else state
        self._groups[lane] = groups
        name = "s5fxp_model_step" + ("_at" if exps is not None else "") + ("_f32" if f32 else "")
        eh = None if exps is None else self._exps_host(exps)   # the entry reads the host array before it returns: keep it alive
        tail = () if eh is None else (eh.ctypes.data,)
        check(getattr(lib, name)(self._h, x.data_ptr(), xb, xe, groups, B, L, y.data_ptr(),
                                 state.data_ptr() if state is not None else None, so.data_ptr() if so is not None else None,
                                 self.lane_status(lane, groups).data_ptr(), *tail, torch.cuda.current_stream().cuda_stream), name)
        return y

    # -- stated exponents ----------------------------------------------------------------------
    def _exps_host(self, exps) -> np.ndarray:
        """`exps` as the contiguous host int32 array the _at entries read, (n_layers, 5)."""
        e = np.ascontiguousarray(np.asarray(exps, dtype=np.int32))
        if e.shape != (self.n_layers, 5):
            raise ValueError(f"exps must have shape ({self.n_layers}, 5), got {e.shape}")
        return e

    def exp_max(self) -> np.ndarray:
        """(n_layers, 5) int32: the largest exponent each of a layer's five compute_best ops can take -- BatchNorm add(-mean),
        mul(invsq_var), mul(scale), add(bias) and the residual add, the order of status words [8 + 8 * l + 0 .. 4] -- and -1
        where the layer has no such op (``s5fxp_model_exp_max``)."""
        return np.array([[lib.s5fxp_model_exp_max(self._h, l, k) for k in range(5)] for l in range(self.n_layers)], dtype=np.int32)

    def check_exps(self, exps) -> None:
        """Raises what the _at entries would refuse `exps` with (``s5fxp_model_exps_check``, host only): ValueError for an
        exponent outside 0 .. ``exp_max()`` or one that makes a shift negative or larger than 31, NotImplementedError for a
        model off the fused path or of more than 8 layers."""
        eh = self._exps_host(exps)
        rc = lib.s5fxp_model_exps_check(self._h, eh.ctypes.data)
        if rc == _lib.S5FXP_EBADARG:
            raise ValueError("s5fxp_model_exps_check: an exponent is outside 0 .. exp_max()")
        check(rc, "s5fxp_model_exps_check")

    def calibrate_exps(self, clips, headroom: int = 0, lane=0) -> np.ndarray:
        """Exponents for ``exps=`` from data: runs ``forward_clips`` on `clips` (a list of FxpArray) and takes, per layer and
        op, the MINIMUM of the exponents the clips chose -- the largest range any of them needed -- over the clips that have
        frames and no error bit; `headroom` more integer bits are then taken off, not below 0.  Host arithmetic on the status
        words of the one launch.  Returns (n_layers, 5) int32, 0 where the layer has no such op."""
        clips = list(clips)
        self.forward_clips(clips, lane=lane)
        n, W = len(clips), _lib.STATUS_WORDS
        st = self.lane_status(lane, n).cpu().numpy()[:n * W].reshape(n, W)
        ok = np.array([c.data.shape[0] > 0 for c in clips], dtype=bool) & ((st[:, 0] & ~_lib.ST_WIDE_STATE) == 0)
        if not ok.any():
            raise ValueError("calibrate_exps: no clip with frames came back without an error bit")
        e = st[ok][:, 8:8 + 8 * self.n_layers].reshape(-1, self.n_layers, 8)[:, :, :5].min(axis=0)
        return np.where(self.exp_max() >= 0, np.maximum(e - int(headroom), 0), 0).astype(np.int32)

    # -- many clips of different lengths, one launch --------------------------------------------
    def clips_ok(self, Lmax: int) -> bool:
        """True when ``clips`` serves this model at Lmax frames per clip: a model on the fused path."""
        return lib.s5fxp_model_clips_ok(self._h, int(Lmax)) == 1

    def _clips_workspace(self, n: int, Lmax: int, lane) -> torch.Tensor:
        """The lane's scratch for a clip launch (kept apart from the batch path's workspace of the same lane)."""
        key, ws = self._wsl.get(("clips", lane), (None, None))
        if key != (n, Lmax):
            ws = torch.empty(lib.s5fxp_clips_workspace_bytes(self._h, n, Lmax), dtype=torch.uint8, device=self.device)
            self._wsl[("clips", lane)] = ((n, Lmax), ws)
        return ws

    def clips(self, x, lens: torch.Tensor, y: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
              state_out: Optional[torch.Tensor] = None, x_bits: Optional[int] = None, x_exp: Optional[int] = None,
              lane=0, exps=None) -> torch.Tensor:
        """n clips of different lengths as ONE kernel launch (``s5fxp_model_clips``): enqueue only -- nothing is
        synchronised, and apart from the lane's scratch nothing is allocated when `y` is given.

        x: (n, Lmax, d_in) int32 (or an FxpArray of that shape) or float32 (``s5fxp_model_clips_f32``; x_bits / x_exp default
        to the encoder's input configuration), clip e in rows 0 .. lens[e]-1 of x[e]; lens: (n,) int32 device tensor; y:
        (n, Lmax, d_out) of the same dtype -- rows from lens[e] on are never written.  state: the carry (n, n_layers, 2, P)
        int32, read and -- unless `state_out` names another tensor -- replaced in place; None starts from zeros and keeps no
        carry.  Clip e gets, bit for bit, ``enqueue(x[e, :len], ..., B=1, L=len)`` on its own: own compute_best exponents,
        own status words (``lane_status(lane, n)``), own carry, whatever else is in the launch.  The status words are the
        caller's to read: a clip with ST_WIDE_INPUT has left its y rows and carry untouched (serve it on ``generic_twin()``).

        The trade-off: one workgroup -- one CU -- walks a clip tile by tile (107 us per 32 frames at dim_scale 0.5, 143 us at
        1.0), so the launch is as long as its longest clip and pays off for MANY short clips, where the batch path needs 17
        launches (93 .. 165 us) per clip.  Measured break-even: about 5 clips of 128 frames, 15 .. 20 clips
        of mixed lengths up to 512 frames; 10 .. 19 times faster than per-clip forwards from 256 clips on.  A single clip
        never pays (32 frames: 127 against 93 us; 2048 frames: 6.8 against 0.15 ms): it belongs on ``forward``, which spreads
        it over the chip.  Clips that share one length are 3.6 .. 4 times faster on ``forward_batches``.

        exps: an (n_layers, 5) array of stated exponents (``exp_max`` has the layout; ``calibrate_exps`` makes one from data)
        runs ``s5fxp_model_clips_at[_f32]``: every clip at those exponents instead of its own, which is what a stream pushed
        through ``SessionPool(exps=)`` computes for the same signal however it is cut."""
        return self._clips_launch(x, lens, y, state, state_out, x_bits, x_exp, lane, False, None, exps)[0]

    def clips_traced(self, x, lens: torch.Tensor, y: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
                     state_out: Optional[torch.Tensor] = None, x_bits: Optional[int] = None, x_exp: Optional[int] = None,
                     lane=0, traces: Optional[List[Dict[str, torch.Tensor]]] = None):
        """``clips`` with the eleven trace planes of every layer (``s5fxp_model_clips_traced[_f32]``): still ONE
        launch, enqueue only, no sync.  Returns ``(y, traces)``: ``traces[l][k]`` for ``k`` in ``TRACE_FIELDS`` is an int32 plane
        padded like y, (n, Lmax, H) or (n, Lmax, P) for ``Bu_*`` / ``xs_*``; rows t < lens[e] of clip e are bit for bit what
        ``forward(x[e, :len], traces=True)`` stores, rows from lens[e] on are never written (``torch.empty`` unless `traces`
        hands in the planes).  y, the carry and the status words are those of ``clips``.  A diagnostic path: the traced kernel
        stores 11 planes per layer and is slower than ``clips``."""
        return self._clips_launch(x, lens, y, state, state_out, x_bits, x_exp, lane, True, traces)

    def _clips_launch(self, x, lens, y, state, state_out, x_bits, x_exp, lane, traced: bool, traces, exps=None):
        """The checks and the one launch behind ``clips`` and ``clips_traced`` -> (y, the trace planes or None)."""
        if isinstance(x, FxpArray):
            x_bits, x_exp, x = x.bits, x.exp, x.data
        f32 = x.dtype == torch.float32
        if not f32 and x.dtype != torch.int32:
            raise ValueError(f"x must be int32 or float32, got {x.dtype}")
        if x.ndim != 3 or x.shape[-1] != self.d_in or not x.is_contiguous() or not x.is_cuda or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x must be a contiguous device tensor of shape (n, Lmax, {self.d_in}), got {tuple(x.shape)}")
        n, Lmax = int(x.shape[0]), int(x.shape[1])
        if lens.dtype != torch.int32 or tuple(lens.shape) != (n,) or not lens.is_contiguous() or not lens.is_cuda:
            raise ValueError(f"lens must be a contiguous int32 device tensor of shape ({n},)")
        xb = (self.inp_bits if f32 else 32) if x_bits is None else int(x_bits)
        xe = self.inp_exp if x_exp is None else int(x_exp)
        if y is None:
            y = torch.empty((n, Lmax, self.d_out), dtype=x.dtype, device=x.device)
        elif y.dtype != x.dtype or tuple(y.shape) != (n, Lmax, self.d_out) or not y.is_contiguous() or not y.is_cuda:
            raise ValueError(f"y must be a contiguous {x.dtype} device tensor of shape {(n, Lmax, self.d_out)}")
        want = (n, self.n_layers, 2, self.P)
        for name, t in (("state", state), ("state_out", state_out)):
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous() or not t.is_cuda):
                raise ValueError(f"{name} must be a contiguous int32 device tensor of shape {want}")
        tail = ()
        if traced:
            if traces is None:
                traces = [self._trace_planes(x) for _ in range(self.n_layers)]
            if len(traces) != self.n_layers:
                raise ValueError(f"traces must have {self.n_layers} entries, got {len(traces)}")
            tr = (LayerTrace * self.n_layers)()
            for t, planes in zip(tr, traces):
                for k in TRACE_FIELDS:
                    pl = planes.get(k)
                    if pl is None:
                        continue
                    w = self.P if k in ("Bu_re", "Bu_im", "xs_re", "xs_im") else self.H
                    if pl.dtype != torch.int32 or tuple(pl.shape) != (n, Lmax, w) or not pl.is_contiguous() or pl.device != x.device:
                        raise ValueError(f"trace plane {k} must be a contiguous int32 device tensor of shape {(n, Lmax, w)}")
                    setattr(t, k, pl.data_ptr())
            tail = (tr,)
        eh = None if exps is None else self._exps_host(exps)   # read before the entry returns: kept alive until then
        if eh is not None:
            tail = (eh.ctypes.data,)
        so = state_out if state_out is not None else state
        ws = self._clips_workspace(n, Lmax, lane)
        self._groups[lane] = n
        name = "s5fxp_model_clips" + ("_traced" if traced else "_at" if exps is not None else "") + ("_f32" if f32 else "")
        check(getattr(lib, name)(self._h, x.data_ptr(), xb, xe, n, Lmax, lens.data_ptr(), y.data_ptr(),
                                 state.data_ptr() if state is not None else None, so.data_ptr() if so is not None else None,
                                 ws.data_ptr(), ws.numel(), self.lane_status(lane, n).data_ptr(), *tail,
                                 torch.cuda.current_stream().cuda_stream), name)
        return y, traces

    def _forward_clips(self, xs, dtype: torch.dtype, xb: int, xe: int, lane, exps=None) -> List[torch.Tensor]:
        """Pads the clips (each (L_e, d_in) of `dtype`), launches once, reads the status once; a clip the 16-bit planes
        cannot hold (ST_WIDE_INPUT) is served on the generic engine on its own -- or, with `exps`, raises: the generic engine
        cannot honour stated exponents.  Returns the (L_e, d_out) outputs."""
        datas = []
        for d in xs:
            d = torch.as_tensor(d)
            if d.ndim != 2 or d.shape[-1] != self.d_in or d.dtype != dtype:
                raise ValueError(f"every clip must be a (L, {self.d_in}) {dtype} array, got {tuple(d.shape)} {d.dtype}")
            datas.append(d.to(self.device))
        n = len(datas)
        lens = [int(d.shape[0]) for d in datas]
        Lmax = max(lens, default=0)
        if Lmax == 0:
            return [torch.empty((0, self.d_out), dtype=dtype, device=self.device) for _ in range(n)]
        if not self.clips_ok(Lmax):
            raise NotImplementedError("the clip kernel needs a model on the fused path: use forward() clip by clip")
        x = torch.zeros((n, Lmax, self.d_in), dtype=dtype, device=self.device)
        for e, d in enumerate(datas):
            x[e, :lens[e]] = d
        y = self.clips(x, torch.tensor(lens, dtype=torch.int32, device=self.device), x_bits=xb, x_exp=xe, lane=lane, exps=exps)
        st = self.lane_status(lane, n).cpu().numpy()[:n * _lib.STATUS_WORDS].reshape(n, _lib.STATUS_WORDS)
        bad = int(np.bitwise_or.reduce(st[:, 0] & ~_lib.ST_WIDE_INPUT))
        if bad & _lib.ST_NEGSHIFT:
            raise ValueError("invalid result_exp: a data-dependent shift came out negative (fxparray.py:619-621)")
        if bad & _lib.ST_NEGEXP:
            raise ValueError("a compute_best exponent came out negative")
        out = [y[e, :lens[e]] for e in range(n)]
        if exps is not None and (st[:, 0] & _lib.ST_WIDE_INPUT).any():
            raise OverflowError("a clip holds input values beyond 16 bits: only the generic engine serves it, and that engine "
                                "chooses its own exponents")
        for e in np.nonzero(st[:, 0] & _lib.ST_WIDE_INPUT)[0]:
            out[e] = self.generic_twin()._forward(datas[e].contiguous(), xb, xe, dtype, False, None, True)[0]
        return out

    def forward_clips(self, xs, lane=0, exps=None) -> List[FxpArray]:
        """xs: a list of FxpArray (L_e, d_in) of one configuration, lengths free (0 included).  Returns the list of
        FxpArray (L_e, d_out) that ``forward`` gives each clip on its own, from ONE kernel launch (``clips``) and one
        read of the status words.  For many short clips; see ``clips`` for where a long clip belongs.  With `exps` every
        clip runs at those stated exponents instead (``clips(..., exps=)``)."""
        xs = list(xs)
        if not xs:
            return []
        cfg = {(x.bits, x.exp) for x in xs}
        if len(cfg) != 1:
            raise ValueError(f"the clips of one launch share one input configuration, got {sorted(cfg)}")
        (xb, xe), = cfg
        return [self._fxp(y) for y in self._forward_clips([x.data for x in xs], torch.int32, xb, xe, lane, exps)]

    def forward_clips_float(self, xs, x_bits: Optional[int] = None, x_exp: Optional[int] = None, lane=0,
                            exps=None) -> List[torch.Tensor]:
        """The same for float32 clips (L_e, d_in): fxp_from_fp (FLOOR) to (x_bits, x_exp) -- the encoder's input configuration
        by default -- the model, to_float, in the one launch.  Returns float32 tensors (L_e, d_out)."""
        xs = [torch.as_tensor(x) for x in xs]
        return self._forward_clips(xs, torch.float32, self.inp_bits if x_bits is None else int(x_bits),
                                   self.inp_exp if x_exp is None else int(x_exp), lane, exps)

    def generic_twin(self) -> "Engine":
        """The same model on the generic int32 kernels (MODEL_FORCE_GENERIC), built on first use: what serves inputs the
        fused kernels refuse (ST_WIDE_INPUT)."""
        if self._flags & _lib.MODEL_FORCE_GENERIC:
            return self
        if self._generic is None:
            self._generic = Engine(self._export, self._flags | _lib.MODEL_FORCE_GENERIC, self.device)
        return self._generic

    def pool(self, sessions: int, B: int = 1, exps=None) -> "SessionPool":
        return SessionPool(self, sessions, B, exps)


class StreamingSession:
    """Frame-chunk-at-a-time inference with the SSM states carried between calls (the paper's
    real-time denoising use).  ``push`` takes (B,L,d_in) / (L,d_in) chunks of any length and returns the outputs of
    exactly those frames."""

    def __init__(self, engine: "Engine", B: int = 1):
        self.engine, self.B = engine, B
        self.state = engine.zero_state(B)
        self.frames = 0

    def push(self, x: FxpArray) -> FxpArray:
        y, self.state = self.engine.forward_chunk(x, self.state)
        self.frames += x.data.shape[-2]
        return y

    def reset(self) -> None:
        self.state = self.engine.zero_state(self.B)
        self.frames = 0


class SessionPool:
    """`sessions` independent streams of B sequences each, served together: one group per session, every chunk of all
    sessions in ONE kernel launch (``Engine.step``) where the model and the chunk allow it -- a model on the fused path and
    B * L <= 32 rows per session -- and through the grouped batch path (``Engine.enqueue(..., groups=sessions)``) or the
    generic engine otherwise, so every model and chunk length is served.  The pool owns the carry (updated by every push)
    and reusable output buffers: what ``push`` returns is valid until the next push of the same chunk shape.

    Each session's chunk is its own compute_best batch: session s of a pool computes what a ``StreamingSession`` fed the
    same chunks computes.

    exps: an (n_layers, 5) array of stated exponents (``Engine.exp_max`` has the layout, ``Engine.calibrate_exps`` makes one)
    replaces that rule: every push runs the _at entries at those exponents, so a session's outputs are the same however its
    signal is cut into pushes, and equal ``Engine.clips(..., exps=)`` on the whole signal.  A push of more than 32 rows per
    session is then split into steps of at most 32 rows instead of leaving the step kernel, and a chunk with input values
    beyond 16 bits raises: the generic engine, which serves such chunks otherwise, chooses its own exponents."""

    def __init__(self, engine: "Engine", sessions: int, B: int = 1, exps=None):
        if sessions < 1 or B < 1:
            raise ValueError("sessions and B must be >= 1")
        self.engine, self.sessions, self.B = engine, int(sessions), int(B)
        self.exps = None
        if exps is not None:
            engine.check_exps(exps)
            self.exps = engine._exps_host(exps).copy()
            if not engine.step_ok(self.B, 1):
                raise NotImplementedError(f"stated exponents need the step kernel, which serves B <= {32} sequences per session")
        shape = (self.sessions, engine.n_layers, 2, self.B, engine.P)
        self._state = torch.zeros(shape, dtype=torch.int32, device=engine.device)
        self._next = torch.zeros(shape, dtype=torch.int32, device=engine.device)
        self.frames = np.zeros(self.sessions, dtype=np.int64)
        self.last_path: Optional[int] = None
        self._lane = ("pool", id(self))
        self._y: Dict[tuple, torch.Tensor] = {}
        self._err = torch.zeros(self.sessions, dtype=torch.int32, device=engine.device)  # error bits of unchecked pushes
        self._unchecked = False
        self._desc = None   # push_ragged: (device descriptors, [pinned staging buffer, its copy's event] x 2, turn)

    @property
    def state(self) -> torch.Tensor:
        """The carry, (sessions, n_layers, 2, B, P) int32."""
        return self._state

    def reset(self, ids=None) -> None:
        """Zeroes the carry (and the frame count) of the sessions in `ids`; None: all of them."""
        if ids is None:
            self._state.zero_()
            self.frames[:] = 0
        else:
            idx = torch.as_tensor(list(ids), dtype=torch.long, device=self._state.device)
            self._state.index_fill_(0, idx, 0)
            self.frames[list(ids)] = 0

    def _raise(self, bits: int) -> None:
        if bits & _lib.ST_NEGSHIFT:
            raise ValueError("invalid result_exp: a data-dependent shift came out negative (fxparray.py:619-621)")
        if bits & _lib.ST_NEGEXP:
            raise ValueError("a compute_best exponent came out negative")
        if bits & _lib.ST_WIDE_INPUT:
            raise OverflowError("an unchecked push held input values beyond 16 bits: its outputs and the carry are invalid; "
                                "reset the sessions and push with check=True")

    def check(self) -> None:
        """Synchronises and raises what an unchecked push since the last check would have raised."""
        if self._unchecked:
            bits = int(np.bitwise_or.reduce(self._err.cpu().numpy()))
            self._err.zero_()
            self._unchecked = False
            self._raise(bits)

    def _batch(self, eng: "Engine", x, xb, xe, y, L, check: bool) -> None:
        S = self.sessions
        sin, sout = (self._state, self._next) if S > 1 else (self._state[0], self._next[0])
        launch = lambda fl: eng.enqueue(x, xb, xe, y, self.B, L, flags=fl, lane=self._lane, state_in=sin, state_out=sout, groups=S)
        if check:
            eng.run_ladder(launch, lambda: eng.check_status(self._lane))
            self.last_path = int(eng.lane_status(self._lane, S)[2].item())
        else:
            launch(0)  # self-contained: the gated exact re-run is part of the one enqueue
            self._err |= eng.lane_status(self._lane, S)[:S * _lib.STATUS_WORDS].view(S, _lib.STATUS_WORDS)[:, 0]
            self._unchecked = True
            self.last_path = _lib.PATH_FUSED if lib.s5fxp_model_is_fast(eng._h) else _lib.PATH_GENERIC
        self._state, self._next = self._next, self._state

    def _push_pinned(self, data, xb, xe, y, L: int, check: bool) -> None:
        """A push at stated exponents: steps of at most 32 // B frames per sequence, each one launch on the carry in place."""
        eng, S, B = self.engine, self.sessions, self.B
        step = max(1, 32 // B)
        d4, y4 = data.view(S, B, L, eng.d_in), y.view(S, B, L, eng.d_out)
        for t0 in range(0, L, step):
            t1 = min(L, t0 + step)
            whole = t0 == 0 and t1 == L
            xs = d4 if whole else d4[:, :, t0:t1].contiguous()
            ys = y4 if whole else torch.empty((S, B, t1 - t0, eng.d_out), dtype=y.dtype, device=y.device)
            eng.step(xs, self._state, ys, B, t1 - t0, S, xb, xe, lane=self._lane, exps=self.exps)
            if not whole:
                y4[:, :, t0:t1] = ys
            st = eng.lane_status(self._lane, S)
            if check:
                bits = int(np.bitwise_or.reduce(st.cpu().numpy()[:S * _lib.STATUS_WORDS].reshape(S, _lib.STATUS_WORDS)[:, 0]))
                if bits & _lib.ST_WIDE_INPUT:
                    raise OverflowError("a chunk holds input values beyond 16 bits: only the generic engine serves it, and that "
                                        "engine chooses its own exponents; the carry is invalid, reset the sessions")
            else:
                self._err |= st[:S * _lib.STATUS_WORDS].view(S, _lib.STATUS_WORDS)[:, 0]
                self._unchecked = True
        self.last_path = _lib.PATH_STEP

    def push(self, x, check: bool = True):
        """x: (sessions, L, d_in) (B == 1) or (sessions, B, L, d_in), an FxpArray or a float32 tensor.  Returns the outputs
        of exactly those frames, an FxpArray or a float32 tensor of the same leading shape.  check=False enqueues only:
        nothing is synchronised, the status words are folded into the pool on the device and raised by the next checked
        push or ``check()``."""
        eng = self.engine
        fxp = isinstance(x, FxpArray)
        if fxp:
            data, xb, xe = x.data, x.bits, x.exp
            if data.dtype != torch.int32:
                raise ValueError(f"expected int32 FxpArray data, got {data.dtype}")
        else:
            data = torch.as_tensor(x)
            if data.dtype != torch.float32:
                raise ValueError(f"expected an FxpArray or a float32 tensor, got {data.dtype}")
            xb, xe = eng.inp_bits, eng.inp_exp
        data = data.to(eng.device).contiguous()
        S, B = self.sessions, self.B
        if data.ndim == 3 and B == 1:
            L = data.shape[1]
        elif data.ndim == 4 and data.shape[1] == B:
            L = data.shape[2]
        else:
            raise ValueError(f"expected ({S}, L, {eng.d_in})" + (f" or ({S}, {B}, L, {eng.d_in})"), f"got {tuple(data.shape)}")
        if data.shape[0] != S or data.shape[-1] != eng.d_in or L < 1:
            raise ValueError(f"expected {S} sessions of {eng.d_in} inputs and at least one frame, got {tuple(data.shape)}")
        if check:
            self.check()
        key = (tuple(data.shape[:-1]), data.dtype)
        y = self._y.get(key)
        if y is None:
            y = self._y[key] = torch.empty(key[0] + (eng.d_out,), dtype=data.dtype, device=eng.device)
        if self.exps is not None:
            self._push_pinned(data, xb, xe, y, L, check)
        elif eng.step_ok(B, L):
            if check:
                eng.step(data, self._state, y, B, L, S, xb, xe, state_out=self._next, lane=self._lane)
                st = eng.lane_status(self._lane, S).cpu().numpy()[:S * _lib.STATUS_WORDS].reshape(S, _lib.STATUS_WORDS)
                bits = int(np.bitwise_or.reduce(st[:, 0]))
                if bits & _lib.ST_WIDE_INPUT:
                    # the fused kernels take 16-bit inputs: this chunk goes through the generic engine, from the same carry
                    self._batch(eng.generic_twin(), data, xb, xe, y, L, True)
                else:
                    self._raise(bits)
                    self._state, self._next = self._next, self._state
                    self.last_path = int(st[0, 2])
            else:
                eng.step(data, self._state, y, B, L, S, xb, xe, lane=self._lane)
                self._err |= eng.lane_status(self._lane, S)[:S * _lib.STATUS_WORDS].view(S, _lib.STATUS_WORDS)[:, 0]
                self._unchecked = True
                self.last_path = _lib.PATH_STEP
        else:
            self._batch(eng, data, xb, xe, y, L, check)
        self.frames += L
        return FxpArray(y, eng.out_bits, eng.out_exp, True) if fxp else y


    # -- sessions that start, stop and idle on their own -----------------------------------------------------
    def stage_desc(self, ids, rows, flags, hops=None, h4=None, Lmax: int = 0, cmax: int = 0) -> torch.Tensor:
        """Builds the ``s5fxp_push_desc`` array of a ragged push (one entry per id: sequences or arrays of integers; `hops` /
        `h4` for the audio kernels), validates it on the host (``s5fxp_push_desc_check``) and copies it to the device without
        blocking.  Returns the device array, (len(ids), 8) int32, valid until the next call.  Two pinned staging buffers
        alternate, and one is written again only after the copy that last read it has completed."""
        n, audio = len(ids), hops is not None
        if self._desc is None:
            dev = torch.zeros((self.sessions, 8), dtype=torch.int32, device=self.engine.device)
            pins = [torch.zeros((self.sessions, 8), dtype=torch.int32).pin_memory() for _ in range(2)]
            self._desc = [dev, [[p, p.numpy(), torch.cuda.Event(), False] for p in pins], 0]
        dev, pins, turn = self._desc
        if not 1 <= n <= self.sessions:
            raise ValueError(f"a push names 1 .. {self.sessions} sessions, got {n}")
        pin = pins[turn]
        if pin[3]:
            pin[2].synchronize()   # the copy that last read this buffer
        host = pin[1]
        host[:n, 0], host[:n, 1], host[:n, 2] = ids, rows, flags
        if audio:
            host[:n, 3], host[:n, 4] = hops, h4
        else:
            host[:n, 3:5] = 0
        check(lib.s5fxp_push_desc_check(host.ctypes.data, n, self.sessions, int(Lmax), int(cmax), int(audio)), "s5fxp_push_desc_check")
        out = dev[:n]
        out.copy_(pin[0][:n], non_blocking=True)
        pin[2].record()
        pin[3] = True
        self._desc[2] = turn ^ 1
        return out

    def _entry(self, eng: "Engine", e: int, slot: int, data, xb, xe, y, L: int, fresh: bool, fxp: bool) -> None:
        """One entry of a ragged push on the per-session route: ``forward_chunk*`` of `eng` on the slot's carry."""
        if fresh:
            self._state[slot].zero_()
        if L == 0:
            return
        chunk = data[e][..., :L, :].contiguous()
        if fxp:
            out, new = eng.forward_chunk(FxpArray(chunk, xb, xe, True), self._state[slot])
            out = out.data
        else:
            out, new = eng.forward_chunk_float(chunk, self._state[slot], xb, xe)
        y[e][..., :L, :] = out
        self._state[slot].copy_(new)

    def push_ragged(self, ids, x, rows, fresh=(), check: bool = True, desc: Optional[torch.Tensor] = None):
        """One push for any subset of the pool: entry e is session ``ids[e]`` with its first ``rows[e]`` frames (0 .. Lmax) of
        x[e]; sessions not named idle.  x: (n, Lmax, d_in) (B == 1) or (n, B, Lmax, d_in), an FxpArray or a float32 tensor;
        ids, rows and fresh are sequences or arrays of integers.  Returns the padded outputs of the same leading shape: frames
        rows[e] .. Lmax-1 of entry e are never read and their outputs are not written.  Sessions in `fresh` start a new
        signal: their carry is taken as zeros (no reset needed), and with rows == 0 it is zeroed.  One kernel launch
        (``s5fxp_model_step_ragged``) updates the carries in place.  Each entry computes what ``push`` computes for that
        session alone with that chunk.  `desc`: the descriptor array of exactly these ids, rows and fresh, already validated
        and staged with ``stage_desc`` (audio.SessionDenoiser shares one among its three launches).

        check=True reads the status words: an entry that came back with ST_WIDE_INPUT -- its outputs and carry untouched -- is
        served from its carry by the generic engine; NEGSHIFT / NEGEXP raise ValueError, and the carries of the sessions of
        that push are then invalid and need ``reset(ids)``.  check=False folds the status words into the pool as ``push``
        does.  A model or chunk the step kernel does not serve takes ``Engine.forward_chunk*`` entry by entry: correct, not
        fast."""
        eng = self.engine
        fxp = isinstance(x, FxpArray)
        if fxp:
            data, xb, xe = x.data, x.bits, x.exp
            if data.dtype != torch.int32:
                raise ValueError(f"expected int32 FxpArray data, got {data.dtype}")
        else:
            data = torch.as_tensor(x)
            if data.dtype != torch.float32:
                raise ValueError(f"expected an FxpArray or a float32 tensor, got {data.dtype}")
            xb, xe = eng.inp_bits, eng.inp_exp
        data = data.to(eng.device).contiguous()
        ids, rows, B = np.asarray(ids, dtype=np.int64).reshape(-1), np.asarray(rows, dtype=np.int64).reshape(-1), self.B
        n = len(ids)
        if data.ndim == 3 and B == 1:
            Lmax = data.shape[1]
        elif data.ndim == 4 and data.shape[1] == B:
            Lmax = data.shape[2]
        else:
            raise ValueError(f"expected (n, Lmax, {eng.d_in})" + (f" or (n, {B}, Lmax, {eng.d_in})") + f", got {tuple(data.shape)}")
        if n < 1 or data.shape[0] != n or len(rows) != n or data.shape[-1] != eng.d_in or Lmax < 1:
            raise ValueError(f"expected one row count and one ({'' if B == 1 else str(B) + ', '}Lmax >= 1, {eng.d_in}) block per id, "
                             f"got {n} ids, {len(rows)} row counts and x {tuple(data.shape)}")
        new = np.zeros(n, dtype=bool) if not len(fresh) else np.isin(ids, np.asarray(fresh, dtype=np.int64))
        if desc is None:
            seen = np.zeros(self.sessions, dtype=bool)
            if ids.min() < 0 or ids.max() >= self.sessions:
                raise ValueError(f"ids must be sessions 0 .. {self.sessions - 1}, got {ids.tolist()}")
            seen[ids] = True
            if int(seen.sum()) != n:
                raise ValueError(f"a session is named twice: {ids.tolist()}")
            if rows.min() < 0 or rows.max() > Lmax:
                raise ValueError(f"rows must be 0 .. {Lmax}, got {rows.tolist()}")
            if int(new.sum()) != len(set(int(i) for i in fresh)):
                raise ValueError("fresh names a session that is not in ids")
        if check:
            self.check()
        key = ("ragged", tuple(data.shape[:-1]), data.dtype)
        y = self._y.get(key)
        if y is None:
            y = self._y[key] = torch.empty(key[1] + (eng.d_out,), dtype=data.dtype, device=eng.device)
        W = _lib.STATUS_WORDS
        if self.exps is not None and not eng.step_ok(B, Lmax):
            # stated exponents: the result does not depend on the split, so a long push is steps of at most 32 rows
            if desc is not None:
                raise NotImplementedError("a staged descriptor array describes one step: push at most 32 rows per session with it")
            step = max(1, 32 // B)
            d4, y4 = data.view(n, B, Lmax, eng.d_in), y.view(n, B, Lmax, eng.d_out)
            for t0 in range(0, Lmax, step):
                t1 = min(Lmax, t0 + step)
                xs = d4[:, :, t0:t1].reshape((n,) + ((B,) if data.ndim == 4 else ()) + (t1 - t0, eng.d_in))
                part = self.push_ragged(ids, FxpArray(xs, xb, xe, True) if fxp else xs, np.clip(rows - t0, 0, t1 - t0),
                                        fresh if t0 == 0 else (), check)
                y4[:, :, t0:t1] = (part.data if fxp else part).view(n, B, t1 - t0, eng.d_out)
            return FxpArray(y, eng.out_bits, eng.out_exp, True) if fxp else y
        if eng.step_ok(B, Lmax):
            if desc is None:
                desc = self.stage_desc(ids, rows, new * _lib.PUSH_FRESH, Lmax=Lmax)
            name = "s5fxp_model_step_ragged" + ("_at" if self.exps is not None else "") + ("" if fxp else "_f32")
            tail = () if self.exps is None else (self.exps.ctypes.data,)
            st = eng.lane_status(self._lane, n)
            eng._groups[self._lane] = n
            _lib.check(getattr(lib, name)(eng._h, data.data_ptr(), xb, xe, n, B, Lmax, y.data_ptr(), desc.data_ptr(),
                                          self._state.data_ptr(), self.sessions, st.data_ptr(), *tail,
                                          torch.cuda.current_stream().cuda_stream), name)
            self.last_path = _lib.PATH_STEP
            if check:
                bits = st.cpu().numpy()[:n * W].reshape(n, W)[:, 0]
                if self.exps is not None and (bits & _lib.ST_WIDE_INPUT).any():
                    raise OverflowError("an entry holds input values beyond 16 bits: only the generic engine serves it, and that "
                                        "engine chooses its own exponents")
                for e in np.nonzero(bits & _lib.ST_WIDE_INPUT)[0]:
                    # the kernel left this entry's outputs and carry alone: the generic engine serves it from that carry
                    self._entry(eng.generic_twin(), int(e), int(ids[e]), data, xb, xe, y, int(rows[e]), bool(new[e]), fxp)
                    self.last_path = _lib.PATH_GENERIC
                self._raise(int(np.bitwise_or.reduce(bits)) & ~_lib.ST_WIDE_INPUT)
            else:
                # check() reduces the words with OR: which session a word belongs to does not matter
                self._err[:n] |= st[:n * W].view(n, W)[:, 0]
                self._unchecked = True
        else:
            for e in range(n):
                self._entry(eng, e, int(ids[e]), data, xb, xe, y, int(rows[e]), bool(new[e]), fxp)
            self.last_path = _lib.PATH_FUSED if lib.s5fxp_model_is_fast(eng._h) else _lib.PATH_GENERIC
        if new.any():
            self.frames[ids[new]] = 0
        self.frames[ids] += rows
        return FxpArray(y, eng.out_bits, eng.out_exp, True) if fxp else y


class InflightRunner:
    """Keeps up to ``depth`` forwards of one Engine in flight, each on its own HIP stream and lane.

    One layer's recurrence is a latency chain that occupies B*P/16 waves; the projections around it want the
    whole chip.  Within one forward they cannot overlap (every layer's exponents depend on the whole previous
    layer), but the recurrence of one batch overlaps the projections of the others.  Batches are independent,
    so the results are the ones ``Engine.forward`` gives.

    submit() returns at once; a lane is synchronised and its status words are checked (with the exact re-run if
    ST_REDO came back) when the lane is reused or on drain().
    """

    def __init__(self, engine: Engine, depth: int = 3):
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.engine, self.depth = engine, depth
        self.streams = [torch.cuda.Stream(device=engine.device) for _ in range(depth)]
        self._pending: List[Optional[tuple]] = [None] * depth
        self._next = 0
        # engine lanes 1..depth: lane 0 (its workspace and status words) stays Engine.forward's, which may run on
        # another stream while batches are in flight here
        self._lane0 = 1

    def submit(self, x: torch.Tensor, x_bits: int, x_exp: int, y: torch.Tensor, B: int, L: int, check: bool = True,
               scan_events: Optional[list] = None, groups: int = 1, exps=None) -> int:
        """x and y: both int32, both float32 or both int16, as ``Engine.enqueue`` takes them; exps: stated exponents, as there.  check=False skips the status
        check of the lane's previous batch (only sound when every batch of the lane is the same input, as in bench.py: the
        last check then speaks for all)."""
        lane = self._next
        self._next = (lane + 1) % self.depth
        if check:
            self._finish(lane)
        s = self.streams[lane]
        s.wait_stream(torch.cuda.current_stream(self.engine.device))
        level = self.engine.level
        with torch.cuda.stream(s):
            self.engine.enqueue(x, x_bits, x_exp, y, B, L, flags=Engine.LEVEL_FLAGS[level], lane=self._lane0 + lane,
                                scan_events=scan_events, groups=groups, exps=exps)
        # the tensors were allocated on another stream: tell the caching allocator that this lane's stream uses them, so
        # that dropping the previous job's references below (check=False) cannot hand their memory out while kernels of
        # this stream still read or write it
        x.record_stream(s)
        y.record_stream(s)
        self._pending[lane] = (x, x_bits, x_exp, y, B, L, level, groups, exps)
        return lane

    def _finish(self, lane: int) -> None:
        job = self._pending[lane]
        if job is None:
            return
        self._pending[lane] = None
        s = self.streams[lane]
        s.synchronize()
        x, x_bits, x_exp, y, B, L, level, groups, exps = job
        st = self.engine.check_status(self._lane0 + lane)
        while (st[0] & _lib.ST_REDO) and level < 2:   # climb the ladder: pair -> quad -> exact
            level = self.engine.note_redo(level)
            with torch.cuda.stream(s):
                self.engine.enqueue(x, x_bits, x_exp, y, B, L, flags=Engine.LEVEL_FLAGS[level], lane=self._lane0 + lane, groups=groups,
                                    exps=exps)
            s.synchronize()
            st = self.engine.check_status(self._lane0 + lane)

    def lane_of(self, slot: int) -> int:
        """Engine lane (status words, workspace) of in-flight slot `slot`."""
        return self._lane0 + slot

    def drain(self) -> None:
        for lane in range(self.depth):
            self._finish(lane)
