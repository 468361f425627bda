"""Models and inputs from outside the one recipe (synth.make_model) the rest of the suite draws from.

The fused MFMA path takes any model s5fxp_fast.hpp fast_eligible admits: int8 weights over all of [-128, 127], a 16-bit D,
Bu up to 32 bits, every state live or only a few, gate exponents up to the PK16 epilogue's limits.  The recipe's models fill
only a corner of that (B_bar in [-2, 2], two thirds of the states dead).  The builders here make every model in float space
plus qconfig edits, so the product (build_regression_model -> Engine), the NumPy oracle (O.RegressionModel) and the C oracle
(cref.CModel of the product's export) all start from the same float tree and qconfig: no route sees an integer tensor the
other two never saw.

Families (``CASES``):
  F1 calibrated full range  -- the recipe with ``full_range`` (exponent = calibrated fraction bits): every state live
  F2 weights on the rails   -- chosen float entries scaled past the range, so every 8-bit matrix holds -128 and 127 in its
                               first and last row and column, and hence in every 32-wide tile along either axis
  F3 wide corners           -- D at 16 bits on both rails, Bu at 24 bits, a 32-bit decoder output, biases above 16 bits,
                               d_in / d_out at the edges of fast_eligible
  F4 live-state patterns    -- rows of the float B zeroed after calibration: n_live states per layer, placed as the leading
                               block (layer 0), the trailing block (layer 1) and with a stride (layer 2)
  F5 PK16 hazards           -- y_exp raised so that 2 cx leaves int16 while 2 cx + D u does not, l_exp - y_exp at 14
"""
from __future__ import annotations

import copy
from typing import Dict, List, Optional

import numpy as np

from oracle import fxp_oracle as O
from sparsernns_amd import synth

F32 = np.float32
FULL = dict(synth.W8A16, full_range=True)   # a local precision dict: synth.PRECISIONS stays as it is
RAIL = 1e6   # far past any calibrated range: quantises to the rail of the entry's sign


class Case:
    """One contract model: the float tree, the qconfig, dims, and edits the engine / oracles apply after construction."""

    def __init__(self, name: str, md: dict, qc: dict, dims: dict, **meta):
        self.name, self.md, self.qc, self.dims, self.meta = name, md, qc, dims, meta
        self._model = self._export = self._np = self._cm = None

    def model(self):
        """The product's model (sparsernns_amd.fxpmodel)."""
        if self._model is None:
            from sparsernns_amd.fxpmodel import build_regression_model
            self._model = build_regression_model(self.md, self.qc, self.dims["n_layers"])
        return self._model

    def export(self) -> dict:
        if self._export is None:
            self._export = self.model().export()
        return self._export

    def numpy_oracle(self) -> O.RegressionModel:
        if self._np is None:
            self._np = O.RegressionModel(self.md, self.qc, self.dims["n_layers"])
        return self._np

    def c_oracle(self):
        from oracle import cref
        if self._cm is None:
            self._cm = cref.CModel(self.export())
        return self._cm

    def engine(self, flags: int = 0):
        from sparsernns_amd.engine import Engine
        return Engine(self.export(), flags=flags) if flags else self.model().engine()

    @property
    def in_bits(self) -> int:
        return self.qc["encoder"]["inp_bits"]

    @property
    def in_exp(self) -> int:
        return self.qc["encoder"]["inp_exp"]


def _calibrate(dims: dict, precisions: dict, seed: int = 1919, calib_L: int = 256, edit_float=None, headroom: int = 0):
    """synth.make_model's steps with a precision dict of our own (make_model only takes the names of synth.PRECISIONS).
    headroom: integer bits added to the state (synth.make_model state_headroom_bits), so that the int16 recurrence rungs
    hold the full-range states and a forward on them completes without a step down the ladder."""
    md = synth.make_float_params(dims, seed)
    if edit_float is not None:
        edit_float(md)
    stats: dict = {}
    xcal = synth.make_input(2, calib_L, dims["d_in"], seed=seed + 1)
    synth.float_forward(md, xcal, dims["n_layers"], calibrate_bn=True, stats=stats)
    qc = synth.derive_qconfig(md, stats, dims["n_layers"], precisions)
    for k in ("x_re", "x_im"):
        qc["blocks"]["ssm"]["activations"][k]["exp"] -= headroom
    synth.cap_result_exponents(qc)
    synth._assert_exps_nonnegative(qc)
    return md, qc


def _layers(md: dict, dims: dict):
    return [md["encoder"][f"layers_{i}"] for i in range(dims["n_layers"])]


def _bbar_coef(mixer: dict) -> np.ndarray:
    """B_bar = coef[:, None] * B_tilde (synth.zoh): the per-state factor, so that a chosen B_bar entry can be set in float."""
    lam = (mixer["Lambda_re"] + 1j * mixer["Lambda_im"]).astype(np.complex64)
    step = np.exp(mixer["log_step"][:, 0]).astype(F32)
    lam_bar = np.exp(lam * step).astype(np.complex64)
    return (1 / lam * (lam_bar - 1)).astype(np.complex64)


def rail_mask(R: int, C: int) -> np.ndarray:
    """+1 / -1 where an (R, C) matrix is pushed to its rails, 0 elsewhere: every 5th entry of the first and last row and
    column carries +1 and the one two further on -1, so both rails sit in both edge rows and columns and in every 32-wide
    tile along either axis."""
    m = np.zeros((R, C), dtype=np.int8)
    for r in (0, R - 1):
        c = np.arange(C)
        m[r, c % 5 == 0] = 1
        m[r, c % 5 == 2] = -1
        m[r, C - 1] = -1 if r == 0 else 1
    for cc in (0, C - 1):
        r = np.arange(R)
        m[r % 5 == 1, cc] = 1
        m[r % 5 == 3, cc] = -1
    m[0, 0], m[R - 1, 0] = 1, -1
    return m


def _push_rails(md: dict, dims: dict):
    """F2: float entries scaled past the calibrated range (after calibration, so the exponents stay): 8-bit quantisation
    saturates them to -128 / 127."""
    for d in (md["encoder"]["encoder"], md["decoder"]):
        k = d["kernel"]
        m = rail_mask(*k.shape)
        d["kernel"] = np.where(m != 0, F32(RAIL) * m, k).astype(F32)
    for layer in _layers(md, dims):
        k = layer["out2"]["kernel"]
        m = rail_mask(*k.shape)
        layer["out2"]["kernel"] = np.where(m != 0, F32(RAIL) * m, k).astype(F32)
        mx = layer["mixer"]
        P, H = mx["B"].shape[:2]
        # B_bar[p, h] = coef[p] * B_tilde[p, h]: the re and im planes get their own masks (the im one mirrored)
        mre, mim = rail_mask(P, H), rail_mask(P, H)[:, ::-1]
        coef = _bbar_coef(mx)
        bt = (mx["B"][..., 0] + 1j * mx["B"][..., 1]).astype(np.complex128)
        want = F32(RAIL) * (mre + 1j * mim) / coef[:, None].astype(np.complex128)
        bt = np.where((mre != 0) | (mim != 0), want, bt)
        # an entry on a rail in one plane and zero-masked in the other: keep the other plane's value near 0
        mx["B"] = np.stack([bt.real, bt.imag], -1).astype(F32)
        C = mx["C"]
        Hc, Pc = C.shape[:2]
        cre, cim = rail_mask(Hc, Pc), rail_mask(Hc, Pc)[::-1]
        C[..., 0] = np.where(cre != 0, F32(RAIL) * cre, C[..., 0])
        C[..., 1] = np.where(cim != 0, F32(RAIL) * cim, C[..., 1])
        D = mx["D"]
        D[0], D[-1], D[1], D[-2] = RAIL, -RAIL, -RAIL, RAIL


def live_rows(P: int, n: int, place: str) -> np.ndarray:
    """Indices of the n live states: the leading block, the trailing block (state P - 1 live), or spread with a stride."""
    if place == "lead":
        return np.arange(n)
    if place == "trail":
        return np.arange(P - n, P)
    if n == 0:
        return np.arange(0)
    stride = max(1, P // n)
    idx = (P - 1 - np.arange(n) * stride)[::-1]   # the last state always among them
    return idx if idx.min() >= 0 else np.arange(P - n, P)


PLACES = ("lead", "trail", "stride")   # layer i takes PLACES[i % 3]


def _kill_states(md: dict, dims: dict, n_live: int, places=PLACES):
    for i, layer in enumerate(_layers(md, dims)):
        keep = np.zeros(dims["P"], dtype=bool)
        keep[live_rows(dims["P"], n_live, places[i % len(places)])] = True
        layer["mixer"]["B"][~keep] = 0


# --------------------------------------------------------------------------------------------------------------------
# families
# --------------------------------------------------------------------------------------------------------------------
def _dims(ds: float, **over) -> dict:
    d = synth.ndns_dims(ds)
    d.update(over)
    return d


def f1_full_range(ds: float) -> Case:
    dims = _dims(ds)
    md, qc = _calibrate(dims, FULL)
    return Case(f"F1_full_ds{ds}", md, qc, dims, family="F1")


def f2_rails(ds: float) -> Case:
    dims = _dims(ds)
    md, qc = _calibrate(dims, FULL)
    _push_rails(md, dims)
    return Case(f"F2_rails_ds{ds}", md, qc, dims, family="F2")


def f3_wide_D(ds: float) -> Case:
    """D at 16 bits, with entries on both 16-bit rails."""
    dims = _dims(ds)
    md, qc = _calibrate(dims, FULL)
    w = qc["blocks"]["ssm"]["weights"]["D"]
    absmax = max(float(np.abs(l["mixer"]["D"]).max()) for l in _layers(md, dims))
    w["bits"], w["exp"] = 16, synth.fracbits_from_absmax(absmax, 16)
    for l in _layers(md, dims):
        D = l["mixer"]["D"]
        D[0], D[-1] = RAIL, -RAIL
    synth.cap_result_exponents(qc)
    return Case(f"F3_D16_ds{ds}", md, qc, dims, family="F3", D_bits=16)


def f3_wide_bu(ds: float, bits: int = 24) -> Case:
    """Bu at 24 bits, exponents unchanged: the int16 Bu streams no longer provably fit (select_rung s16)."""
    dims = _dims(ds)
    md, qc = _calibrate(dims, FULL)
    a = qc["blocks"]["ssm"]["activations"]
    a["Bu_re"]["bits"] = a["Bu_im"]["bits"] = bits
    return Case(f"F3_Bu{bits}_ds{ds}", md, qc, dims, family="F3", Bu_bits=bits)


def f3_wide_out(ds: float) -> Case:
    """A 32-bit decoder output, encoder / out2 biases of 24 / 20 bits with the exponents raised to match."""
    dims = _dims(ds)
    md, qc = _calibrate(dims, FULL)
    qc["decoder"]["out_bits"] = 32
    qc["decoder"]["out_exp"] += 8
    qc["encoder"]["b_bits"], qc["encoder"]["b_exp"] = 24, qc["encoder"]["b_exp"] + 8
    qc["blocks"]["out2"]["b_bits"], qc["blocks"]["out2"]["b_exp"] = 20, qc["blocks"]["out2"]["b_exp"] + 4
    synth.cap_result_exponents(qc)
    return Case(f"F3_out32_ds{ds}", md, qc, dims, family="F3")


def f3_dims(d_in: int, d_out: int, ds: float = 0.5) -> Case:
    dims = _dims(ds, d_in=d_in, d_out=d_out)
    md, qc = _calibrate(dims, FULL)
    return Case(f"F3_dims{d_in}x{d_out}_ds{ds}", md, qc, dims, family="F3")


def f4_live(ds: float, n_live: int) -> Case:
    """n_live states per layer (leading / trailing / strided in layers 0 / 1 / 2), zeroed after a full-range calibration so
    the live rows keep full-range values and the states are not trivially small."""
    dims = _dims(ds)
    md, qc = _calibrate(dims, FULL, headroom=5)
    _kill_states(md, dims, n_live)
    return Case(f"F4_live{n_live}_ds{ds}", md, qc, dims, family="F4", n_live=n_live)


def f5_pk16(ds: float, y_up: int, l_minus_y: Optional[int] = None) -> Case:
    """y_exp raised by y_up (the full-range recipe leaves |cx| below 2^13: it takes 3 or 4 more bits before 2 cx leaves int16) (out2's input exponent with it, so that the gate kernel converts nothing: a PK16 condition), and
    optionally l_exp = y_exp + l_minus_y."""
    dims = _dims(ds)
    md, qc = _calibrate(dims, FULL, headroom=6)
    b = qc["blocks"]
    b["ssm"]["activations"]["y"]["exp"] += y_up
    ye = b["ssm"]["activations"]["y"]["exp"]
    b["out2"]["inp_exp"] = max(b["out2"]["inp_exp"], ye)
    b["out2"]["out_exp"] = max(b["out2"]["out_exp"], 6)
    w, a = b["ssm"]["weights"], b["ssm"]["activations"]
    assert ye <= min(a["x_re"]["exp"] + w["C_re"]["exp"], a["x_im"]["exp"] + w["C_im"]["exp"], w["D"]["exp"] + a["u"]["exp"])
    if l_minus_y is not None:   # the gate product keeps its right shift l_exp + r_exp - res_exp
        mg = b["multgate"]
        mg["res_exp"] += ye + l_minus_y - mg["l_exp"]
        mg["l_exp"] = ye + l_minus_y
    tag = f"F5_y+{y_up}" + (f"_l-y{l_minus_y}" if l_minus_y is not None else "")
    return Case(f"{tag}_ds{ds}", md, qc, dims, family="F5", y_up=y_up, l_minus_y=l_minus_y)


# the live counts of F4 at P = 64 / 128 (every boundary of the compaction rules: 0, 1, odd, 32 / 33, P/2 - 1, P/2, P/2 + 1, P)
def live_counts(P: int) -> List[int]:
    return sorted({0, 1, 2, 3, 31, 32, 33, P // 2 - 1, P // 2, P // 2 + 1, P})


BUILDERS = {}
for _ds in (0.5, 1.0):
    BUILDERS[f"F1_full_ds{_ds}"] = (f1_full_range, (_ds,))
    BUILDERS[f"F2_rails_ds{_ds}"] = (f2_rails, (_ds,))
    BUILDERS[f"F3_D16_ds{_ds}"] = (f3_wide_D, (_ds,))
    BUILDERS[f"F3_Bu24_ds{_ds}"] = (f3_wide_bu, (_ds,))
    BUILDERS[f"F3_out32_ds{_ds}"] = (f3_wide_out, (_ds,))
    for _n in live_counts(synth.ndns_dims(_ds)["P"]):
        BUILDERS[f"F4_live{_n}_ds{_ds}"] = (f4_live, (_ds, _n))
    BUILDERS[f"F5_y+4_ds{_ds}"] = (f5_pk16, (_ds, 4))
    BUILDERS[f"F5_y+3_l-y14_ds{_ds}"] = (f5_pk16, (_ds, 3, 14))
    BUILDERS[f"F5_y+3_l-y15_ds{_ds}"] = (f5_pk16, (_ds, 3, 15))   # one past the PK16 limit: the boundary pair
for _di, _do in ((257, 1), (288, 257), (257, 272)):   # d_out > 272 is refused at creation (s5fxp_api.hip validate)
    BUILDERS[f"F3_dims{_di}x{_do}_ds0.5"] = (f3_dims, (_di, _do))

_CACHE: Dict[str, Case] = {}


def case(name: str) -> Case:
    """The contract model `name` (built once per process)."""
    if name not in _CACHE:
        fn, args = BUILDERS[name]
        _CACHE[name] = fn(*args)
    return _CACHE[name]


# --------------------------------------------------------------------------------------------------------------------
# inputs (integer, at the encoder's input format: every route gets the same int32 array)
# --------------------------------------------------------------------------------------------------------------------
INPUTS = ("zeros", "pos_full", "neg_full", "flip", "impulse_first", "impulse_last", "mixed", "ndns")


def make_input(kind: str, B: int, L: int, d_in: int, bits: int, seed: int = 0) -> np.ndarray:
    hi, lo = (1 << (bits - 1)) - 1, -(1 << (bits - 1))
    x = np.zeros((B, L, d_in), dtype=np.int32)
    if kind == "zeros":
        pass
    elif kind == "pos_full":
        x[:] = hi
    elif kind == "neg_full":
        x[:] = lo
    elif kind == "flip":     # full scale with a sign flip every frame (and across channels, so the encoder sees both)
        t = np.arange(L)[None, :, None]
        c = np.arange(d_in)[None, None, :]
        x[:] = np.where((t + c) % 2 == 0, hi, lo)
    elif kind in ("impulse_first", "impulse_last"):
        t = 0 if kind == "impulse_first" else L - 1
        rng = np.random.Generator(np.random.PCG64(seed))
        x[:, t, :] = np.where(rng.random((B, d_in)) < 0.5, hi, lo)
    elif kind == "mixed":    # one sequence at full scale, the others all zero
        x[0] = hi
    elif kind == "ndns":     # the recipe's own input, for reference
        xf = synth.make_input(B, L, d_in, seed=seed)
        return O.from_fp(xf, bits, 14, True, O.FLOOR).data
    else:
        raise ValueError(kind)
    return x


def input_for(c: Case, kind: str, B: int, L: int, seed: int = 0):
    """(int32 data, bits, exp) of input `kind` for case c."""
    if kind == "ndns":
        xf = synth.make_input(B, L, c.dims["d_in"], seed=seed)
        return O.from_fp(xf, c.in_bits, c.in_exp, True, O.FLOOR).data, c.in_bits, c.in_exp
    return make_input(kind, B, L, c.dims["d_in"], c.in_bits, seed), c.in_bits, c.in_exp


# --------------------------------------------------------------------------------------------------------------------
# what an export says about the fused path (restatements of the host rules, for the tests' expectations)
# --------------------------------------------------------------------------------------------------------------------
def export_live(export: dict, n_layers: int) -> List[np.ndarray]:
    """Indices of the live states of each layer: a row of B_real or B_imag with a nonzero entry
    (s5fxp_fast.hpp pack_fast; include/s5fxp.h s5fxp_model_live_states)."""
    ex = export["params"]["encoder"]
    return [np.flatnonzero((np.asarray(ex[f"layers_{i}"]["mixer"]["B_real"]) != 0).any(axis=1) |
                           (np.asarray(ex[f"layers_{i}"]["mixer"]["B_imag"]) != 0).any(axis=1)) for i in range(n_layers)]


def compact_slots(n_live: int, P: int) -> int:
    """State slots of a layer on an untraced carry-free forward: Pc = max(32, ceil32(n_live)) when Pc <= P / 2, else P."""
    pc = max(32, (n_live + 31) // 32 * 32)
    return pc if pc <= P // 2 else P


def stream_slots(n_live: int, P: int, int16_rung: bool) -> int:
    """State slots the recurrence streams keep (s5fxp_fast.hpp stream_live_slots): on the int16 rungs of a compacted layer,
    whole live state pairs (at least one)."""
    w = compact_slots(n_live, P)
    if not int16_rung or w == P:
        return w
    n = max(2, 2 * ((n_live + 1) // 2))
    return n if n < w else w


def copy_case(c: Case, name: str) -> Case:
    return Case(name, copy.deepcopy(c.md), copy.deepcopy(c.qc), dict(c.dims), **dict(c.meta))
