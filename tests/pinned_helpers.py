"""Helpers of tests/test_pinned_exps.py, tests/test_forward_at.py and tests/test_pinned_box.py: the NumPy oracle
(oracle/fxp_oracle.py) run at STATED exponents through its MAX_EXCHANGE hook, a host restatement of which exponent sets leave
every static shift inside 0..31, and of which arm of the B projection's row chain a set puts on a layer.

The hook sees every compute_best op's float32 maxima in the order the model runs them: per layer BatchNorm add(-mean),
mul(invsq_var), [mul(scale)], [add(bias)], then the residual add.  Forcing op k's maximum to a float whose intbits is
ib = result_bits - 1 - e makes the oracle choose the exponent e for it: 0.5 for ib = 0, 1.5 * 2^(ib - 1) otherwise (the add's
other two maxima only size the operands' widening, which never clips, so forcing them too changes nothing).
"""
import contextlib

import numpy as np

from oracle import fxp_oracle as O

F32 = np.float32


def op_bits(om) -> np.ndarray:
    """(n_layers, 5) result bits of the five compute_best ops of every layer, 0 where the layer has no such op."""
    out = np.zeros((len(om.layers), 5), dtype=np.int32)
    hb = om.encoder.qc["out_bits"]
    for i, l in enumerate(om.layers):
        n = l.norm
        b1 = max(hb, n.minus_mean.bits)
        b2 = max(b1, n.invsq_var.bits)
        b3 = max(b2, n.scale.bits) if n.scale is not None else b2
        b4 = max(b3, n.bias.bits) if n.bias is not None else b3
        rb = l.qc["multgate"]["res_bits"]
        out[i] = (b1, b2, b3 if n.scale is not None else 0, b4 if n.bias is not None else 0, rb)
        hb = rb
    return out


def exp_max(om) -> np.ndarray:
    """What Engine.exp_max() must report: result bits - 1, -1 for an absent op."""
    return op_bits(om) - 1


def forced_float(ib: int) -> np.float32:
    return F32(0.5) if ib == 0 else F32(1.5 * 2.0 ** (ib - 1))


class _Hook:
    """MAX_EXCHANGE callable: records the exponent every op would choose on its own and, with `exps`, forces the stated one.
    The ops of one forward come in a fixed order, so a call counter modulo the ops per forward names the op."""

    def __init__(self, om, exps=None):
        bits = op_bits(om)
        self.slots = [(l, k) for l in range(bits.shape[0]) for k in range(5) if bits[l, k] > 0]
        self.bits, self.exps, self.calls = bits, None if exps is None else np.asarray(exps), 0
        self.natural = []   # one (n_layers, 5) array per forward

    def __call__(self, v):
        l, k = self.slots[self.calls % len(self.slots)]
        if self.calls % len(self.slots) == 0:
            self.natural.append(np.zeros_like(self.bits))
        self.calls += 1
        self.natural[-1][l, k] = self.bits[l, k] - 1 - O.intbits_f32(v[0], 1e-6)
        if self.exps is None:
            return v
        ib = int(self.bits[l, k]) - 1 - int(self.exps[l, k])
        assert ib >= 0, (l, k, self.exps[l, k])
        return np.full_like(v, forced_float(ib))


@contextlib.contextmanager
def hooked(om, exps=None):
    h, old = _Hook(om, exps), O.MAX_EXCHANGE
    O.MAX_EXCHANGE = h
    try:
        yield h
    finally:
        O.MAX_EXCHANGE = old


def oracle_run(om, clip, bits, exp, exps=None, chunks=None, state=None):
    """clip (L, d_in) int32 through the oracle as the chunks `chunks` (default: one) with the carry handed on, at the stated
    `exps` (None: each chunk's own).  state: (n_layers, 2, P) carry in or None (zeros).
    Returns (y (L, d_out), carry out (n_layers, 2, P), the exponents each chunk would have chosen / was given)."""
    L = clip.shape[0]
    chunks = [L] if chunks is None else list(chunks)
    assert sum(chunks) == L
    st = om.zero_state((1,))
    if state is not None:
        for i in range(len(st)):
            st[i][0], st[i][1] = state[i, 0][None].astype(np.int32).copy(), state[i, 1][None].astype(np.int32).copy()
    ys, at = [], 0
    with hooked(om, exps) as h:
        for c in chunks:
            if c:
                ys.append(om(O.Fx(clip[None, at:at + c], bits, exp, True), state=st).data[0])
            at += c
    y = np.concatenate(ys, axis=0) if ys else np.zeros((0, om.decoder.weight.data.shape[1]), dtype=np.int32)
    carry = np.stack([np.stack([s[0][0], s[1][0]]) for s in st]).astype(np.int32)
    return y, carry, (h.natural if exps is None else [np.asarray(exps)] * len(h.natural))


def forced_run(om, clip, bits, exp, exps):
    """oracle_run for one chunk from a zero carry, with what tests/test_pinned_box.py asks of the pool beside it: returns
    (y, carry out, the (n_layers, 5) exponents every op WOULD have chosen at that point of the forced run)."""
    st = om.zero_state((1,))
    with hooked(om, exps) as h:
        y = om(O.Fx(clip[None], bits, exp, True), state=st).data[0]
    carry = np.stack([np.stack([s[0][0], s[1][0]]) for s in st]).astype(np.int32)
    return y, carry, h.natural[0]


def shifts_ok(om, exps) -> bool:
    """The host rule of s5fxp_model_exps_check for the static shifts, restated from the ops' definitions: an add's two operand
    shifts and its result shift (fxparray.py:420-448), a mul's right shift (fxparray.py:619-621), the change_cfg to the SSM
    input, the decoder's input conversion and right shift."""
    e = np.asarray(exps)

    def add_ok(eo, xe, ye):
        ea = max(xe, ye)
        return ea - xe <= 31 and ea - ye <= 31 and -31 <= eo - ea <= 31

    hb, he = om.encoder.qc["out_bits"], om.encoder.qc["out_exp"]
    for i, l in enumerate(om.layers):
        n = l.norm
        if not add_ok(e[i, 0], he, n.minus_mean.exp) or not 0 <= e[i, 0] + n.invsq_var.exp - e[i, 1] <= 31:
            return False
        be = e[i, 1]
        if n.scale is not None:
            if not 0 <= be + n.scale.exp - e[i, 2] <= 31:
                return False
            be = e[i, 2]
        if n.bias is not None:
            if not add_ok(e[i, 3], be, n.bias.exp):
                return False
            be = e[i, 3]
        if abs(int(be) - l.mixer.qc["activations"]["u"]["exp"]) > 31:
            return False
        if not add_ok(e[i, 4], l.qc["multgate"]["res_exp"], he):
            return False
        hb, he = l.qc["multgate"]["res_bits"], e[i, 4]
    d = om.decoder.qc
    conv = hb > d["inp_bits"] or he > d["inp_exp"]
    if conv and abs(int(he) - d["inp_exp"]) > 31:
        return False
    return 0 <= (d["inp_exp"] if conv else he) + d["w_exp"] - d["out_exp"] <= 31


ROW_GENERIC, ROW_PACKED, ROW_SHIFTED = 0, 1, 2
ARM_NAMES = {ROW_GENERIC: "ROW_GENERIC", ROW_PACKED: "ROW_PACKED", ROW_SHIFTED: "ROW_SHIFTED"}


def row_arms(om, exps) -> list:
    """Per layer the arm of mfma_bn.hpp bn16_row_arm at the stated exponents, None for a layer with a BatchNorm scale or bias
    (no row chain).  The rule restated: the packed forms need every width at 16 bits, the input shift shx1 <= 14, no left
    shift of the sum (l1 == 0) and the change_cfg to the SSM input within cl <= 14 / cr <= 15; PACKED is r1 == 0, SHIFTED
    r1 >= 1, everything else GENERIC.  shx1, l1 and r1 are the first add's shifts (pinned_exps.hpp pinned_add_cb: the layer
    input's exponent against the mean's, then the stated result exponent against their maximum), cl / cr the distance from the
    second op's exponent to the SSM input's."""
    e = np.asarray(exps)
    xb, xe = om.encoder.qc["out_bits"], om.encoder.qc["out_exp"]
    arms = []
    for i, l in enumerate(om.layers):
        n, u = l.norm, l.mixer.qc["activations"]["u"]
        if n.scale is not None or n.bias is not None:
            arms.append(None)
        else:
            mb, ib = n.minus_mean.bits, n.invsq_var.bits
            b1 = max(xb, mb)
            b2 = max(b1, ib)
            ea = max(xe, n.minus_mean.exp)
            shx1, post, de = ea - xe, int(e[i, 0]) - ea, u["exp"] - int(e[i, 1])
            l1, r1, cl, cr = max(post, 0), max(-post, 0), max(de, 0), max(-de, 0)
            w16 = ((xb == 16 or (shx1 == 0 and xb < 16)) and mb <= 16 and ib <= 16 and b1 == 16 and b2 == 16 and
                   min(b2, u["bits"]) == 16 and shx1 <= 14 and l1 == 0 and cl <= 14 and cr <= 15)
            arms.append(ROW_GENERIC if not w16 else ROW_PACKED if r1 == 0 else ROW_SHIFTED)
        xb, xe = l.qc["multgate"]["res_bits"], int(e[i, 4])
    return arms


def add_posts(om, exps) -> list:
    """The result shift (pinned_exps.hpp pinned_add_cb: post = eo - max(xe, ye)) of every add at the stated exponents, in model
    order: per layer the add of -mean, the add of the bias where the layer has one, the residual add."""
    e = np.asarray(exps)
    out, he = [], om.encoder.qc["out_exp"]
    for i, l in enumerate(om.layers):
        n = l.norm
        out.append(int(e[i, 0]) - max(he, n.minus_mean.exp))
        if n.bias is not None:
            out.append(int(e[i, 3]) - max(int(e[i, 2 if n.scale is not None else 1]), n.bias.exp))
        out.append(int(e[i, 4]) - max(l.qc["multgate"]["res_exp"], he))
        he = int(e[i, 4])
    return out


def corner(om, base, delta: int) -> np.ndarray:
    """`base` moved by `delta` (+1 / -1) per op, again and again, until no op can move: shifted()'s greedy rule to its end."""
    e = np.asarray(base, dtype=np.int32)
    while True:
        nxt = shifted(om, e, delta)
        if np.array_equal(nxt, e):
            return e
        e = nxt


def shifted(om, base, delta: int) -> np.ndarray:
    """`base` with every op moved by `delta` where that is legal: inside 0 .. exp_max and with every static shift in range.
    Ops are moved one after the other, in model order, and an op whose move breaks a shift keeps its value."""
    mx, e = exp_max(om), np.asarray(base, dtype=np.int32).copy()
    for l in range(e.shape[0]):
        for k in range(5):
            if mx[l, k] < 0:
                continue
            old = e[l, k]
            e[l, k] = min(max(old + delta, 0), mx[l, k])
            if not shifts_ok(om, e):
                e[l, k] = old
    return e
