"""The fast recurrence kernels at their exactness bound, and on carries beyond it.

csrc/scan_quad.hpp: the quad and pair kernels multiply with 24-bit multiply-adds and are exact only while |state| <= xmax.  The
consumer of the states (the gate kernel; k_cproj on the generic path) checks that bound on every STORED state, the recurrence
kernels check it on the state they START from (the streaming carry, s5fxp_forward_opts::state_in), and by induction over t every
product was exact.  When a check fires a default forward runs its exact 32-bit kernels (LayerDyn::redo) and a
S5FXP_FWD_DEFER_REDO forward reports S5FXP_ST_REDO.  Two things are tested here, bit for bit against
oracle.cref.CModel.forward(..., trace=True, state=...):

  A. carries wider than the bound (which the exact kernels, s5fxp_model_step and the exact re-run of a loud chunk all leave
     behind legitimately) are never silently wrong, on every rung, in every layer;
  B. one state placed exactly at T - 1, T and T + 1, T being the value the rung's check compares with: no false
     S5FXP_ST_REDO at |state| == T, no missed one at T + 1, in the first, the last and the bound-setting qualifying state, in
     the first and the last sequence, in ragged 4- and 8-step blocks and where the extreme is the last frame (L = 1).

T per rung: the pair kernels check s5fxp_model_recurrence_xmax; quad16 (DEFER_REDO | NO_PAIR) min(that query under
S5FXP_NO_PAIR, 32766); the default forward's quad32 min(quad bound, 32767); the generic path's quad kernel its quad bound.
Engines are created with S5FXP_NO_COMPACT=1 so that the query answers for the slots a forward with a carry runs on.
"""
import functools

import numpy as np
import pytest

from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth

gpu = pytest.mark.gpu

B = 2
LS = (1, 5, 37)           # 5: a ragged 4-step block; 37: a ragged 8-step block (the pair kernels' item)
DIM_SCALES = (0.25, 0.5, 0.75, 1.0)
GENERIC = "generic"       # P = 16 states, 24-bit operands: the generic path's quad kernel
MODELS = DIM_SCALES + (GENERIC,)
ST_WIDE_STATE, ST_REDO = 4, 16
DEFER, EXACT, NO_PAIR = 1, 2, 4
RK_QUAD32, RK_QUAD16, RK_PAIR, RK_PAIRL, RK_EXACT = 1, 2, 3, 4, 5

# engines: every one with S5FXP_NO_COMPACT (see above); the switches are read once, by s5fxp_model_create
SWITCHES = {
    "default": {},
    "pair_global": {"S5FXP_PAIR_GLOBAL": "1"},
    "pairl_blocks16": {"S5FXP_PAIRL_BLOCKS": "16"},
    "no_pair": {"S5FXP_NO_PAIR": "1"},
}
# DEFER_REDO rungs of a fused model: (engine, forward flags, status code [8 + 8l + 5], which T)
DEFER_RUNGS = {
    "pairl": ("default", DEFER, RK_PAIRL, "pair"),
    "pair_global": ("pair_global", DEFER, RK_PAIR, "pair"),
    "pairl_blocks16": ("pairl_blocks16", DEFER, RK_PAIRL, "pair"),
    "quad16": ("default", DEFER | NO_PAIR, RK_QUAD16, "quad16"),
}


# ------------------------------------------------------------------------------------------------------------------
# models, inputs, oracle runs (no GPU)
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(name):
    from sparsernns_amd.fxpmodel import build_regression_model
    if name == GENERIC:
        md, qc, dims = synth.make_model(dims=synth.tiny_dims(H=32, P=16, d_in=5, d_out=30, n_layers=2), calib_L=64)
    else:
        md, qc, dims = synth.make_model(dim_scale=name, calib_L=256, state_headroom_bits=1)
    export = build_regression_model(md, qc, dims["n_layers"]).export()
    return qc, dims, export, cref.CModel(export)


def _mixer(name, l):
    _, _, export, _ = _model(name)
    m = export["params"]["encoder"][f"layers_{l}"]["mixer"]
    q = export["qconfig"]["encoder"][f"layers_{l}"]["mixer"]
    a_re, a_im = np.asarray(m["A_real"]).astype(np.int64), np.asarray(m["A_imag"]).astype(np.int64)
    return a_re, a_im, int(q["A_real_exp"]), int(q["A_imag_exp"]), m


@functools.lru_cache(maxsize=None)
def _base(name, L):
    """The input of every case at (model, L) and the oracle's run from a zero carry."""
    qc, dims, _, cm = _model(name)
    xf = synth.make_input(B, L, dims["d_in"], seed=700 + L, scale=0.25)
    fx = O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    state = np.zeros((dims["n_layers"], 2, B, dims["P"]), dtype=np.int32)
    y0, _, ye, tr0 = cm.forward(fx.data, fx.bits, fx.exp, trace=True, state=state)
    for a in (xf, fx.data, y0):
        a.setflags(write=False)
    return dict(xf=xf, x=fx.data, bits=fx.bits, exp=fx.exp, y0=y0, ye=ye, tr0=tr0, L=L, name=name)


def _oracle(name, L, state):
    """The oracle's run from `state` (not modified): y, carry out, max |stored state| per layer, the traces."""
    _, _, _, cm = _model(name)
    base = _base(name, L)
    st = np.ascontiguousarray(state, dtype=np.int32).copy()
    y, _, _, tr = cm.forward(base["x"], base["bits"], base["exp"], trace=True, state=st)
    tops = [max(int(np.abs(t["xs_re"].astype(np.int64)).max()), int(np.abs(t["xs_im"].astype(np.int64)).max())) for t in tr]
    return y, st, tops, tr


def _quad_bound(name, l):
    """scan_quad.hpp: |c * x| + 2^16 < 2^31 with c = A * 2^(16 - e), i.e. scan_bounds()'s quad_xmax."""
    a_re, a_im, e_re, e_im, _ = _mixer(name, l)
    cmax = max(1, int(max(np.abs(a_re).max(), np.abs(a_im).max())) << max(16 - e_re, 16 - e_im))
    return min((2 ** 31 - 1 - 65536) // cmax, 2 ** 23 - 1)


def _criterion(name, l):
    """States whose first step can be driven to the bound from a carry inside it: |A_re| + |A_im| > 1.05 * 2^e."""
    a_re, a_im, e_re, e_im, _ = _mixer(name, l)
    assert e_re == e_im
    return [int(q) for q in np.flatnonzero(np.abs(a_re) + np.abs(a_im) > 1.05 * 2 ** e_re)]


@functools.lru_cache(maxsize=None)
def _qualifying(name, l, T):
    """The states section B plants in: of those that meet the criterion, the ones whose planted trajectory peaks at its first
    step for every sequence, component, sign, target and L used here (_holds: a fast-rotating state, |A_im| well above |A_re|,
    turns the carry's other component into a larger one a few steps later, and its maximum is then not the planted value).
    Returns the bound-setting one (largest max(|A_re|, |A_im|)), the first and the last, without repeats."""
    a_re, a_im, _, _, _ = _mixer(name, l)
    q = _criterion(name, l)
    first = lambda order: next((p for p in order if _holds(name, l, p, T)), None)   # lazily: _holds walks 72 trajectories
    by_size = sorted(q, key=lambda p: -max(abs(int(a_re[p])), abs(int(a_im[p]))))   # stable: the lowest index among equals
    picks = [first(by_size), first(q), first(reversed(q))]
    return tuple(dict.fromkeys(p for p in picks if p is not None))


def _dead_states(name, l):
    m = _mixer(name, l)[4]
    return np.flatnonzero(~((np.asarray(m["B_real"]) != 0).any(axis=1) | (np.asarray(m["B_imag"]) != 0).any(axis=1)))


@functools.lru_cache(maxsize=None)
def _zero_run(name, L, l):
    """Of the oracle's zero-carry run of layer l: its states as Python-int friendly arrays and max |state| per (b, p)."""
    t0 = _base(name, L)["tr0"][l]
    re, im = t0["xs_re"].astype(np.int64), t0["xs_im"].astype(np.int64)
    return re, im, np.maximum(np.abs(re).max(axis=1), np.abs(im).max(axis=1))


def _step(ar, ai, e_re, e_im, xr, xi):
    """The reference step without its Bu term (sparseRNNs/fxpmodel.py:155-169), on Python ints."""
    return ((ar * xr) >> e_re) - ((ai * xi) >> e_re), ((ar * xi) >> e_im) + ((ai * xr) >> e_im)


def plant_at_bound(name, L, l, p, b, comp, s, T, target):
    """A carry for layer l, zero except state (b, p), from which the oracle's first stored state of component `comp` of (b, p)
    is s * target: the component's own carry is s * sign(A_re) * T, the other one's is found by bisection over 0 .. T on the
    reference step (the layer's input does not depend on its own carry, so the step's Bu terms are those of the oracle's
    zero-carry run).  Both carry components stay within T, so the carry itself is legitimate and |c| * T is the worst product
    the bound allows.  Returns (state, w, the largest |state| the layer will store) or None when no w in 0 .. T hits the target."""
    _, dims, _, _ = _model(name)
    a_re, a_im, e_re, e_im, _ = _mixer(name, l)
    ar, ai = int(a_re[p]), int(a_im[p])
    zre, zim, zmax = _zero_run(name, L, l)
    # Bu_t at the state exponent = (zero-carry state t) - step(zero-carry state t - 1)
    bu = []
    for t in range(L):
        pr, pi = (int(zre[b, t - 1, p]), int(zim[b, t - 1, p])) if t else (0, 0)
        sr, si = _step(ar, ai, e_re, e_im, pr, pi)
        bu.append((int(zre[b, t, p]) - sr, int(zim[b, t, p]) - si))
    sg = lambda v: (v > 0) - (v < 0)

    def carry(w):
        return (s * sg(ar) * T, -s * sg(ai) * w) if comp == "re" else (s * sg(ai) * w, s * sg(ar) * T)

    def first(w):   # s * (the component after the first step), non-decreasing in w by at most 1 per step of w
        sr, si = _step(ar, ai, e_re, e_im, *carry(w))
        return s * ((sr + bu[0][0]) if comp == "re" else (si + bu[0][1]))

    lo, hi = 0, T
    if first(lo) > target or first(hi) < target:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if first(mid) < target:
            lo = mid + 1
        else:
            hi = mid
    if first(lo) != target:
        return None
    state = np.zeros((dims["n_layers"], 2, B, dims["P"]), dtype=np.int32)
    state[l, 0, b, p], state[l, 1, b, p] = carry(lo)
    others = zmax.copy()
    others[b, p] = 0
    top, (xr, xi) = int(others.max()), carry(lo)
    for t in range(L):
        sr, si = _step(ar, ai, e_re, e_im, xr, xi)
        xr, xi = sr + bu[t][0], si + bu[t][1]
        top = max(top, abs(xr), abs(xi))
    return state, lo, top


@functools.lru_cache(maxsize=None)
def _holds(name, l, p, T):
    for L in LS:
        for b in (0, B - 1):
            for comp in ("re", "im"):
                for s in (1, -1):
                    for target in (T - 1, T, T + 1):
                        got = plant_at_bound(name, L, l, p, b, comp, s, T, target)
                        if got is None or got[2] != target:
                            return False
    return True


def _planted(name, L, l, p, b, comp, s, T, target):
    """plant_at_bound + the oracle's run from it, with the construction asserted on the oracle: the carry is within T, the hit
    is exact and it is the largest |state| the layer stores anywhere."""
    got = plant_at_bound(name, L, l, p, b, comp, s, T, target)
    tag = (name, L, l, p, b, comp, s, T, target)
    assert got is not None, ("no carry within T reaches the target", tag)
    state, w, _ = got
    assert int(np.abs(state).max()) <= T, tag
    y, out, tops, tr = _oracle(name, L, state)
    hit = int(tr[l]["xs_re" if comp == "re" else "xs_im"][b, 0, p])
    assert hit == s * target, ("missed", tag, hit)
    assert tops[l] == target, ("the planted state is not the layer's largest", tag, tops)
    return state, y, out, tops


def _bound_cases(name, l, T):
    return [(p, b, comp, s) for p in _qualifying(name, l, T) for b in (0, B - 1) for comp in ("re", "im") for s in (1, -1)]


# ------------------------------------------------------------------------------------------------------------------
# C. the construction itself, wherever the suite runs
# ------------------------------------------------------------------------------------------------------------------
def test_planting_hits_the_target_on_the_oracle():
    """Without a GPU, for T in {16544, 32766, 32767}: for every model, layer, planted state (bound-setting, first, last),
    sequence, component and sign, and for targets T - 1, T, T + 1, the planted carry stays within T, the oracle's first stored
    state is exactly the target and nothing else the layer stores is larger.  T = 16544 stands for the pair kernels' bounds
    (16.5k - 17.0k on these models), 32766 and 32767 are the quad thresholds.  Fails if the helper misses by one anywhere: the
    GPU tests of section B would then test another value than the bound."""
    L = 5
    for T in (16544, 32766, 32767):
        n = 0
        for name in MODELS:
            _, dims, _, _ = _model(name)
            for l in range(dims["n_layers"]):
                cases = _bound_cases(name, l, T)
                assert len(cases) >= 16, (T, name, l, "fewer than two states to plant in")
                for (p, b, comp, s) in cases:
                    for target in (T - 1, T, T + 1):
                        _planted(name, L, l, p, b, comp, s, T, target)
                        n += 1
        assert n >= (4 * 3 + 2) * 16 * 3


# ------------------------------------------------------------------------------------------------------------------
# GPU side: engines, thresholds, forwards
# ------------------------------------------------------------------------------------------------------------------
_ENGINES, _DEV = {}, {}


def _engine(name, switch, monkeypatch):
    from sparsernns_amd.engine import Engine
    if (name, switch) not in _ENGINES:
        env = dict(SWITCHES[switch], S5FXP_NO_COMPACT="1")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            _ENGINES[(name, switch)] = Engine(_model(name)[2])
        finally:
            for k in env:
                monkeypatch.delenv(k)
    return _ENGINES[(name, switch)]


def _thresholds(name, monkeypatch):
    """Per layer, the value each rung's check compares with (module docstring), with the queries and the recurrence kernels
    they answer for asserted."""
    from sparsernns_amd import _lib
    lib = _lib.lib
    nl = _model(name)[1]["n_layers"]
    if name == GENERIC:
        eng = _engine(name, "default", monkeypatch)
        assert lib.s5fxp_model_is_fast(eng._h) == 0
        out = []
        for l in range(nl):
            assert lib.s5fxp_model_recurrence_kernel(eng._h, l) == RK_QUAD32
            t = lib.s5fxp_model_recurrence_xmax(eng._h, l)
            assert t == _quad_bound(name, l), (l, t)
            out.append(dict(generic=t))
        return out
    e = {k: _engine(name, k, monkeypatch) for k in SWITCHES}
    out = []
    for l in range(nl):
        codes = {k: lib.s5fxp_model_recurrence_kernel(e[k]._h, l) for k in SWITCHES}
        assert codes == dict(default=RK_PAIRL, pair_global=RK_PAIR, pairl_blocks16=RK_PAIRL, no_pair=RK_QUAD16), (name, l, codes)
        tp = lib.s5fxp_model_recurrence_xmax(e["default"]._h, l)
        assert tp == lib.s5fxp_model_recurrence_xmax(e["pair_global"]._h, l) == lib.s5fxp_model_recurrence_xmax(e["pairl_blocks16"]._h, l)
        tq, qb = lib.s5fxp_model_recurrence_xmax(e["no_pair"]._h, l), _quad_bound(name, l)
        assert tq == min(qb, 32766) and 16384 <= tp <= tq, (name, l, tp, tq, qb)
        out.append(dict(pair=tp, quad16=min(tq, 32766), quad32=min(qb, 32767)))
    return out


def _dev(name, L):
    import torch
    if (name, L) not in _DEV:
        base = _base(name, L)
        _DEV[(name, L)] = (torch.from_numpy(base["x"].copy()).cuda(), torch.from_numpy(base["xf"].copy()).cuda())
    return _DEV[(name, L)]


def _run(eng, name, L, flags, state, f32=False):
    """One enqueue from `state`: y (float entry: converted back to the integers), carry out, status words."""
    import torch
    base = _base(name, L)
    x = _dev(name, L)[1 if f32 else 0]
    y = torch.empty((B, L, eng.d_out), dtype=x.dtype, device="cuda")
    sin = torch.from_numpy(state).cuda()
    sout = torch.zeros_like(sin)
    eng.enqueue(x, base["bits"], base["exp"], y, B, L, flags=flags, state_in=sin, state_out=sout)
    st = eng.check_status()
    assert np.array_equal(sin.cpu().numpy(), state), "state_in was written"
    y = y.cpu().numpy()
    if f32:
        yi = np.ldexp(y.astype(np.float64), eng.out_exp)
        assert np.array_equal(yi, np.rint(yi))
        y = yi.astype(np.int64).astype(np.int32)
    return y, sout.cpu().numpy(), st


def _ladder(eng, name, L, state):
    """Engine.forward_chunk from `state`, from the ladder's first rung."""
    import torch
    from sparsernns_amd.fxparray import FxpArray
    base = _base(name, L)
    eng.level, eng._redos = 0, [0, 0]
    y, new = eng.forward_chunk(FxpArray(_dev(name, L)[0], base["bits"], base["exp"]), torch.from_numpy(state).cuda())
    return y.numpy(), new.cpu().numpy()


def _diff(got, ref):
    """(mismatches in y, mismatches in the carry out)"""
    return int(np.count_nonzero(got[0] != ref[0])), int(np.count_nonzero(got[1] != ref[1]))


def _codes(st, nl):
    return [int(st[8 + 8 * i + 5]) for i in range(nl)]


# ------------------------------------------------------------------------------------------------------------------
# A. wide carries
# ------------------------------------------------------------------------------------------------------------------
def _wide_carries(name, l, Ts, rng):
    """(label, carry of layer l (2, B, P)) for every class of wide carry; Ts: the layer's thresholds."""
    P = _model(name)[1]["P"]
    shape = (2, B, P)
    sign = lambda: rng.choice(np.array([-1, 1], dtype=np.int64), shape)
    out = [("uniform", sign() * rng.integers(min(Ts) + 1, 65536, shape)),
           ("wrap24", sign() * (2 ** 24 + rng.integers(0, 8, shape))),
           ("bits27", rng.integers(-2 ** 26, 2 ** 26, shape))]
    # one value just beyond each threshold, in the last slot of all; positive: the complex ReLU drops a state whose real
    # part is negative, and y would not move
    for k, T in enumerate(sorted(set(Ts))):
        c = np.zeros(shape, dtype=np.int64)
        c[k % 2, B - 1, P - 1] = T + 1
        out.append((f"single_{T + 1}", c))
    dead = _dead_states(name, l)
    if name in (0.5, 1.0):
        assert dead.size, (name, l, "no all-zero B_bar row")
    if dead.size:
        m = _mixer(name, l)[4]
        p = int(dead[-1])
        assert not np.asarray(m["B_real"])[p].any() and not np.asarray(m["B_imag"])[p].any()
        c = np.zeros(shape, dtype=np.int64)
        c[0, B - 1, p], c[1, B - 1, p] = 40000, -50000
        out.append(("dead", c))
    return [(k, v.astype(np.int32)) for k, v in out]


@gpu
@pytest.mark.parametrize("name", MODELS)
def test_wide_carries_are_never_silently_wrong(name, monkeypatch):
    """A carry beyond the rung's threshold T, planted in one layer at a time: uniform in +-[T + 1, 65535] (wrapped products,
    first state back in range), +-(2^24 + r) (multiplied as r by a 24-bit multiply), 27-bit values, one value of T + 1 in the
    last (b, p) slot, and a wide value on a dead state (all-zero B_bar row: nothing but the carry ever moves it).  The default
    and EXACT forwards, the float entry and Engine.forward_chunk must give the oracle's y and carry out; every DEFER_REDO rung
    (LDS-fed pair kernel with 32- and 16-block buffers, pair kernel from global memory, quad16) must report S5FXP_ST_REDO
    where |x0| > T and otherwise either report it or match; state_in is never written.  The generic model runs its quad kernel
    (it has no DEFER_REDO: every forward must match).

    Fails without the range check of the carry (scan_quad.hpp CarryCheck): the stored states of a wrapped first step are in
    range, nothing re-runs, y and the carry out differ from the oracle's and no DEFER_REDO forward reports S5FXP_ST_REDO.  The
    single_<T + 1> cases fail if the carry check compares with T + 1 or more; a check against less than T is caught by
    test_a_state_exactly_at_the_bound, whose carries sit at T.  On the commit before the check this test failed at all five
    models (DESIGN.md 5b has the counts)."""
    from sparsernns_amd import _lib
    nl = _model(name)[1]["n_layers"]
    thr = _thresholds(name, monkeypatch)
    eng = _engine(name, "default", monkeypatch)
    fused = name != GENERIC
    rungs = {k: (_engine(name, v[0], monkeypatch),) + v[1:] for k, v in DEFER_RUNGS.items()} if fused else {}
    rng = np.random.Generator(np.random.PCG64(2024))
    bad, n = [], 0
    for L in LS:
        y0 = _base(name, L)["y0"]
        for l in range(nl):
            Ts = list(thr[l].values())
            for label, c in _wide_carries(name, l, Ts, rng):
                state = np.zeros((nl, 2, B, c.shape[-1]), dtype=np.int32)
                state[l] = c
                tag = (L, l, label)
                top = int(np.abs(c.astype(np.int64)).max())
                ry, rout, _, _ = _oracle(name, L, state)
                assert top > min(Ts) and not np.array_equal(ry, y0), ("vacuous", tag)   # on the oracle
                ref = (ry, rout)
                n += 1
                y, out, st = _run(eng, name, L, 0, state)
                assert st[2] == (_lib.PATH_FUSED if fused else _lib.PATH_GENERIC) and _codes(st, nl) == [RK_QUAD32] * nl, (tag, st[:32])
                if _diff((y, out), ref) != (0, 0):
                    bad.append((tag, "default") + _diff((y, out), ref))
                y, out, st = _run(eng, name, L, EXACT, state)
                assert not fused or _codes(st, nl) == [RK_EXACT] * nl, (tag, st[:32])
                if _diff((y, out), ref) != (0, 0):
                    bad.append((tag, "exact") + _diff((y, out), ref))
                y, out, st = _run(eng, name, L, 0, state, f32=True)
                if _diff((y, out), ref) != (0, 0):
                    bad.append((tag, "f32") + _diff((y, out), ref))
                got = _ladder(eng, name, L, state)
                if _diff(got, ref) != (0, 0):
                    bad.append((tag, "forward_chunk") + _diff(got, ref))
                if not fused:   # the forward flags mean nothing on the generic path: a match is the only right answer
                    y, out, st = _run(eng, name, L, DEFER, state)
                    if _diff((y, out), ref) != (0, 0):
                        bad.append((tag, "generic+DEFER") + _diff((y, out), ref))
                for rung, (e, flags, code, kind) in rungs.items():
                    y, out, st = _run(e, name, L, flags, state)
                    assert _codes(st, nl) == [code] * nl, (tag, rung, st[:32])
                    redo = bool(st[0] & ST_REDO)
                    if top > thr[l][kind] and not redo:
                        bad.append((tag, rung, "no ST_REDO") + _diff((y, out), ref))
                    elif not redo and _diff((y, out), ref) != (0, 0):
                        bad.append((tag, rung, "silently wrong") + _diff((y, out), ref))
    print(f"wide carries, model {name}: {n} carries, {len(bad)} failures")
    assert not bad, (len(bad), bad[:12])


@gpu
def test_grouped_call_with_one_wide_carry(monkeypatch):
    """G = 3 groups in one set of launches (dim_scale 0.5, L = 37): group 0 starts from zeros, group 1 from a carry of
    +-(2^24 + r) in layer 1 (a 24-bit multiply sees r: the stored states stay small), group 2 from a small carry.  Every group must match its own oracle run; only group 1 may
    re-run (S5FXP_ST_WIDE_STATE of a default forward) or report S5FXP_ST_REDO, and it must.  Fails without the carry check
    (group 1 silently wrong, no S5FXP_ST_REDO), and if the check raises the flag or the status bits of another group than
    its own (GroupOff strides)."""
    import torch
    from sparsernns_amd import _lib
    name, L, G = 0.5, 37, 3
    nl, P = _model(name)[1]["n_layers"], _model(name)[1]["P"]
    thr = _thresholds(name, monkeypatch)
    rng = np.random.Generator(np.random.PCG64(7))
    state = np.zeros((G, nl, 2, B, P), dtype=np.int32)
    state[1, 1] = rng.choice(np.array([-1, 1]), (2, B, P)) * (2 ** 24 + rng.integers(0, 8, (2, B, P)))
    state[2, 0] = rng.integers(-200, 201, state[2, 0].shape)
    refs = [_oracle(name, L, state[g]) for g in range(G)]
    assert all(int(np.abs(state[1, 1]).max()) > t for t in thr[1].values())
    assert not np.array_equal(refs[1][0], refs[0][0]) and not np.array_equal(refs[2][0], refs[0][0])
    assert all(refs[g][2][i] <= thr[i]["pair"] for g in (0, 2) for i in range(nl)), "groups 0 and 2 must stay in range"
    ry, rout = np.concatenate([r[0] for r in refs]), np.stack([r[1] for r in refs])
    base = _base(name, L)
    x = _dev(name, L)[0].repeat(G, 1, 1)
    runs = [("default", "default", 0, RK_QUAD32)] + [(k,) + v[:3] for k, v in DEFER_RUNGS.items()]
    for rung, switch, flags, code in runs:
        eng = _engine(name, switch, monkeypatch)
        y = torch.empty((G * B, L, eng.d_out), dtype=torch.int32, device="cuda")
        sin = torch.from_numpy(state).cuda()
        sout = torch.zeros_like(sin)
        eng.enqueue(x, base["bits"], base["exp"], y, B, L, flags=flags, state_in=sin, state_out=sout, groups=G)
        torch.cuda.synchronize()
        st = eng.lane_status(0, G).cpu().numpy()[:G * _lib.STATUS_WORDS].reshape(G, _lib.STATUS_WORDS)
        y, out = y.cpu().numpy().reshape(G, B, L, -1), sout.cpu().numpy()
        for g in range(G):
            assert _codes(st[g], nl) == [code] * nl, (rung, g)
            raised = bool(st[g][0] & (ST_REDO if flags else ST_WIDE_STATE))
            assert raised == (g == 1), (rung, g, st[g][:8])
            if not (flags and g == 1):
                d = _diff((y[g], out[g]), (refs[g][0], refs[g][1]))
                assert d == (0, 0), (rung, g, d)
    assert np.array_equal(ry.shape, (G * B, L, _model(name)[1]["d_out"])) and rout.shape == state.shape


@gpu
@pytest.mark.parametrize("check", [True, False])
def test_loud_step_chunk_then_batch_chunk(check, monkeypatch):
    """End to end: a SessionPool serves a (1, 16) chunk at input scale 6 with the step kernel, which is exact for states of
    any width and leaves a carry beyond 16 bits, then a quiet 40-frame chunk from that carry through the batch path (the
    ladder with check=True, one self-contained default forward with check=False).  Outputs and carries must be the oracle's.
    Fails without the carry check: the second chunk's first steps multiply wrapped carries and nothing notices."""
    from sparsernns_amd import SessionPool, _lib
    from sparsernns_amd.fxparray import FxpArray
    name, S = 0.5, 2
    qc, dims, _, cm = _model(name)
    thr = _thresholds(name, monkeypatch)
    eng = _engine(name, "default", monkeypatch)
    eng.level, eng._redos = 0, [0, 0]
    pool = SessionPool(eng, S)
    ref_state = np.zeros((S, dims["n_layers"], 2, 1, dims["P"]), dtype=np.int32)
    for i, (L, scale, path) in enumerate(((16, 6.0, _lib.PATH_STEP), (40, 0.25, _lib.PATH_FUSED))):
        xf = synth.make_input(S, L, dims["d_in"], seed=900 + i, scale=scale)
        fx = O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
        if i == 1:   # on the oracle: the carry between the chunks is beyond every rung's threshold
            tops = np.abs(ref_state.astype(np.int64)).max(axis=(0, 2, 3, 4))
            assert any(tops[l] > max(thr[l].values()) for l in range(dims["n_layers"])), tops
            quiet = [cm.forward(fx.data[s][None], fx.bits, fx.exp, trace=True)[3] for s in range(S)]
            assert max(int(np.abs(t[k]).max()) for q in quiet for t in q for k in ("xs_re", "xs_im")) < min(thr[0].values())
        ref = []
        for s in range(S):
            st = np.ascontiguousarray(ref_state[s])
            ref.append(cm.forward(fx.data[s][None], fx.bits, fx.exp, state=st)[0][0])
            ref_state[s] = st
        y = pool.push(FxpArray(fx.data, fx.bits, fx.exp), check=check or i == 0)
        pool.check()
        assert pool.last_path == path, (i, pool.last_path)
        assert np.array_equal(y.numpy(), np.stack(ref)), (i, int(np.count_nonzero(y.numpy() != np.stack(ref))))
        assert np.array_equal(pool.state.cpu().numpy(), ref_state), (i, "carry")


# ------------------------------------------------------------------------------------------------------------------
# B. one state exactly at the bound
# ------------------------------------------------------------------------------------------------------------------
KINDS = [(ds, k) for ds in DIM_SCALES for k in ("pair", "quad16", "quad32")] + [(GENERIC, "generic")]


@gpu
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("name,kind", KINDS)
def test_a_state_exactly_at_the_bound(name, kind, L, monkeypatch):
    """The planted state (plant_at_bound: exact hit and layer maximum asserted on the oracle) at T - 1, T and T + 1, T being
    what the rung of `kind` compares with; the carry's components are at most T, one of them exactly T, so the carry is legal
    and its product with the coefficient is the largest the bound admits.  Planted in the bound-setting, the first and the
    last plantable state, in sequence 0 and B - 1, in both components with both signs; L = 1 (the extreme is the last frame
    and the carry out), 5 (ragged 4-step block), 37 (ragged 8-step block).

    Rungs of that kind under DEFER_REDO: at T - 1 and T no S5FXP_ST_REDO and the oracle's y and carry out; at T + 1
    S5FXP_ST_REDO, and Engine.forward_chunk gives the oracle's result.  (A state near full scale in an early layer can push
    a later layer's states past that layer's own threshold on the longer inputs; the oracle's traces say where, and
    S5FXP_ST_REDO is then required at every target.  The last layer, and every layer at L = 1, is free of that.)  The default forward gives the oracle's result at all
    three, and -- its only trace of a re-run -- raises S5FXP_ST_WIDE_STATE exactly when the oracle's largest state exceeds its
    quad32 (generic: quad) threshold.

    Fails if the checked value is T - 1 or less (S5FXP_ST_REDO / a re-run at T, or already for the carry of T), if it is
    T + 1 or more (no S5FXP_ST_REDO at T + 1; for quad16 the saturated 32767 passes, for quad32 a state of 32768 reaches the
    16-bit planes), if a check skips the last frame of a ragged block, the last state slot or the last sequence, and if
    scan_bounds' bound is too loose by one (the product at T wraps: wrong y without S5FXP_ST_REDO)."""
    nl = _model(name)[1]["n_layers"]
    thr = _thresholds(name, monkeypatch)
    eng = _engine(name, "default", monkeypatch)
    rungs = {k: (_engine(name, v[0], monkeypatch),) + v[1:] for k, v in DEFER_RUNGS.items() if v[3] == kind}
    rerun_T = [t["generic" if name == GENERIC else "quad32"] for t in thr]
    bad, n, clean = [], 0, [0] * nl
    for l in range(nl):
        T = thr[l][kind]
        cases = _bound_cases(name, l, T)
        assert len(cases) >= 16, (name, l, T, "fewer than two states to plant in")
        for (p, b, comp, s) in cases:
            for target in (T - 1, T, T + 1):
                state, ry, rout, tops = _planted(name, L, l, p, b, comp, s, T, target)
                ref, tag = (ry, rout), (l, p, b, comp, s, target - T)
                n += 1
                y, out, st = _run(eng, name, L, 0, state)
                assert _codes(st, nl) == [RK_QUAD32] * nl, (tag, st[:32])
                d = _diff((y, out), ref)
                if d != (0, 0):
                    bad.append((tag, "default") + d)
                if bool(st[0] & ST_WIDE_STATE) != any(tops[i] > rerun_T[i] for i in range(nl)):
                    bad.append((tag, "default", "re-run" if st[0] & ST_WIDE_STATE else "no re-run"))
                # the planted layer's output feeds the next ones: a later layer may leave the rung's range by itself
                wide = any(tops[i] > thr[i][kind] for i in range(nl))
                assert wide or target <= T
                clean[l] += target == T and not wide
                for rung, (e, flags, code, _) in rungs.items():
                    y, out, st = _run(e, name, L, flags, state)
                    assert _codes(st, nl) == [code] * nl, (tag, rung, st[:32])
                    redo, d = bool(st[0] & ST_REDO), _diff((y, out), ref)
                    if redo != wide:
                        bad.append((tag, rung, "false ST_REDO" if redo else "no ST_REDO") + d)
                    elif not redo and d != (0, 0):
                        bad.append((tag, rung, "wrong") + d)
                    if wide:
                        d = _diff(_ladder(e, name, L, state), ref)
                        if d != (0, 0):
                            bad.append((tag, rung, "forward_chunk") + d)
    print(f"at the bound, model {name}, {kind}, L = {L}: {n} plantings, {len(bad)} failures; per layer, plantings at T with "
          f"every layer in range: {clean}")
    # where the maximum sits exactly at T and nothing else is out of range, the forward must not have asked for a repeat: that
    # is the case in the last layer always (nothing follows it) and in every layer for the single frame
    assert clean[nl - 1] >= 16 and (L > 1 or min(clean) >= 16), clean
    assert not bad, (len(bad), bad[:12])
