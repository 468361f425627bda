"""The stated-exponent entries over the whole box s5fxp_model_exps_check admits (include/s5fxp.h s5fxp_model_forward_at,
s5fxp_model_clips_at, s5fxp_model_step_at and their _f32 / _i16 forms): tests/test_pinned_exps.py and
tests/test_forward_at.py run two exponent sets per model, both next to the ones the data would choose.  Here every model runs a
pool of legal sets -- the edges of the box, sets directed at each arm of bn16_row8, uniformly random sets and sets near the
natural one -- and every GPU comparison is np.array_equal against the NumPy oracle forced to the same exponents
(tests/pinned_helpers.py).

The pool is built on the CPU from fixed seeds.  Its premises (test_the_pool_*: every op clips in some set and loses three
bits in another, every reachable arm is reached, no set's output is degenerate, wide and narrow carries both occur) are
conditions on the pool, asserted without a GPU; the GPU tests run every set of the pool and filter nothing.

Three of those conditions no pool can meet, and the tests assert why where they say so: an add of -mean whose operands stay
below 1.0 chooses exp_max itself, so nothing legal lies above it; the scale-plus-bias model's carry is wide at every set; an
add's result shift beyond +-15 needs an operand exponent above 15, which only that model has.

Models: synth.make_model(calib_L=256) at dim_scale 0.25, 0.5, 0.75 and 1.0 and the scale-plus-bias contract model of
tests/test_forward_at.py (its _model), and one more at dim_scale 0.25 with negated BatchNorm means (_model below: the only
one in which the clip after x + (-mean) can act).  Inputs: two 70-frame sequences per model (one 64-frame tile and a tail; two 32-frame
tiles and a tail), and for the clip list three clips of 70, 33 and 1 frames.
"""
import functools
import itertools

import numpy as np
import pytest

import pinned_helpers as PH
import test_forward_at as FA
import test_pinned_exps as PE
from oracle import fxp_oracle as O
from sparsernns_amd import synth

gpu = pytest.mark.gpu
MODELS = ("s025", "s05", "s075", "s10", "bnsb", "negm025")
EXTRA = ("negm025",)   # beside the issue's five: dim_scale 0.25 with negated means (_model)
FAMILIES = ("edges", "arms", "uniform", "near")
L = 70
SEQ_SEEDS = (150, 151)
CLIP_LENS = (70, 33, 1)
STEPS = (1, 31, 32, 6)
N_RANDOM = {"s025": 24, "s05": 24, "s075": 12, "s10": 12, "bnsb": 12, "negm025": 12}
# "near": the common minimum plus an integer in -r..r per op.  r = 4 gives no carry beyond 16 bits at the larger models (0 of
# 150 at dim_scale 1.0), so the range is wider there
NEAR_RANGE = {"s025": 4, "s05": 4, "s075": 6, "s10": 6, "bnsb": 4, "negm025": 4}
MODEL_SEED = {k: 1000 + 17 * i for i, k in enumerate(MODELS)}


# ------------------------------------------------------------------------------------------------------------------
# sequences, the natural run, the pool, and the forced oracle results (computed once, shared, never written to)
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(key):
    """The five models of tests/test_forward_at.py, and one more: synth.make_model(calib_L=256) at dim_scale 0.25 with the
    calibrated BatchNorm means of every other channel negated.  A layer input is the output of a ReLU and a calibrated mean
    of it is >= 0, so in the five models x + (-mean) cannot leave the wider operand's bits and the clip after that sum never
    acts, whatever the exponents: where the sum is stated too tight it is the operand's own shift that clips.  With -mean > 0
    an input on its rail plus the mean leaves 16 bits, and the clip after the sum is what the oracle's result hangs on."""
    if key not in EXTRA:
        return FA._model(key)
    md, qc, dims = synth.make_model(dim_scale=0.25, calib_L=256)
    for i in range(dims["n_layers"]):
        md["encoder"][f"layers_{i}"]["norm"]["mean"][::2] *= -1

    @functools.lru_cache(maxsize=None)
    def product():
        from sparsernns_amd.fxpmodel import build_regression_model
        return build_regression_model(md, qc, dims["n_layers"])

    return FA._Model(O.RegressionModel(md, qc, dims["n_layers"]), qc, dims, product)


@functools.lru_cache(maxsize=None)
def _seqs(key):
    m = _model(key)
    return np.stack([FA._seq(m, L, s) for s in SEQ_SEEDS])


def _clips(key):
    a, b = _seqs(key)
    return [a, b[:33], a[:1]]


@functools.lru_cache(maxsize=None)
def _natural(key):
    """Per sequence (y, carry, exponents) of the unforced oracle from a zero carry."""
    m = _model(key)
    return tuple(PH.forced_run(m.om, s, m.bits, m.exp, None) for s in _seqs(key))


@functools.lru_cache(maxsize=None)
def _base(key):
    """The batch's common minimum set: per op the smaller of the two sequences' own exponents."""
    e = np.min([n[2] for n in _natural(key)], axis=0).astype(np.int32)
    assert PH.shifts_ok(_model(key).om, e)
    return e


def _present(key):
    mx = PH.exp_max(_model(key).om)
    return [(l, k) for l in range(mx.shape[0]) for k in range(5) if mx[l, k] >= 0]


def _legal(key, e) -> bool:
    mx = PH.exp_max(_model(key).om)
    return all(0 <= e[l, k] <= mx[l, k] for l, k in _present(key)) and PH.shifts_ok(_model(key).om, e)


def _coordinate_range(key, l, k):
    """The lowest and the highest value of op (l, k) that is legal with every other op at the common minimum."""
    mx, e = PH.exp_max(_model(key).om), _base(key).copy()
    ok = []
    for v in range(mx[l, k] + 1):
        e[l, k] = v
        if PH.shifts_ok(_model(key).om, e):
            ok.append(v)
    return ok[0], ok[-1]


def _with(base, pairs):
    e = base.copy()
    for (l, k), v in pairs:
        e[l, k] = v
    return e


@functools.lru_cache(maxsize=None)
def _arm_candidates(key):
    """{(layer, arm): [legal sets]} over every value of the three exponents bn16_row_arm's shifts come from -- the layer's first
    two ops and the residual add of the layer before -- with the other ops at the common minimum.  What the restated rule
    can reach on a layer is what this holds."""
    om, base, mx = _model(key).om, _base(key), PH.exp_max(_model(key).om)
    out = {}
    for i in range(base.shape[0]):
        if PH.row_arms(om, base)[i] is None:
            continue
        prev = range(mx[i - 1, 4] + 1) if i else [None]
        for p, a, b in itertools.product(prev, range(mx[i, 0] + 1), range(mx[i, 1] + 1)):
            e = _with(base, [((i, 0), a), ((i, 1), b)] + ([((i - 1, 4), p)] if i else []))
            if PH.shifts_ok(om, e):
                out.setdefault((i, PH.row_arms(om, e)[i]), []).append(e)
    return out


def _directed(key):
    """Sets that put each arm on every layer where it is reachable: per (layer, arm) the candidate at the median distance from
    the common minimum and the one farthest from it.  The scale-plus-bias model has no row chain: its directed sets are the four joint
    extremes of a layer's scale multiply and bias add, the bias add moved back towards the minimum where the pair is not legal."""
    base = _base(key)
    out = []
    if key == "bnsb":
        for l in range(base.shape[0]):
            r2, r3 = _coordinate_range(key, l, 2), _coordinate_range(key, l, 3)
            for v2, v3 in itertools.product(r2, r3):
                step = 1 if base[l, 3] > v3 else -1
                while not _legal(key, _with(base, [((l, 2), v2), ((l, 3), v3)])):
                    v3 += step
                out.append(_with(base, [((l, 2), v2), ((l, 3), v3)]))
        return out
    for (i, arm), sets in sorted(_arm_candidates(key).items()):
        # the nearest would be the minimum itself or a step from it, which tests/test_forward_at.py runs; down to the SSM
        # input's exponent a looser second op of layer 0 alone changes no bit of the output
        order = np.argsort([int(np.abs(e - base).sum()) for e in sets], kind="stable")
        out += [sets[order[len(order) // 2]], sets[order[-1]]]
    return out


def _random(key, near: bool):
    om, base, mx, rng = _model(key).om, _base(key), PH.exp_max(_model(key).om), np.random.default_rng(MODEL_SEED[key] + near)
    out, r = [], NEAR_RANGE[key]
    while len(out) < N_RANDOM[key]:
        if near:
            e = np.clip(base + rng.integers(-r, r + 1, size=base.shape), 0, np.maximum(mx, 0))
        else:
            e = rng.integers(0, np.maximum(mx, 0) + 1)
        e = np.where(mx >= 0, e, 0).astype(np.int32)
        if PH.shifts_ok(om, e):
            out.append(e)
    return out


def _unique(sets):
    seen, out = set(), []
    for e in sets:
        t = tuple(int(v) for v in np.asarray(e).ravel())
        if t not in seen:
            seen.add(t)
            out.append(t)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _pool(key):
    """{family: tuple of sets}, a set as the flat tuple of its 5 * n_layers values (0 in an absent op's slot)."""
    om, base = _model(key).om, _base(key)
    edges = []
    for l, k in _present(key):
        edges += [_with(base, [((l, k), v)]) for v in _coordinate_range(key, l, k)]
    edges += [PH.corner(om, base, -1), PH.corner(om, base, +1)]
    edges = [e for e in edges if not np.array_equal(e, base)]   # the minimum itself is what tests/test_forward_at.py runs
    pool = {"edges": _unique(edges), "arms": _unique(_directed(key)), "uniform": _unique(_random(key, False)),
            "near": _unique(_random(key, True))}
    for fam, sets in pool.items():
        assert all(_legal(key, _arr(key, t)) for t in sets), (key, fam)
    return pool


def _arr(key, t):
    return np.asarray(t, dtype=np.int32).reshape(-1, 5)


def _all_sets(key):
    return [(fam, t) for fam in FAMILIES for t in _pool(key)[fam]]


@functools.lru_cache(maxsize=None)
def _ref(key, t):
    """Per sequence (y, carry, the exponents each op would have chosen there) of the oracle forced to the set t."""
    m = _model(key)
    return tuple(PH.forced_run(m.om, s, m.bits, m.exp, _arr(key, t)) for s in _seqs(key))


@functools.lru_cache(maxsize=None)
def _ref_clips(key, t):
    """Per clip (y, carry) of the forced oracle: the first is sequence 0 whole."""
    m = _model(key)
    a, b, c = _clips(key)
    return (_ref(key, t)[0][:2],) + tuple(PH.forced_run(m.om, s, m.bits, m.exp, _arr(key, t))[:2] for s in (b, c))


def _wide(key, t) -> bool:
    return any(np.abs(r[1]).max() > 32767 for r in _ref(key, t))


# ------------------------------------------------------------------------------------------------------------------
# not GPU: the premises.  Conditions on the pool, not on the kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MODELS)
def test_the_pool_is_legal_and_spans_the_box(key):
    m, pool, base, mx = _model(key), _pool(key), _base(key), PH.exp_max(_model(key).om)
    sizes = {fam: len(pool[fam]) for fam in FAMILIES}
    print(f"{key}: pool {sizes}, {sum(sizes.values())} sets; common minimum {base.tolist()}")
    assert sizes["uniform"] == N_RANDOM[key] and sizes["near"] == N_RANDOM[key], sizes
    assert sizes["edges"] >= len(_present(key)) + 2 and sizes["arms"] >= 2, sizes
    sets = np.array([_arr(key, t) for _, t in _all_sets(key)])
    for l, k in _present(key):
        lo, hi = _coordinate_range(key, l, k)
        assert lo <= base[l, k] <= hi and sets[:, l, k].min() <= lo and sets[:, l, k].max() >= hi, (l, k)
        assert hi - lo >= 4, (l, k, lo, hi)   # a box, not a point
    low, high = PH.corner(m.om, base, -1), PH.corner(m.om, base, +1)
    assert np.all(low <= base) and np.all(high >= base) and not np.array_equal(low, high)
    # a corner is one: no single op can move further out
    for e, d in ((low, -1), (high, +1)):
        for l, k in _present(key):
            assert not _legal(key, _with(e, [((l, k), e[l, k] + d)])), (d, l, k)


@pytest.mark.parametrize("key", MODELS)
def test_the_pool_spans_the_adds_result_shifts(key):
    """An add's result shift `post` is legal in -31..31.  With every operand exponent at 15 or below, as in the recipe's models,
    no stated exponent takes it out of -15..0 for the add of -mean; the contract model's encoder output has exponent 20, and
    there the pool must hold shifts beyond -15 -- a derivation that is right only up to 15 passes everywhere else."""
    om = _model(key).om
    posts = [PH.add_posts(om, _arr(key, t)) for _, t in _all_sets(key)]
    beyond = sum(any(abs(p) > 15 for p in ps) for ps in posts)
    lowest = -max(om.encoder.qc["out_exp"], om.layers[0].norm.minus_mean.exp)
    print(f"{key}: result shifts of the adds span {min(map(min, posts))}..{max(map(max, posts))}; {beyond} sets hold one beyond 15; "
          f"layer 0's lowest possible is {lowest}")
    assert min(map(min, posts)) <= -15 and max(map(max, posts)) >= 0
    assert beyond >= 4 if lowest < -15 else beyond == 0, (beyond, lowest)


@pytest.mark.parametrize("key", MODELS)
def test_the_pool_clips_and_loses_precision_at_every_op(key):
    """For every present op one set states an exponent above what the op would choose at that point of the forced run (the
    result clips) and one states it at least 3 below (three bits are lost).

    No set can clip an op that chooses exp_max itself: no legal exponent lies above it.  That is the add of -mean (op 0) of the
    first layers, on any input: the encoder output is a 16-bit value at exponent 15 or more after a ReLU, below 1.0, every -mean
    is <= 0, so the sum stays below 1.0 and takes no integer bit; a later layer's input is the ReLU of a residual that these
    inputs keep below 1.0 as well.  Such an op is not waved through: it must be an op 0, and it must choose exp_max in EVERY
    forced run of the pool (asserted), which is the statement that the condition cannot be met for it."""
    mx = PH.exp_max(_model(key).om)
    above, below, at_max, runs = {}, {}, {}, 0
    for _, t in _all_sets(key):
        e = _arr(key, t)
        for y, carry, would in _ref(key, t):
            runs += 1
            for l, k in _present(key):
                above[l, k] = above.get((l, k), 0) + int(e[l, k] > would[l, k])
                below[l, k] = below.get((l, k), 0) + int(e[l, k] <= would[l, k] - 3)
                at_max[l, k] = at_max.get((l, k), 0) + int(would[l, k] == mx[l, k])
    never = [op for op in _present(key) if at_max[op] == runs]
    print(f"{key}: (sequence, set) pairs that clip {above}, that lose 3 bits {below}; ops that choose exp_max in all {runs} runs {never}")
    if key in EXTRA:   # not one of the five models the conditions are set for: held to what it was added for
        assert any(above[l, 0] >= 1 for l in range(mx.shape[0])), above
        return
    assert all(k == 0 for _, k in never), never
    for op in _present(key):
        assert below[op] >= 1, (op, below[op])
        assert above[op] >= 1 or op in never, (op, above[op], at_max[op], runs)


@pytest.mark.parametrize("key", MODELS)
def test_the_pool_reaches_every_reachable_arm(key):
    om = _model(key).om
    if key == "bnsb":
        assert PH.row_arms(om, _base(key)) == [None] * len(om.layers)   # scale and bias: never the row chain
        mx = PH.exp_max(om)
        sets = np.array([_arr(key, t) for t in _pool(key)["arms"]])
        for l in range(len(om.layers)):
            for k in (2, 3):
                lo, hi = _coordinate_range(key, l, k)
                assert mx[l, k] >= 0 and sets[:, l, k].min() == lo and sets[:, l, k].max() == hi, (l, k)
        return
    reachable = set(_arm_candidates(key))
    count = {}
    for fam, t in _all_sets(key):
        for i, arm in enumerate(PH.row_arms(om, _arr(key, t))):
            count[i, arm] = count.get((i, arm), 0) + 1
    report = {f"layer {i} {PH.ARM_NAMES[a]}": n for (i, a), n in sorted(count.items())}
    print(f"{key}: sets per arm {report}")
    for i in range(len(om.layers)):
        # the two packed arms are what the natural exponents give; GENERIC is asserted only where the rule says it can be had
        assert (i, PH.ROW_PACKED) in reachable or (i, PH.ROW_SHIFTED) in reachable, i
    assert set(count) == reachable, (report, sorted(reachable))   # every reachable arm, and none the enumeration missed
    # Layer 0's shx1 is fixed by the encoder, and with it and the mean at exponent 15 the stated exponent of the sum cannot
    # exceed their maximum (l1 = 0): GENERIC there needs a change_cfg to the SSM input beyond the packed shifts, which the
    # legal range of op 1 may or may not hold.  What the rule says is what the candidates hold; it is reported, not assumed
    q = om.encoder.qc
    ea = max(q["out_exp"], om.layers[0].norm.minus_mean.exp)
    lo1, hi1 = _coordinate_range(key, 0, 1)
    ue = om.layers[0].mixer.qc["activations"]["u"]["exp"]
    generic0 = ea - q["out_exp"] > 14 or PH.exp_max(om)[0, 0] > ea or ue - lo1 > 14 or hi1 - ue > 15
    print(f"{key}: layer 0 shx1 = {ea - q['out_exp']}, op 1 legal in {lo1}..{hi1} at u_exp {ue}: GENERIC reachable there: {generic0}")
    assert ((0, PH.ROW_GENERIC) in reachable) == generic0, report
    for i in range(1, len(om.layers)):
        assert (i, PH.ROW_GENERIC) in reachable, (i, report)   # a residual exponent of 0 in front gives shx1 = 15


@pytest.mark.parametrize("key", MODELS)
def test_the_pool_s_outputs_keep_their_variety(key):
    m = _model(key)
    q = m.om.decoder.qc
    rails = (-(1 << (q["out_bits"] - 1)), (1 << (q["out_bits"] - 1)) - 1)
    for fam, t in _all_sets(key):
        ref, nat = _ref(key, t), _natural(key)
        assert any(not np.array_equal(r[0], n[0]) for r, n in zip(ref, nat)), (fam, t)
        for b, (y, carry, _) in enumerate(ref):
            rows = len(np.unique(y, axis=0))
            on_rails = float(np.mean((y == rails[0]) | (y == rails[1])))
            assert rows >= L // 2 and on_rails < 0.5, (fam, t, b, rows, on_rails)


@pytest.mark.parametrize("key", MODELS)
def test_the_pool_has_wide_and_narrow_carries(key):
    wide = {fam: sum(_wide(key, t) for t in _pool(key)[fam]) for fam in FAMILIES}
    n = {fam: len(_pool(key)[fam]) for fam in FAMILIES}
    print(f"{key}: sets with a carry beyond 32767 per family {wide} of {n}")
    assert sum(wide.values()) >= 10, (wide, n)
    # A narrow carry needs a model that has one.  The scale-plus-bias model keeps its states at exponents 17 and 18, and both
    # sequences' own carries leave 16 bits by a factor of two; of 300 further legal sets, uniform and within 6 of the minimum,
    # none brought the largest state below 60 481.  Nothing is asked of it but that this stays so: if a set of its pool ever
    # has a narrow carry the condition applies to it again.  Every other model must have at least 10 sets of either kind
    if key in EXTRA:   # not one of the five models the condition is set for; its negated means make every layer loud
        return
    if key == "bnsb" and sum(wide.values()) == sum(n.values()):
        assert all(np.abs(c).max() > 2 * 32767 for _, c, _ in _natural(key))
    else:
        assert sum(n.values()) - sum(wide.values()) >= 10, (wide, n)


# ------------------------------------------------------------------------------------------------------------------
# GPU: every set of the pool against the forced oracle, np.array_equal
# ------------------------------------------------------------------------------------------------------------------
def _words(key, e):
    return np.where(PH.exp_max(_model(key).om) >= 0, e, 0)


def _fwd_equals(key, eng, t, flags=0, carry=True, redo_ok=False):
    """One forward_at of the two sequences at the set t against the oracle; returns True where a deferred forward raised REDO."""
    from sparsernns_amd import _lib
    m, e, ref = _model(key), _arr(key, t), _ref(key, t)
    y, c, st = FA._fwd_raw(eng, _seqs(key), m.bits, m.exp, e, carry=carry, flags=flags)
    assert st[0, 2] == _lib.PATH_FUSED and np.array_equal(FA._exps_words(st[0], eng.n_layers), _words(key, e)), (t, flags)
    if redo_ok and st[0, 0] & _lib.ST_REDO:
        return True
    assert (st[0, 0] & ~_lib.ST_WIDE_STATE) == 0, (t, flags, st[0, 0])
    for b in range(2):
        assert np.array_equal(y[b], ref[b][0]), (t, flags, carry, b)
        if carry:
            assert np.array_equal(c[:, :, b], ref[b][1]), (t, flags, b)
    return False


@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("key", MODELS)
def test_forward_at_equals_the_forced_oracle(key, family):
    from sparsernns_amd import _lib
    eng = _model(key).engine()
    redo = 0
    for t in _pool(key)[family]:
        eng.check_exps(_arr(key, t))
        _fwd_equals(key, eng, t, carry=False)
        _fwd_equals(key, eng, t)
        redo += _fwd_equals(key, eng, t, flags=_lib.FWD_DEFER_REDO, redo_ok=True)
        _fwd_equals(key, eng, t, flags=_lib.FWD_EXACT)
    print(f"{key} {family}: {redo} of {len(_pool(key)[family])} deferred forwards raised ST_REDO")


@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("key", MODELS)
def test_clips_at_equals_the_forced_oracle(key, family):
    from sparsernns_amd import _lib
    m = _model(key)
    eng = m.engine()
    x = PE._pad(_clips(key), L)
    for t in _pool(key)[family]:
        e, ref = _arr(key, t), _ref_clips(key, t)
        y, carry, st = PE._clips_raw(eng, x, CLIP_LENS, m.bits, m.exp, e)
        for i, n in enumerate(CLIP_LENS):
            assert np.array_equal(y[i, :n], ref[i][0]), (t, i)
            assert np.all(y[i, n:] == PE.SENTINEL), (t, i)
            assert np.array_equal(carry[i], ref[i][1]), (t, i)
            assert (st[i, 0] & ~_lib.ST_WIDE_STATE) == 0 and st[i, 1] == eng.out_exp and st[i, 2] == _lib.PATH_CLIP, (t, i)
            assert np.array_equal(FA._exps_words(st[i], eng.n_layers), _words(key, e)), (t, i)


@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("key", MODELS)
def test_steps_with_the_carry_equal_the_forced_oracle(key, family):
    """The 70 frames as steps of 1, 31, 32 and 6 rows, each sequence a group of one stream: chunk invariance at every set."""
    from sparsernns_amd import _lib
    m = _model(key)
    eng, x = m.engine(), _seqs(key)[:, None]
    for t in _pool(key)[family]:
        e, ref = _arr(key, t), _ref(key, t)
        state, ys, at = np.zeros((2, eng.n_layers, 2, 1, eng.P), dtype=np.int32), [], 0
        for n in STEPS:
            y, state, st = PE._step_raw(eng, x[:, :, at:at + n], m.bits, m.exp, e, state)
            for g in range(2):
                assert (st[g, 0] & ~_lib.ST_WIDE_STATE) == 0 and st[g, 2] == _lib.PATH_STEP, (t, at)
                assert np.array_equal(FA._exps_words(st[g], eng.n_layers), _words(key, e)), (t, at)
            ys.append(y[:, 0])
            at += n
        y = np.concatenate(ys, axis=1)
        for g in range(2):
            assert np.array_equal(y[g], ref[g][0]), (t, g)
            assert np.array_equal(state[g, :, :, 0], ref[g][1]), (t, g)


@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("key", MODELS)
def test_two_forwards_with_the_carry_equal_the_forced_oracle(key, family):
    """Frames 0..32 and 33..69 as two forward_at calls: every edge and arm set, every third random one."""
    m = _model(key)
    eng, x = m.engine(), _seqs(key)
    sets = _pool(key)[family]
    for t in sets if family in ("edges", "arms") else sets[::3]:
        e, ref = _arr(key, t), _ref(key, t)
        ya, ca, _ = FA._fwd_raw(eng, x[:, :33], m.bits, m.exp, e, carry=True)
        yb, cb, _ = FA._fwd_raw(eng, x[:, 33:], m.bits, m.exp, e, state_in=ca)
        y = np.concatenate([ya, yb], axis=1)
        for b in range(2):
            assert np.array_equal(y[b], ref[b][0]) and np.array_equal(cb[:, :, b], ref[b][1]), (t, b)


@gpu
@pytest.mark.parametrize("family", ["edges", "arms"])
@pytest.mark.parametrize("key", ["s05", "s10"])
def test_float_and_int16_boundaries_equal_the_forced_oracle(key, family):
    """The conversions of tests/test_forward_boundaries.py: _f32 is from_fp -> the int entry -> to_float, _i16 the int entry on
    the same integers in 2 bytes.  At the edges the decoder's output sits on its rails most often."""
    m = _model(key)
    eng, x = m.engine(), _seqs(key)
    xf = np.ldexp(x.astype(np.float32), -m.exp).astype(np.float32)   # floats whose FLOOR at m.exp is exactly x
    assert eng.out_bits <= 16 and np.abs(x).max() < 32768
    for t in _pool(key)[family]:
        e, ref = _arr(key, t), _ref(key, t)
        yf, cf, _ = FA._fwd_raw(eng, xf, m.bits, m.exp, e, carry=True)
        yi, ci, _ = FA._fwd_raw(eng, x.astype(np.int16), m.bits, m.exp, e, carry=True)
        assert yi.dtype == np.int16
        for b in range(2):
            want = np.ldexp(ref[b][0].astype(np.float32), -eng.out_exp).astype(np.float32)
            assert np.array_equal(yf[b].view(np.int32), want.view(np.int32)), (t, b)
            assert np.array_equal(yi[b].astype(np.int32), ref[b][0]), (t, b)
            assert np.array_equal(cf[:, :, b], ref[b][1]) and np.array_equal(ci[:, :, b], ref[b][1]), (t, b)


@gpu
@pytest.mark.parametrize("family", ["edges", "arms"])
@pytest.mark.parametrize("key", ["s025", "s05"])
def test_the_four_reduction_route_equals_the_default_engine(key, family, monkeypatch):
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine
    m = _model(key)
    eng, x = m.engine(), _seqs(key)
    monkeypatch.setenv("S5FXP_NO_BN_EXT", "1")   # read once, at creation: a fused model on the four-reduction route
    four = Engine(m.export())
    monkeypatch.delenv("S5FXP_NO_BN_EXT")
    assert _lib.lib.s5fxp_model_is_fast(four._h)
    for t in _pool(key)[family]:
        e, ref = _arr(key, t), _ref(key, t)
        for carry in (False, True):
            a, b = FA._fwd_raw(four, x, m.bits, m.exp, e, carry=carry), FA._fwd_raw(eng, x, m.bits, m.exp, e, carry=carry)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and (not carry or np.array_equal(a[1], b[1])), t
            for s in range(2):
                assert np.array_equal(a[0][s], ref[s][0]) and (not carry or np.array_equal(a[1][:, :, s], ref[s][1])), (t, s)


# ------------------------------------------------------------------------------------------------------------------
# the host check against its restatement (gpu only because creating a model needs a device)
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", MODELS)
def test_exps_check_is_the_restated_rule(key):
    from sparsernns_amd import _lib
    m = _model(key)
    eng, mx = m.engine(), PH.exp_max(m.om)
    assert np.array_equal(eng.exp_max(), mx)
    rng = np.random.default_rng(MODEL_SEED[key] + 7)
    seen = {_lib.S5FXP_OK: 0, _lib.S5FXP_EBADARG: 0, _lib.S5FXP_ENEGSHIFT: 0}
    for n in range(2000):
        e = rng.integers(-1, 17, size=mx.shape).astype(np.int32)
        if n % 2:   # an absent op's slot may hold anything
            e = np.where(mx >= 0, e, rng.integers(-2 ** 31, 2 ** 31 - 1, size=mx.shape, dtype=np.int64).astype(np.int32))
        inside = bool(np.all((mx < 0) | ((e >= 0) & (e <= mx))))
        want = _lib.S5FXP_EBADARG if not inside else _lib.S5FXP_OK if PH.shifts_ok(m.om, e) else _lib.S5FXP_ENEGSHIFT
        eh = np.ascontiguousarray(e)
        assert _lib.lib.s5fxp_model_exps_check(eng._h, eh.ctypes.data) == want, (e.tolist(), want)
        seen[want] += 1
        if want == _lib.S5FXP_OK:
            eng.check_exps(e)
    print(f"{key}: {seen}")
    assert all(v >= 20 for v in seen.values()), seen
