"""gate_ext: between two lazy layers the gate kernel gathers the per-channel extremes of the aligned
sum U it stores -- packed uint16 running minima / maxima over the frames it really stores -- and leaves them, in U units, in the
EXT_REPS replicas of the next layer's block of extremes.  The residual pass keeps its launch and its head (the result shift, status
word 4) but reads no plane: one workgroup per group resolves every word of the block in place.

  * CPU: on the C oracle's traces, resolve-per-replica-then-fold over an arbitrary split of the frames into 8 replicas gives the
    per-channel extremes of the oracle's residual output; the biased-float encoding round-trips the values U can take;
  * GPU parity: four engines from one export -- default, MODEL_NO_GATE_EXT, MODEL_NO_RESID_LAZY, MODEL_NO_RESID_FOLD -- give
    equal outputs and per-layer status words, equal to the C oracle's, group by group; the default engine's residual launches
    have one workgroup per group;
  * a sequence that ends on a burst (the padded steps behind it keep growing: the mask on the frames a tile really holds);
  * the float and the int16 model boundaries take the route and match the MODEL_NO_GATE_EXT engine bit for bit.
"""
import numpy as np
import pytest

from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth
from test_resid_fold import I32, _forms, _input, _model, _np_traces, _profiled, np_resolve, np_usum
from test_resid_lazy import POSTS, _lazy

EXT_BIAS = np.float32(65536.0)   # mfma_bn.hpp
EXT_REPS = 8


# --------------------------------------------------------------------------------------------------------------------
# the restatement: what the gate kernel's tail, the head-only pass and the B projection's prologue do with the extremes
# --------------------------------------------------------------------------------------------------------------------
def np_encode(v, is_max):
    v = np.asarray(v).astype(np.float32)
    return (EXT_BIAS + v if is_max else EXT_BIAS - v).astype(np.float32)


def np_decode(e, is_max):
    e = np.asarray(e, dtype=np.float32)
    return ((e - EXT_BIAS) if is_max else (EXT_BIAS - e)).astype(np.int64)


def np_gate_tail(u, replica_of_frame):
    """(EXT_REPS, 2, H) float32: per replica the encoded minima and maxima of the frames that went to it; a replica nobody
    wrote keeps the zeros the forward's head left there."""
    H = u.shape[-1]
    ext = np.zeros((EXT_REPS, 2, H), dtype=np.float32)
    for r in range(EXT_REPS):
        rows = u[replica_of_frame == r]
        if rows.shape[0]:
            ext[r, 0] = np_encode(rows.min(axis=0), False)
            ext[r, 1] = np_encode(rows.max(axis=0), True)
    return ext


def np_head_only(ext, post):
    out = ext.copy()
    for b, is_max in ((0, False), (1, True)):
        w = ext[:, b]
        res = np_encode(np_resolve(np_decode(w, is_max), post), is_max)
        out[:, b] = np.where(w == 0, np.float32(0), res)
    return out


def np_prologue_fold(ext):
    e = ext.max(axis=0)   # bn_finalize_mm_body: a float maximum over the replicas, then the decode
    return np_decode(e[0], False), np_decode(e[1], True)


def test_biased_float_encoding_round_trips_the_sum():
    for v in (0, 1, 32767, 32768, 65534):
        for is_max in (False, True):
            e = np_encode(v, is_max)
            assert e.dtype == np.float32 and e > 0          # above the zero of a word nobody wrote
            assert int(np_decode(e, is_max)) == v, (v, is_max)
    # the identities of a thread that stored no frame stay below / at every real value
    assert np_encode(65535, False) > 0 and np_encode(65535, False) < np_encode(65534, False)
    assert 0 < np_encode(0, True) <= np_encode(1, True) and np_encode(0, True) < np_encode(65534, True)
    u = np.arange(0, 65535)
    assert np.array_equal(np_decode(np_encode(u, False), False), u) and np.array_equal(np_decode(np_encode(u, True), True), u)


@pytest.mark.parametrize("scale", [0.25, 1.0])
def test_resolved_replicas_fold_to_the_extremes_of_the_residual_output(scale):
    """On the C oracle's traces of the benchmark model (B = 2, L = 70), every layer that feeds another layer.  The C trace has no
    encoder output, so layer 0's skip operand and the static exponents come from the NumPy oracle's trace, whose planes are
    checked to be the C oracle's."""
    B, L = 2, 70
    md, qc, dims, export = _model("synth_ds0.5")
    nl = dims["n_layers"]
    fx = _input(qc, dims, B, L, seed=600, scale=scale)
    _, _, _, rtr = cref.CModel(export).forward(fx.data, fx.bits, fx.exp, trace=True)
    layers = _np_traces(md, qc, dims, fx)
    rng = np.random.Generator(np.random.PCG64(14))
    for li in range(nl - 1):
        z, skip = layers[li]["post_GLU"], layers[li]["ssm_input"]
        assert np.array_equal(z.data, rtr[li]["post_glu"]) and np.array_equal(layers[li]["residadd"].data, rtr[li]["residadd"])
        skip_data = skip.data if li == 0 else np.maximum(rtr[li - 1]["residadd"], 0)
        assert li == 0 or skip.exp == rtr[li - 1]["residadd_exp"]
        assert np.array_equal(skip_data, skip.data)
        H = z.data.shape[-1]
        u = np_usum(rtr[li]["post_glu"], skip_data, z.exp, skip.exp).reshape(-1, H)
        post = rtr[li]["residadd_exp"] - max(z.exp, skip.exp)
        assert post in POSTS
        h = np.maximum(rtr[li]["residadd"], 0).reshape(-1, H)
        # an arbitrary split: random, one replica left empty, and everything in one replica
        splits = [rng.integers(0, EXT_REPS, u.shape[0]), rng.integers(0, EXT_REPS - 1, u.shape[0]), np.full(u.shape[0], 3)]
        for rep in splits:
            lo, hi = np_prologue_fold(np_head_only(np_gate_tail(u, rep), post))
            assert np.array_equal(lo, h.min(axis=0)), (scale, li, post)
            assert np.array_equal(hi, h.max(axis=0)), (scale, li, post)


# --------------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------------
def _engines():
    from sparsernns_amd import _lib
    return (("gate_ext", 0), ("reading", _lib.MODEL_NO_GATE_EXT), ("stored", _lib.MODEL_NO_RESID_LAZY), ("two_plane", _lib.MODEL_NO_RESID_FOLD))


def _lazy_grids(kernels):
    return [g for n, g in kernels if "k_resid_minmax16" in n and "ResidLazyArgs" in n]


def _check_launches(eng_name, kernels, nl, G, many_frames=False):
    fold, plain, r1, r2 = _forms(kernels)
    assert (fold, plain, r1, r2) == ((0, nl, 0, nl - 1) if eng_name == "two_plane" else (nl, 0, nl - 1, 0)), (eng_name, fold, plain, r1, r2)
    assert _lazy(kernels) == (nl - 1 if eng_name in ("gate_ext", "reading") else 0), (eng_name, [n for n, _ in kernels])
    grids = _lazy_grids(kernels)
    if eng_name == "gate_ext":   # the head-only launch: one workgroup per group
        assert len(grids) == nl - 1 and all(g[0] == 1 and g[1] == G for g in grids), grids
    elif eng_name == "reading" and many_frames:   # the reading pass: a workgroup per span of frames (one span holds 128 of them)
        assert len(grids) == nl - 1 and all(g[0] > 1 and g[1] == G for g in grids), grids


def _run_four(export, dims, parts, B, L, G, refs, carry_refs=None, s_in=None):
    """The grouped forward of `parts` on the four engines: launch forms, outputs and status words against refs (the C oracle's
    traced forwards) and against each other."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine

    nl, P = dims["n_layers"], dims["P"]
    bits, exp = parts[0].bits, parts[0].exp
    x = torch.from_numpy(np.concatenate([p.data for p in parts])).cuda()
    got = {}
    for eng_name, flags in _engines():
        eng = Engine(export, flags=flags)
        assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
        y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        kw = {}
        if s_in is not None:
            kw = dict(state_in=torch.from_numpy(s_in).cuda(), state_out=torch.empty((G, nl, 2, B, P), dtype=torch.int32, device="cuda"))
        kernels = _profiled(lambda: eng.enqueue(x, bits, exp, y, B, L, flags=_lib.FWD_DEFER_REDO, groups=G, **kw))
        st = eng.lane_status(0, G).cpu().numpy().copy()
        _check_launches(eng_name, kernels, nl, G, many_frames=B * L > 128)
        yy = y.cpu().numpy().reshape(G, B, L, -1)
        for g in range(G):
            ref, rb, re_, rtr = refs[g]
            w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
            assert w[2] == _lib.PATH_FUSED and not (w[0] & (_lib.ST_REDO | _lib.ST_NEGSHIFT | _lib.ST_NEGEXP)), (eng_name, w[:8])
            assert all(int(w[8 + 8 * i + 5]) in (2, 3, 4) for i in range(nl)), (eng_name, w[8:8 + 8 * nl])
            assert (eng.out_bits, eng.out_exp) == (rb, re_)
            assert np.array_equal(yy[g], ref), (eng_name, g, np.count_nonzero(yy[g] != ref))
            assert [int(w[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in rtr], (eng_name, g)
        if s_in is not None:
            assert np.array_equal(kw["state_out"].cpu().numpy(), carry_refs), eng_name
        got[eng_name] = (yy, st)
    for other in ("reading", "stored", "two_plane"):
        assert np.array_equal(got["gate_ext"][0], got[other][0]), other
        for g in range(G):       # every per-layer status word [8 + 8l + 0..7], group by group
            a = got["gate_ext"][1][g * _lib.STATUS_WORDS + 8:g * _lib.STATUS_WORDS + 8 + 8 * nl]
            b = got[other][1][g * _lib.STATUS_WORDS + 8:g * _lib.STATUS_WORDS + 8 + 8 * nl]
            assert np.array_equal(a, b), (other, g, a, b)


# G = 2, B = 2, L = 70: two full 32-frame gate tiles and a 6-frame one per sequence, two groups whose residual adds get different
# exponents; L = 1 and L = 33 with B = 1: a workgroup with a single tile, whose z leaves through the final tiles_in_out(false)
@pytest.mark.gpu
@pytest.mark.parametrize("G,B,L,carry", [(2, 2, 70, False), (1, 1, 1, False), (1, 1, 33, False), (2, 2, 70, True)])
def test_four_engines_agree_with_the_oracle(G, B, L, carry):
    _, qc, dims, export = _model("synth_ds0.5")
    nl, P = dims["n_layers"], dims["P"]
    cm = cref.CModel(export)
    scales = (1.0, 0.25)
    parts = [_input(qc, dims, B, L, seed=610 + g, scale=scales[g]) for g in range(G)]
    state = np.zeros((G, nl, 2, B, P), dtype=I32)
    if carry:
        for g in range(G):   # what a first chunk of 19 frames leaves behind
            first = _input(qc, dims, B, 19, seed=620 + g, scale=scales[g])
            cm.forward(first.data, first.bits, first.exp, state=state[g])
    s_in = state.copy() if carry else None
    refs = [cm.forward(parts[g].data, parts[g].bits, parts[g].exp, trace=True, state=state[g] if carry else None) for g in range(G)]
    _run_four(export, dims, parts, B, L, G, refs, carry_refs=state if carry else None, s_in=s_in)


@pytest.mark.gpu
def test_a_ragged_tail_behind_a_burst_stays_out_of_the_extremes():
    """One sequence of 70 frames (two steps of its last 4-step block are padding, its last gate tile holds 6 frames) that ends on
    a burst: what the kernels compute for the padded steps keeps growing, and the rows of the last tile beyond its 6 frames
    hold whatever was there.  Neither may reach the extremes: outputs and status words are the oracle's on all four engines."""
    B, L = 1, 70
    _, qc, dims, export = _model("synth_ds0.5")
    xf = synth.make_input(B, L, dims["d_in"], seed=8)
    xf[:, -1, :] *= 400.0                                      # the burst: saturates Bu in the last frame
    fx = O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    refs = [cref.CModel(export).forward(fx.data, fx.bits, fx.exp, trace=True)]
    _run_four(export, dims, [fx], B, L, 1, refs)


@pytest.mark.gpu
@pytest.mark.parametrize("io", ["float", "int16"])
def test_float_and_int16_boundaries_take_the_route(io):
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine

    B, L = 2, 70
    _, qc, dims, export = _model("synth_ds0.5")
    nl = dims["n_layers"]
    fx = _input(qc, dims, B, L, seed=630, scale=1.0)
    ref, rb, re_, rtr = cref.CModel(export).forward(fx.data, fx.bits, fx.exp, trace=True)
    if io == "float":
        xin = torch.from_numpy(synth.make_input(B, L, dims["d_in"], seed=630, scale=1.0).astype(np.float32)).cuda()
        want = np.ldexp(ref.astype(np.float32), -re_).astype(np.float32)
    else:
        assert fx.bits <= 16 and ref.min() >= -32768 and ref.max() <= 32767
        xin = torch.from_numpy(fx.data.astype(np.int16)).cuda()
        want = ref.astype(np.int16)
    got, words = {}, {}
    for eng_name, flags in (("gate_ext", 0), ("reading", _lib.MODEL_NO_GATE_EXT)):
        eng = Engine(export, flags=flags)
        out = {}
        kernels = _profiled(lambda: out.update(y=eng.forward_float(xin) if io == "float" else eng.forward_int16(xin)))
        _check_launches(eng_name, kernels, nl, 1, many_frames=True)
        got[eng_name] = out["y"].cpu().numpy()
        assert got[eng_name].dtype == want.dtype and np.array_equal(got[eng_name], want), (eng_name, np.count_nonzero(got[eng_name] != want))
        st = eng.lane_status(0).cpu().numpy()
        assert st[2] == _lib.PATH_FUSED and not (st[0] & (_lib.ST_REDO | _lib.ST_NEGSHIFT | _lib.ST_NEGEXP)), (eng_name, st[:8])
        assert [int(st[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in rtr], eng_name
        words[eng_name] = st[8:8 + 8 * nl].copy()
    assert got["gate_ext"].tobytes() == got["reading"].tobytes()
    assert np.array_equal(words["gate_ext"], words["reading"])
