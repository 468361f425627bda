"""The 32-frame UREC gate kernels at 32 state slots (mfma_fused_body.inc EARLY) request a tile's states in front of the staging,
wait for them by count behind a full previous tile and drained elsewhere, and map phase A over the live state slots (the columns
of the dead ones are written once).  Everything here is bit-exact against the C oracle on dim_scale 0.5 synthetic models, with a
deferred forward on the fold route, and every case reads from the launches and the status words that the kernel under test ran:
the fused path, the int16 rung asked for, the stream slots expected, three folding gate launches of the form <1, 3, .., 32, ..,
UREC>.

  * tile walks: S5FXP_WGS_CGATE32 caps the gate kernel's workgroups, so that one workgroup walks many tiles across sequence
    boundaries: a first tile alone, a partial tile followed by a full one (drained, then counted), a last 4-step block beyond L;
  * live slots: 4, 20, 22, 24, 26 and 32 live states per layer (rows of the exported B_bar zeroed or set), on both int16 rungs;
  * two groups with different exponents in one launch;
  * the range check: a state beyond the bound raises ST_REDO from the last live slot, from a workgroup's first tile and from a
    last partial tile behind a full one; a burst on the last frame of a sequence whose last block is mostly padding does not;
  * the compiled kernels hold the stores the hand-written wait counts (tools/check_vmwait.py; no GPU).
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import contract_models as CM
from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth
from test_resid_fold import _input, _model, _profiled, _targs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "synth_ds0.5"
_CACHE = {}


def _export_live(n):
    """The synthetic model's export with n live states in every layer (None: as it is, 20 / 19 / 21): the last live rows of the
    8-bit B_bar zeroed, or the first dead rows given one entry of 1."""
    _, qc, dims, export = _model(NAME)
    if n is None:
        return export
    if ("live", n) not in _CACHE:
        ex = copy.deepcopy(export)
        for i, live in enumerate(CM.export_live(export, dims["n_layers"])):
            m = ex["params"]["encoder"][f"layers_{i}"]["mixer"]
            br, bi = np.array(m["B_real"]), np.array(m["B_imag"])
            dead = np.setdiff1d(np.arange(dims["P"]), live)
            br[live[n:]] = 0
            bi[live[n:]] = 0
            br[dead[:max(0, n - len(live))], 0] = 1
            m["B_real"], m["B_imag"] = br, bi
        assert [len(v) for v in CM.export_live(ex, dims["n_layers"])] == [n] * dims["n_layers"]
        _CACHE[("live", n)] = ex
    return _CACHE[("live", n)]


def _oracle(key, export, parts):
    """The C oracle's traced forward of every group, computed once per (model, inputs)."""
    key = ("oracle",) + key
    if key not in _CACHE:
        cm = cref.CModel(export)
        _CACHE[key] = [cm.forward(p.data, p.bits, p.exp, trace=True) for p in parts]
    return _CACHE[key]


def _engine(export, cap, monkeypatch):
    from sparsernns_amd.engine import Engine
    if cap is not None:
        monkeypatch.setenv("S5FXP_WGS_CGATE32", str(cap))   # read when the model is created
    eng = Engine(export)
    monkeypatch.delenv("S5FXP_WGS_CGATE32", raising=False)
    return eng


def _forward(eng, export, dims, parts, B, L, pair=True):
    """One deferred grouped forward: (outputs per group, status words per group), after the checks that the kernels under test ran."""
    import torch
    from sparsernns_amd import _lib

    nl, P, G = dims["n_layers"], dims["P"], len(parts)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    x = torch.from_numpy(np.concatenate([p.data for p in parts])).cuda()
    y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
    flags = _lib.FWD_DEFER_REDO | (0 if pair else _lib.FWD_NO_PAIR)
    kernels = _profiled(lambda: eng.enqueue(x, parts[0].bits, parts[0].exp, y, B, L, flags=flags, groups=G))
    gates = [_targs(n)[1] for n, _ in kernels if _targs(n)[0] == "k_cgate_p"]
    folds = [n for n, _ in kernels if _targs(n)[0] == "k_cgate_p" and "CGateFoldArgs" in n]
    want = ["1", "3", "false", "true", "true", "32", "false", "true" if pair else "false", "true", "false", "true"]
    assert len(folds) == nl and gates == [want] * nl, gates
    st = eng.lane_status(0, G).cpu().numpy().copy()
    live = [len(v) for v in CM.export_live(export, nl)]
    words = []
    for g in range(G):
        w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
        assert w[2] == _lib.PATH_FUSED, w[:8]
        assert [int(w[8 + 8 * i + 5]) for i in range(nl)] == [4 if pair else 2] * nl, w[8:8 + 8 * nl]
        assert [int(w[8 + 8 * i + 6]) for i in range(nl)] == [32] * nl, w[8:8 + 8 * nl]
        assert [int(w[8 + 8 * i + 7]) for i in range(nl)] == [CM.stream_slots(n, P, True) for n in live], (w[8:8 + 8 * nl], live)
        words.append(w)
    return y.cpu().numpy().reshape(G, B, L, -1), words


def _check_exact(eng, outs, words, refs, nl):
    from sparsernns_amd import _lib
    for g, (ref, rb, re_, rtr) in enumerate(refs):
        assert not (words[g][0] & (_lib.ST_REDO | _lib.ST_NEGSHIFT | _lib.ST_NEGEXP)), (g, words[g][:8])
        assert (eng.out_bits, eng.out_exp) == (rb, re_)
        assert np.array_equal(outs[g], ref), (g, np.count_nonzero(outs[g] != ref))
        assert [int(words[g][8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in rtr], g


# --------------------------------------------------------------------------------------------------------------------
# tile walks
# --------------------------------------------------------------------------------------------------------------------
# cap 4, sequences of 1 .. 4 tiles: L <= 32 one (partial or full) tile per sequence, so that with B = 3 a workgroup's tiles are
# all first tiles; L = 33, 65, 100: a workgroup goes from a partial last tile to a full one (drained) and from a full one to a
# full or partial one (counted); L = 1, 3, 33, 65: the last 4-step block reaches beyond L.  None: the default cap.
WALKS = [(4, B, L) for L in (1, 3, 31, 32, 33, 65, 100) for B in (1, 3)] + [(None, 3, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("cap,B,L", WALKS)
def test_tile_walks_match_the_oracle(cap, B, L, monkeypatch):
    _, qc, dims, export = _model(NAME)
    parts = [_input(qc, dims, B, L, seed=700 + L, scale=1.0)]
    refs = _oracle(("walk", B, L), export, parts)
    eng = _engine(export, cap, monkeypatch)
    outs, words = _forward(eng, export, dims, parts, B, L)
    _check_exact(eng, outs, words, refs, dims["n_layers"])


# --------------------------------------------------------------------------------------------------------------------
# live slots: PL = 4 (its minimum), 20, 24 (from 22 and from 24: the one-round edge), 28 (two rounds), and every slot (32)
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pair", [True, False], ids=["pair", "quad16"])
@pytest.mark.parametrize("n_live", [4, 20, 22, 24, 26, 32])
def test_live_slot_counts_match_the_oracle(n_live, pair, monkeypatch):
    _, qc, dims, _ = _model(NAME)
    export = _export_live(n_live)
    B, L = 3, 70
    parts = [_input(qc, dims, B, L, seed=720, scale=1.0)]
    refs = _oracle(("live", n_live), export, parts)
    eng = _engine(export, 2, monkeypatch)
    outs, words = _forward(eng, export, dims, parts, B, L, pair=pair)
    _check_exact(eng, outs, words, refs, dims["n_layers"])


# --------------------------------------------------------------------------------------------------------------------
# groups
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_groups_with_different_exponents(monkeypatch):
    _, qc, dims, export = _model(NAME)
    B, L = 2, 70
    parts = [_input(qc, dims, B, L, seed=730 + g, scale=s) for g, s in enumerate((1.0, 0.25))]
    refs = _oracle(("groups",), export, parts)
    assert any(a[3][i]["residadd_exp"] != b[3][i]["residadd_exp"] for a, b in [refs] for i in range(dims["n_layers"]))
    eng = _engine(export, 3, monkeypatch)
    outs, words = _forward(eng, export, dims, parts, B, L)
    _check_exact(eng, outs, words, refs, dims["n_layers"])


# --------------------------------------------------------------------------------------------------------------------
# the range check
# --------------------------------------------------------------------------------------------------------------------
def _state_tops(rtr, B, L):
    """Per layer |state| maxima of the oracle's trace as (B, L, P)."""
    return [np.maximum(np.abs(t["xs_re"]), np.abs(t["xs_im"])).reshape(B, L, -1) for t in rtr]


def _bounds(eng, nl):
    from sparsernns_amd import _lib
    return [int(_lib.lib.s5fxp_model_recurrence_xmax(eng._h, i)) for i in range(nl)]


def _burst(qc, dims, B, L, frames, seed=8):
    xf = synth.make_input(B, L, dims["d_in"], seed=seed)
    xf[0, frames, :] *= 400.0
    return O.from_fp(xf, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [True, False], ids=["pair", "quad16"])
@pytest.mark.parametrize("place", ["last_live_slot", "first_tile", "last_partial_tile"])
def test_a_state_beyond_the_bound_raises_redo(place, pair, monkeypatch):
    """Where the oracle's states pass 32767 (beyond every bound an int16 stream can have) in ONE place and stay within the
    kernels' bound everywhere else, the deferred forward reports ST_REDO.
    last_live_slot: the last live state of the last layer, its row of B_bar at full scale (cap 2: three tiles per workgroup).
    first_tile: B = 3, L = 32, cap 2: workgroup 0 walks the tiles of sequences 0 and 2; sequence 0 is loud.
    last_partial_tile: B = 3, L = 100, cap 3: workgroup 0 walks (sequence 0, t = 0) and then the 4-frame tile of sequence 0,
    whose frames are loud: the counted wait in front of a partial tile."""
    from sparsernns_amd import _lib
    _, qc, dims, export = _model(NAME)
    nl, P = dims["n_layers"], dims["P"]
    if place == "last_live_slot":
        B, L, cap = 3, 70, 2
        if "lastslot" not in _CACHE:
            ex = copy.deepcopy(export)
            m = ex["params"]["encoder"][f"layers_{nl - 1}"]["mixer"]
            last = CM.export_live(export, nl)[nl - 1][-1]
            br, bi = np.array(m["B_real"]), np.array(m["B_imag"])
            br[last, :], bi[last, :] = 127, 127
            m["B_real"], m["B_imag"] = br, bi
            _CACHE["lastslot"] = (ex, last)
        export, last = _CACHE["lastslot"]
        parts = [_input(qc, dims, B, L, seed=740, scale=1.0)]
    elif place == "first_tile":
        B, L, cap = 3, 32, 2
        parts = [_burst(qc, dims, B, L, slice(0, L))]
    else:
        B, L, cap = 3, 100, 3
        parts = [_burst(qc, dims, B, L, slice(96, 100))]
    tops = _state_tops(_oracle(("redo", place), export, parts)[0][3], B, L)
    eng = _engine(export, cap, monkeypatch)
    bounds = _bounds(eng, nl)
    loud = [np.zeros((B, L, P), dtype=bool) for _ in range(nl)]
    for li in range(nl):
        if place == "last_live_slot":
            loud[li][:, :, last] = li == nl - 1
        elif place == "first_tile":
            loud[li][0] = True
        else:
            loud[li][0, 96:] = True
    assert max(int(t[m].max()) for t, m in zip(tops, loud) if m.any()) > 32767
    for li in range(nl):   # ... and nowhere else is a state beyond the bound the kernels check
        assert int(tops[li][~loud[li]].max()) <= bounds[li], (place, li, int(tops[li][~loud[li]].max()), bounds[li])
    _, words = _forward(eng, export, dims, parts, B, L, pair=pair)
    assert words[0][0] & _lib.ST_REDO, (place, words[0][:8])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [True, False], ids=["pair", "quad16"])
def test_padded_steps_stay_out_of_the_range_check(pair, monkeypatch):
    """L = 97: three of the four steps of every sequence's last block are padding.  Sequence 0 ends on a burst that lifts its
    states by about a quarter of the 16-bit range in its one valid step; the recurrence runs on through the padded steps from
    whatever the stream holds there.  The valid states are within the bound, so no ST_REDO, and the outputs are the oracle's."""
    _, qc, dims, export = _model(NAME)
    nl = dims["n_layers"]
    B, L = 3, 97
    parts = [_burst(qc, dims, B, L, slice(L - 1, L))]
    refs = _oracle(("padded",), export, parts)
    eng = _engine(export, 3, monkeypatch)
    tops, bounds = _state_tops(refs[0][3], B, L), _bounds(eng, nl)
    assert any(int(t[0, L - 1].max()) > 4 * int(t[0, :L - 1].max()) for t in tops)   # the burst is there ...
    assert all(int(t.max()) <= b for t, b in zip(tops, bounds)), ([int(t.max()) for t in tops], bounds)   # ... within the bound
    outs, words = _forward(eng, export, dims, parts, B, L, pair=pair)
    _check_exact(eng, outs, words, refs, nl)


# --------------------------------------------------------------------------------------------------------------------
# the compiled code (no GPU)
# --------------------------------------------------------------------------------------------------------------------
def test_the_compiled_kernels_hold_the_stores_the_waits_count():
    """tools/check_vmwait.py --gate: the four gate kernels that request their states early, compiled alone from the library's
    headers (tests/test_cpu_suite.py runs the tool on the whole library): the register audit of the hidden loads, zero scratch,
    and NVC = 2 16-byte stores per staging copy between the last request and the two waits."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_vmwait.py"), "--gate"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    gate = [l for l in r.stdout.splitlines() if "k_cgate_p" in l and "hidden loads" in l]
    assert len(gate) == 4 and all("private_segment_fixed_size 0" in l and l.endswith(": ok") for l in gate), r.stdout
    assert r.stdout.count("expected 3 arms x 2") == 4 and "MISMATCH" not in r.stdout, r.stdout
