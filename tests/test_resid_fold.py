"""resid_fold: the gate kernel stores the residual add's aligned sum U = max(sat16(z << shx) + sat16(skip << shy), 0)
as uint16 where z went, and the residual pass / the decoder's fused residual read that one plane: h = min(shift(U, post), 32767).

  * CPU: a NumPy restatement of U and of the resolve map against oracle.fxp_oracle add(.., "compute_best") + relu on the
    oracle's own traces of the dim 0.5 synthetic model, and against the oracle's primitives on the whole shift / rail grid;
  * GPU probe (tools/probe_resid_u16.hip): the device helpers against scalar add_cb_apply + ReLU, every operand pair;
  * GPU parity: outputs and status words against the C oracle and against an engine created with MODEL_NO_RESID_FOLD, on a
    grouped call whose groups give the residual add different exponents, with a carry, at the other dim_scales and on the
    contract families; the inputs are shown (from the oracle's trace) to need 17 bits for the sum and both shift directions;
  * path checks: traced, exact and non-deferred forwards keep the two-plane kernels.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import contract_models as CM
from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = np.int32
CFG05 = dict(dim_scale=0.5, calib_L=1024, state_headroom_bits=1)   # bench.py's configs[1] model


# --------------------------------------------------------------------------------------------------------------------
# the restatement: what mfma_bn.hpp sum_u16_pair / resolve_u16 compute, in NumPy
# --------------------------------------------------------------------------------------------------------------------
def _sat16(v):
    return np.clip(v, -32768, 32767)


def np_usum(z, skip, ez, es):
    """U for z at exponent ez and skip >= 0 at exponent es (both within 16 bits); int64 arithmetic, no wrap to worry about."""
    ea = max(ez, es)
    a = _sat16(z.astype(np.int64) << (ea - ez)) if ea > ez else z.astype(np.int64)
    b = _sat16(skip.astype(np.int64) << (ea - es)) if ea > es else skip.astype(np.int64)
    u = np.maximum(a + b, 0)
    assert u.min() >= 0 and u.max() <= 65534
    return u


def np_resolve(u, post):
    v = (u << post) if post > 0 else (u >> -post)
    return np.minimum(v, 32767).astype(I32)


def oracle_h(z, skip, ez, es, post):
    """relu of the compute_best add for a GIVEN result shift, from the oracle's own primitives in the order of
    fxp_oracle.add's compute_best branch (change_cfg to the wider exponent clips at the operand's 16 bits)."""
    ea = max(ez, es)
    ac = O.change_exp(O.Fx(z.astype(I32), 16, ez), ea)
    bc = O.change_exp(O.Fx(skip.astype(I32), 16, es), ea)
    d = O.add32(ac.data, bc.data)
    d = O.shl(d, post) if post > 0 else O.asr(d, -post) if post < 0 else d
    return O.relu(O.Fx(O.sat(d, 16), 16, ea + post)).data


def _operands(rng, n):
    z = rng.integers(-32768, 32768, n).astype(I32)
    s = rng.integers(0, 32768, n).astype(I32)
    rails_z = np.array([-32768, -32767, -1, 0, 1, 32766, 32767], dtype=I32)
    rails_s = np.array([0, 1, 32766, 32767], dtype=I32)
    zz, ss = np.meshgrid(rails_z, rails_s)
    return np.concatenate([z, zz.ravel()]), np.concatenate([s, ss.ravel()])


def test_restatement_on_the_shift_and_rail_grid():
    """Every (shx, 0) and (0, shy) with shifts up to 15, post in -17 .. 15, random values and the rail values."""
    rng = np.random.Generator(np.random.PCG64(2026))
    z, s = _operands(rng, 4000)
    n = 0
    for sh in range(0, 16):
        for ez, es in ((0, sh), (sh, 0)):
            if sh == 0 and ez != es:
                continue
            u = np_usum(z, s, ez, es)
            for post in range(-17, 16):
                assert np.array_equal(np_resolve(u, post), oracle_h(z, s, ez, es, post)), (ez, es, post)
                n += z.size
    assert n > 4_000_000


def _np_traces(md, qc, dims, fx):
    m = O.RegressionModel(md, qc, dims["n_layers"])
    it = {}
    m(fx, it)
    return [it[f"layers_{i}"] for i in range(dims["n_layers"])]


def _fold_facts(layers):
    """Per layer: (shx, shy, post, max S) of the residual add, from the NumPy oracle's intermediates."""
    out = []
    for li in layers:
        z, skip, r = li["post_GLU"], li["ssm_input"], li["residadd"]
        assert z.bits == 16 and skip.bits == 16 and r.bits == 16 and skip.data.min() >= 0
        ea = max(z.exp, skip.exp)
        u = np_usum(z.data, skip.data, z.exp, skip.exp)
        out.append((ea - z.exp, ea - skip.exp, r.exp - ea, int(u.max())))
    return out


def _input(qc, dims, B, L, seed, scale):
    x = synth.make_input(B, L, dims["d_in"], seed=seed, scale=scale)
    return O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)


_SYNTH = {}


def _synth(**cfg):
    key = tuple(sorted(cfg.items()))
    if key not in _SYNTH:
        _SYNTH[key] = synth.make_model(**cfg)
    return _SYNTH[key]


def test_restatement_on_the_oracle_traces():
    """The oracle's compute_best add + relu of every layer of the dim 0.5 synthetic model (B = 2, L = 256, two input scales) is
    the resolve map of U, element for element, with the shifts the oracle's exponents imply."""
    md, qc, dims = _synth(**CFG05)
    layers = _np_traces(md, qc, dims, _input(qc, dims, 2, 256, seed=11, scale=1.0)) + \
        _np_traces(md, qc, dims, _input(qc, dims, 2, 256, seed=12, scale=2.0))
    posts, smax = [], 0
    for li, (shx, shy, post, top) in zip(layers, _fold_facts(layers)):
        z, skip = li["post_GLU"], li["ssm_input"]
        r = O.add(z, skip, 16, "compute_best")
        assert r.exp == li["residadd"].exp and np.array_equal(r.data, li["residadd"].data)
        u = np_usum(z.data, skip.data, z.exp, skip.exp)
        assert np.array_equal(np_resolve(u, post), O.relu(r).data)
        assert np.array_equal(np_resolve(u, post), li["output"].data)
        assert min(shx, shy) == 0
        posts.append(post)
        smax = max(smax, top)
    assert min(posts) < 0 < max(posts), posts
    assert smax > 32767   # a signed 16-bit sum plane would not do


# --------------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_helpers_equal_add_cb_apply(tmp_path):
    """tools/probe_resid_u16.hip: zero differences on every operand pair, every part ran in full."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "probe_resid_u16")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "probe_resid_u16.hip"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.split() and l.split()[0] in ("SUM", "RESOLVE", "CHAIN")]
    assert [l[0] for l in lines] == ["SUM", "RESOLVE", "CHAIN"], r.stdout
    assert int(lines[0][2]) >= 65536 * 32768 * 31 and int(lines[1][2]) == 65536 * 63
    for l in lines:
        assert int(l[2]) > 0 and int(l[4]) == 0, l


def _profiled(fn):
    """[(kernel name, grid)] of the library's kernels fn() launched, in order (torch.profiler)."""
    import json
    import tempfile
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "trace.json")
        prof.export_chrome_trace(path)
        with open(path) as f:
            ev = json.load(f)["traceEvents"]
    ks = sorted((e for e in ev if e.get("cat") == "kernel" and "s5::" in e.get("name", "")), key=lambda e: e["ts"])
    assert ks, "torch.profiler recorded no kernel of libs5fxp.so"
    return [(e["name"], tuple(e["args"]["grid"])) for e in ks]


def _targs(name):
    """'void s5::k_cgate_p<1, 3, false, ...>(...)' -> ('k_cgate_p', ['1', '3', 'false', ...])"""
    m = re.search(r"s5::(\w+)(?:<([^>]*)>)?\(", name)
    return m.group(1), [a.strip() for a in m.group(2).split(",")] if m.group(2) else []


def _forms(kernels):
    """(gate launches that store U, gate launches that store z, one-plane residual passes, two-plane ones) of a forward."""
    fold = sum(1 for n, _ in kernels if _targs(n)[0] == "k_cgate_p" and "CGateFoldArgs" in n)
    plain = sum(1 for n, _ in kernels if _targs(n)[0] == "k_cgate_p" and "CGateFoldArgs" not in n)
    r1 = sum(1 for n, _ in kernels if _targs(n) == ("k_resid_minmax16", ["true", "true"]))
    r2 = sum(1 for n, _ in kernels if _targs(n)[0] in ("k_resid_minmax16", "k_resid16")) - r1
    return fold, plain, r1, r2


G, B, L = 2, 2, 70          # two full 32-frame tiles and a 6-frame one; two groups
SCALES = (1.0, 0.25)

MODELS = {
    "synth_ds0.5": lambda: _synth(**CFG05),
    "synth_ds0.25": lambda: _synth(dim_scale=0.25, calib_L=256, state_headroom_bits=1),
    "synth_ds0.75": lambda: _synth(dim_scale=0.75, calib_L=256, state_headroom_bits=1),
}
CONTRACT = ["F1_full_ds0.5", "F2_rails_ds0.5", "F5_y+4_ds0.5", "F5_y+3_l-y14_ds0.5"]
# where gate_urec holds, the one-plane kernels must be seen to run: H = 96 and BatchNorm exponents from the per-channel extremes
# (the full-range contract families take the four-reduction route, and with it the two-plane kernels, group by group)
FOLDS = ("synth_ds0.5",)


def _model(name):
    if name in MODELS:
        md, qc, dims = MODELS[name]()
        from sparsernns_amd.fxpmodel import build_regression_model
        key = ("export", name)
        if key not in _SYNTH:
            _SYNTH[key] = build_regression_model(md, qc, dims["n_layers"]).export()
        return md, qc, dims, _SYNTH[key]
    c = CM.case(name)
    return c.md, c.qc, c.dims, c.export()


@pytest.mark.gpu
@pytest.mark.parametrize("name,carry", [(n, False) for n in list(MODELS) + CONTRACT] + [("synth_ds0.5", True)])
def test_grouped_forward_matches_oracle_and_the_two_plane_kernels(name, carry):
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine

    md, qc, dims, export = _model(name)
    nl, P = dims["n_layers"], dims["P"]
    cm = cref.CModel(export)
    parts = [_input(qc, dims, B, L, seed=410 + g, scale=SCALES[g]) for g in range(G)]
    bits, exp = parts[0].bits, parts[0].exp
    state = np.zeros((G, nl, 2, B, P), dtype=I32)
    if carry:
        for g in range(G):   # what a first chunk of 19 frames leaves behind
            first = _input(qc, dims, B, 19, seed=430 + g, scale=SCALES[g])
            cm.forward(first.data, first.bits, first.exp, state=state[g])
    s_in = state.copy()
    refs = [cm.forward(parts[g].data, bits, exp, trace=True, state=state[g] if carry else None) for g in range(G)]
    if name == "synth_ds0.5" and not carry:
        # the conditions that make this a test of the one-plane route: the sum needs 17 bits in some layer, both shift
        # directions of the result occur, and the groups' result shifts differ in some layer
        facts = [_fold_facts(_np_traces(md, qc, dims, parts[g])) for g in range(G)]
        print("residual add (shx, shy, post, max S) per group and layer:", facts)
        assert max(f[3] for f in facts[0]) > 32767, facts
        posts = [[f[2] for f in fg] for fg in facts]
        assert min(posts[0]) < 0 < max(posts[0]), posts
        assert posts[0] != posts[1], posts
    x = torch.from_numpy(np.concatenate([p.data for p in parts])).cuda()
    got = {}
    for eng_name, flags in (("fold", 0), ("two_plane", _lib.MODEL_NO_RESID_FOLD)):
        eng = Engine(export, flags=flags)
        assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
        y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        kw = {}
        if carry:
            kw = dict(state_in=torch.from_numpy(s_in).cuda(), state_out=torch.empty((G, nl, 2, B, P), dtype=torch.int32, device="cuda"))
        launch = lambda fl: eng.enqueue(x, bits, exp, y, B, L, flags=fl, groups=G, **kw)
        kernels = _profiled(lambda: launch(_lib.FWD_DEFER_REDO))
        st = eng.lane_status(0, G).cpu().numpy().copy()
        if any(int(st[g * _lib.STATUS_WORDS]) & _lib.ST_REDO for g in range(G)):
            # a state left the int16 rungs' range: the caller's ladder repeats the forward on a lower rung (include/s5fxp.h).
            # Not on the models this test is about: there the optimistic forward must be the one that is checked.
            assert name not in FOLDS, (name, eng_name, st[:8])
            eng.run_ladder(launch, eng.check_status)
            st = eng.lane_status(0, G).cpu().numpy().copy()
        fold, plain, r1, r2 = _forms(kernels)
        if eng_name == "fold" and name in FOLDS:
            assert (fold, plain, r1, r2) == (nl, 0, nl - 1, 0), (name, fold, plain, r1, r2)
        else:   # (a model off the per-channel-extremes method runs group by group, its last residual pass a launch of its own)
            assert (fold, r1) == (0, 0) and (plain, r2) in ((nl, nl - 1), (G * nl, G * nl)), (name, eng_name, fold, plain, r1, r2)
        yy = y.cpu().numpy().reshape(G, B, L, -1)
        for g in range(G):
            ref, rb, re_, rtr = refs[g]
            w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
            assert w[2] == _lib.PATH_FUSED and not (w[0] & (_lib.ST_REDO | _lib.ST_NEGSHIFT | _lib.ST_NEGEXP)), (name, eng_name, w[:8])
            assert (eng.out_bits, eng.out_exp) == (rb, re_)
            assert np.array_equal(yy[g], ref), (name, eng_name, g, np.count_nonzero(yy[g] != ref))
            assert [int(w[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in rtr], (name, eng_name, g)
        if carry:
            assert np.array_equal(kw["state_out"].cpu().numpy(), state), eng_name
        got[eng_name] = (yy, st)
    assert np.array_equal(got["fold"][0], got["two_plane"][0])
    for g in range(G):       # every per-layer status word [8 + 8l + 0..7], group by group
        a = got["fold"][1][g * _lib.STATUS_WORDS + 8:g * _lib.STATUS_WORDS + 8 + 8 * nl]
        b = got["two_plane"][1][g * _lib.STATUS_WORDS + 8:g * _lib.STATUS_WORDS + 8 + 8 * nl]
        assert np.array_equal(a, b), (name, g, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["traced", "exact", "in_forward_rerun"])
def test_other_forwards_keep_the_two_plane_kernels(route):
    """A traced forward, an S5FXP_FWD_EXACT forward and a non-deferred forward (its in-forward exact re-run would store a plain z)
    launch no kernel of the one-plane route and match the oracle."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine
    from sparsernns_amd.fxparray import FxpArray

    md, qc, dims, export = _model("synth_ds0.5")
    nl = dims["n_layers"]
    fx = _input(qc, dims, B, L, seed=410, scale=1.0)
    ref, rb, re_, rtr = cref.CModel(export).forward(fx.data, fx.bits, fx.exp, trace=True)
    eng = Engine(export)
    if route == "traced":
        out = {}
        kernels = _profiled(lambda: out.update(r=eng.forward(FxpArray(fx.data, fx.bits, fx.exp), traces=True)))
        y, tr = out["r"]
        got = y.numpy()
        for i in range(nl):
            assert np.array_equal(tr[i]["residadd"].cpu().numpy(), rtr[i]["residadd"]), i
        st = eng.status.cpu().numpy()
    else:
        x = torch.from_numpy(fx.data).cuda()
        y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        flags = _lib.FWD_EXACT if route == "exact" else 0
        kernels = _profiled(lambda: eng.enqueue(x, fx.bits, fx.exp, y, B, L, flags=flags))
        got = y.cpu().numpy()
        st = eng.lane_status(0).cpu().numpy()
    fold, plain, r1, r2 = _forms(kernels)
    assert fold == 0 and r1 == 0 and plain >= nl and r2 >= nl - 1, (route, fold, plain, r1, r2)
    assert np.array_equal(got, ref), np.count_nonzero(got != ref)
    assert [int(st[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in rtr]


@pytest.mark.gpu
def test_float_forward_reads_the_one_plane_in_its_decoder():
    """The float-in, float-out forward (k_enc_pf / k_dec_pf): its decoder takes the one-plane route as well, and gives the bits
    of the two-plane engine and of the oracle's integers converted to float."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine

    md, qc, dims, export = _model("synth_ds0.5")
    nl = dims["n_layers"]
    xf = synth.make_input(B, L, dims["d_in"], seed=410, scale=1.0).astype(np.float32)
    fx = _input(qc, dims, B, L, seed=410, scale=1.0)
    ref, rb, re_, _ = cref.CModel(export).forward(fx.data, fx.bits, fx.exp)
    want = np.ldexp(ref.astype(np.float32), -re_).astype(np.float32)
    got = {}
    for eng_name, flags in (("fold", 0), ("two_plane", _lib.MODEL_NO_RESID_FOLD)):
        eng = Engine(export, flags=flags)
        out = {}
        kernels = _profiled(lambda: out.update(y=eng.forward_float(torch.from_numpy(xf).cuda())))
        fold, plain, r1, r2 = _forms(kernels)
        decs = [_targs(n) for n, _ in kernels if _targs(n)[0] in ("k_dec_p", "k_dec_pf")]
        assert decs == [("k_dec_pf", ["3", "true"])], decs
        assert (fold, plain, r1, r2) == ((nl, 0, nl - 1, 0) if eng_name == "fold" else (0, nl, 0, nl - 1)), (eng_name, fold, plain, r1, r2)
        got[eng_name] = out["y"].cpu().numpy()
        assert got[eng_name].dtype == np.float32 and np.array_equal(got[eng_name], want), (eng_name, np.count_nonzero(got[eng_name] != want))
    assert np.array_equal(got["fold"], got["two_plane"])
