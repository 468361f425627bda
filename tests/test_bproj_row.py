"""The B projection whose phase A runs the gate kernel's row chain (k_bproj_p<.., ROW>: mfma_bn.hpp bn16_row8 on the 16-byte row
vectors as loaded, u and the byte planes from the packed pairs) against the C oracle, beside the kernels that keep bn16_x4
(S5FXP_GATE_BN=2):

  * the variant matrix's H = 96 workloads (its w4a8 one included) under all four forward flag sets, bench.py's model at input scales that move the
    BatchNorm shifts, and one model of every contract family at dim_scale 0.5 (3 x 333: five full 64-frame tiles and a 13-frame
    one, L % 4 = 1; 33 x 1: single frames; a lazy and a plain layer input in every forward): outputs, output exponents, per-layer
    exponents and the carry are the oracle's, on both engines.  With flags 0 the overflowing input is re-run inside the forward by
    kernels that read u from memory, so the ROW kernel's u store is what they read;
  * the kernels a DEFER_REDO forward launched (torch.profiler): ROW (the sixth template argument) is true on every k_bproj_p
    launch of a model without a BatchNorm scale / bias stage, false for F_bnsb, under the switch and on a traced forward, and
    arguments 0-4 are the ones the other engine launches;
  * which arm of bn16_row8 a layer takes depends on exponents the device derives.  bn16_row_arm is restated here and every
    layer's arm is derived from the oracle's trace of each case (no GPU): together the cases reach ROW_PACKED, ROW_SHIFTED and
    ROW_GENERIC, and every GPU case asserts that the arms it was chosen for are the ones its inputs give;
  * no k_bproj_p instantiation uses scratch memory (tools/kernel_resources.py, no GPU) -- the two bn16_x4 kernels of the
    uncompacted H = 192 layer on the pair streams spilled 20 bytes per lane before; their prefetch forms its row offsets per
    tile now (proj_p.hpp REFETCH).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import contract_models as CM
from oracle import fxp_oracle as O
from test_gate_urec import CONTRACT, H96, _bproj_stores_u, _flag_sets, _make_engine
from test_variant_matrix import CFG1, _input, _launched, _model, _pre_s5_word, _profiled, _work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = {"default": {}, "no_bproj_row": {"S5FXP_GATE_BN": "2"}}
ROW_GENERIC, ROW_PACKED, ROW_SHIFTED = 0, 1, 2
ARM_NAMES = {ROW_GENERIC: "ROW_GENERIC", ROW_PACKED: "ROW_PACKED", ROW_SHIFTED: "ROW_SHIFTED"}
# bench.py's configs[1] model (A_ragged's) at 3 x 333 under other input scales: DESIGN.md 4a has r1 = 0 .. 4 over 0.25 .. 6
SCALES = (0.25, 6.0)
# ... and the variant matrix's w4a8 workload, whose BatchNorm widths are 8 bits: no contract family has a width other than 16
# there, so this is the case that takes the chain's third arm (ROW_GENERIC)
MATRIX = H96 + ("E_w4a8",)


# ---- the arm a layer's B projection takes, from the oracle alone
def bn16_row_arm(xb, mb, ib, b1, b2, cbits, shx1, l1, r1, cl, cr):
    """mfma_bn.hpp bn16_row_arm."""
    w16 = ((xb == 16 or (shx1 == 0 and xb < 16)) and mb <= 16 and ib <= 16 and b1 == 16 and b2 == 16 and cbits == 16 and
           shx1 <= 14 and l1 == 0 and cl <= 14 and cr <= 15)
    return ROW_GENERIC if not w16 else ROW_PACKED if r1 == 0 else ROW_SHIFTED


def _encoder_output(export, x, bits, exp):
    """relu(encoder(x)) from the export's integers (oracle/fxp_oracle.py Dense)."""
    p, q = export["params"]["encoder"]["encoder"], export["qconfig"]["encoder"]["encoder"]
    d = O.Dense.__new__(O.Dense)
    d.qc = dict(inp_bits=int(q["inp_bits"]), inp_exp=int(q["inp_exp"]), out_bits=int(q["out_bits"]), out_exp=int(q["out_exp"]))
    d.weight = O.Fx(np.asarray(p["weight"]).astype(np.int32), int(q["weight_bits"]), int(q["weight_exp"]), True)
    d.bias = None if p.get("bias") is None else O.Fx(np.asarray(p["bias"]).astype(np.int32), int(q["bias_bits"]), int(q["bias_exp"]), True)
    return O.relu(d(O.Fx(np.asarray(x, dtype=np.int32), bits, exp, True)))


def layer_arms(export, x, bits, exp, rtr):
    """[arm of layer i's B projection], from the model, the input and the oracle's trace: the exponents the B projection's
    prologue derives (mfma_bn.hpp bn_finalize_mm_body, s5fxp_kernels.hpp finalize_add_cb) restated with the oracle's float32
    rules, the widths as s5fxp_api.hip bn_args sets them.  None for a layer with a BatchNorm scale / bias stage (no ROW).  The
    restatement is checked on the way: the chain with the derived shifts gives the trace's pre_s5."""
    arms = []
    h = _encoder_output(export, x, bits, exp)
    for i, t in enumerate(rtr):
        n, nq = export["params"]["encoder"][f"layers_{i}"]["norm"], export["qconfig"]["encoder"][f"layers_{i}"]["norm"]
        mq, lq = export["qconfig"]["encoder"][f"layers_{i}"]["mixer"], export["qconfig"]["encoder"][f"layers_{i}"]["multgate"]
        if "scale" in n or "bias" in n:
            arms.append(None)
        else:
            xb, xe = h.bits, h.exp
            mb, me, ib, ie = int(nq["mean_bits"]), int(nq["mean_exp"]), int(nq["invsq_var_bits"]), int(nq["invsq_var_exp"])
            b1 = max(xb, mb)
            b2 = max(b1, ib)
            m = O.Fx((-np.asarray(n["mean"], dtype=np.int64)).astype(np.int32), mb, me, True)
            isv = np.asarray(n["invsq_var"]).astype(np.int32)
            eo1 = b1 - O.intbits_f32(np.abs((h.f32() + m.f32()).astype(np.float32)).max(), 1e-6) - 1
            ea = max(xe, me)
            shx, shy, post = ea - xe, ea - me, eo1 - ea
            l1, r1 = max(post, 0), max(-post, 0)
            e2 = int(t["pre_s5_exp"])
            rs2, de = eo1 + ie - e2, int(mq["u_exp"]) - e2
            assert rs2 >= 0
            v = O.sat(O.asr(O.shl(O.add32(O.sat(O.shl(h.data, shx), xb), O.sat(O.shl(m.data, shy), mb)), l1), r1), b1)
            assert np.array_equal(O.sat(O.asr(O.mul32(v, isv), rs2), b2), t["pre_s5"]), f"layer {i}: the restated chain is not the oracle's"
            arms.append(bn16_row_arm(xb, mb, ib, b1, b2, min(b2, int(mq["u_bits"])), shx, l1, r1, max(de, 0), max(-de, 0)))
        h = O.Fx(np.maximum(t["residadd"], 0).astype(np.int32), int(lq["res_bits"]), int(t["residadd_exp"]), True)
    return arms


_CASES = {}


def _scaled(scale):
    """bench.py's configs[1] model on 3 x 333 frames at another input scale."""
    key = ("scale", scale)
    if key not in _CASES:
        qc, dims, export, cm = _model(CFG1)
        fx = _input(qc, dims, 3, 333, seed=344, scale=scale)
        ref, rb, re_, rtr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
        _CASES[key] = dict(dims=dims, export=export, x=fx.data, bits=fx.bits, exp=fx.exp, ref=ref, out=(rb, re_), rtr=rtr)
    return _CASES[key]


def _contract(name):
    """[(kind, x, bits, exp, ref, (rb, re), rtr)] of a contract family's two inputs."""
    key = ("contract", name)
    if key not in _CASES:
        c = CM.case(name)
        cm = c.c_oracle()
        rows = []
        for kind in ("ndns", "flip"):
            x, bits, exp = CM.input_for(c, kind, 3, 333, seed=333)
            ref, rb, re_, rtr = cm.forward(x, bits, exp, trace=True)
            rows.append((kind, x, bits, exp, ref, (rb, re_), rtr))
        _CASES[key] = (c, rows)
    return _CASES[key]


def arms_of_every_case():
    """{case id: set of arms its layers take} over everything the GPU tests below run."""
    out = {}
    for w in MATRIX:
        work = _work(w)
        if w == "C_grouped":
            continue   # three groups of A_ragged's model with a carry: their trace is not kept; not counted
        out[w] = set(layer_arms(work["export"], work["x"], work["bits"], work["exp"], work["rtr"]))
    for s in SCALES:
        c = _scaled(s)
        out[f"scale{s}"] = set(layer_arms(c["export"], c["x"], c["bits"], c["exp"], c["rtr"]))
    for name in CONTRACT:
        c, rows = _contract(name)
        out[name] = set()
        for kind, x, bits, exp, ref, o, rtr in rows:
            out[name] |= set(layer_arms(c.export(), x, bits, exp, rtr))
    return out


# what the cases were chosen for (asserted: if a model or an input generator changes, the coverage must be re-established)
WANT_ARMS = {"scale0.25": {ROW_PACKED}, "scale6.0": {ROW_SHIFTED}, "E_w4a8": {ROW_GENERIC}}


def test_cases_reach_every_arm():
    arms = arms_of_every_case()
    print({k: sorted(ARM_NAMES[a] for a in v if a is not None) for k, v in arms.items()})
    reached = set().union(*arms.values())
    assert {ROW_PACKED, ROW_SHIFTED, ROW_GENERIC} <= reached, arms
    for k, want in WANT_ARMS.items():
        assert want <= arms[k], (k, arms[k])
    assert arms["F_bnsb"] == {None}


# ---- launched kernels
def _bprojs(kernels):
    return [a for a, _ in _launched(kernels, "k_bproj_p")]


def _check_rows(kernels, row_ok, nl, what):
    """Every k_bproj_p launch of the forward: six template arguments, H = 96's tile and wave counts, untraced, ROW as promised.
    Returns arguments 0-4 of the launches."""
    bp = _bprojs(kernels)
    assert len(bp) >= nl, (what, bp)
    for a in bp:
        assert len(a) == 6 and a[:3] == ["3", "4", "false"], (what, a)
        assert a[5] == ("true" if row_ok else "false"), (what, a)
    return [a[:5] for a in bp]


_HEADS = {}   # (case, flags) -> arguments 0-4 per launch, as the first engine that ran the case launched them


def _same_heads(case, heads):
    """Arguments 0-4 do not depend on the engine: the bn16_x4 engine launches what the parent launches."""
    assert _HEADS.setdefault(case, heads) == heads, (case, _HEADS[case], heads)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("wname", MATRIX)
def test_matrix_workloads_under_every_flag_set(wname, engine, monkeypatch):
    import torch
    from sparsernns_amd import _lib

    work = _work(wname)
    dims, B, L, G = work["dims"], work["B"], work["L"], work["G"]
    nl = dims["n_layers"]
    if wname in WANT_ARMS:
        assert WANT_ARMS[wname] <= set(layer_arms(work["export"], work["x"], work["bits"], work["exp"], work["rtr"]))
    eng = _make_engine(work["export"], ENGINES[engine], monkeypatch)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    assert (eng.out_bits, eng.out_exp) == work["out"]
    row_ok = engine == "default" and not _bproj_stores_u(work["export"])
    pre_words = [_pre_s5_word(work["export"], i) for i in range(nl)]
    x = torch.from_numpy(work["x"]).cuda()
    grouped = wname == "C_grouped"
    s_in = torch.from_numpy(work["state_in"]).cuda() if grouped else None
    for flags in _flag_sets():
        y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        s_out = torch.empty_like(s_in) if grouped else None
        if grouped:
            run = lambda: eng.enqueue(x, work["bits"], work["exp"], y, B, L, flags=flags, groups=G, state_in=s_in, state_out=s_out)
        else:
            run = lambda: eng.enqueue(x, work["bits"], work["exp"], y, B, L, flags=flags)
        kernels, _ = _profiled(run)
        st = eng.lane_status(0, G).cpu().numpy()
        redo = any(int(st[g * _lib.STATUS_WORDS]) & _lib.ST_REDO for g in range(G))
        _same_heads((wname, flags), _check_rows(kernels, row_ok, nl, (wname, engine, flags)))
        if wname == "G_overflow":
            assert redo == bool(flags & _lib.FWD_DEFER_REDO), (flags, st[:8])
        assert not redo or flags & _lib.FWD_DEFER_REDO, (wname, flags)
        if redo:
            continue
        got = y.cpu().numpy()
        assert np.array_equal(got, work["ref"]), (wname, engine, flags, np.count_nonzero(got != work["ref"]))
        for g in range(G):
            w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
            assert w[2] == _lib.PATH_FUSED
            if grouped:
                assert [int(w[8 + 8 * i + 4]) for i in range(nl)] == work["res_exps"][g], (flags, g)
            else:
                rtr = work["rtr"]
                assert [int(w[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in rtr], flags
                assert [int(w[8 + 8 * i + pre_words[i]]) for i in range(nl)] == [t["pre_s5_exp"] for t in rtr], flags
        if grouped:
            assert np.array_equal(s_out.cpu().numpy(), work["state_out"]), flags


@pytest.mark.gpu
@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("scale", SCALES)
def test_input_scales_move_the_arm(scale, engine, monkeypatch):
    import torch
    from sparsernns_amd import _lib

    c = _scaled(scale)
    nl = c["dims"]["n_layers"]
    assert WANT_ARMS[f"scale{scale}"] <= set(layer_arms(c["export"], c["x"], c["bits"], c["exp"], c["rtr"]))
    eng = _make_engine(c["export"], ENGINES[engine], monkeypatch)
    assert (eng.out_bits, eng.out_exp) == c["out"]
    x = torch.from_numpy(c["x"]).cuda()
    for flags in _flag_sets():
        y = torch.empty((3, 333, c["dims"]["d_out"]), dtype=torch.int32, device="cuda")
        kernels, _ = _profiled(lambda: eng.enqueue(x, c["bits"], c["exp"], y, 3, 333, flags=flags))
        _same_heads((scale, flags), _check_rows(kernels, engine == "default", nl, (scale, engine, flags)))
        st = eng.lane_status(0).cpu().numpy()
        assert st[2] == _lib.PATH_FUSED
        if int(st[0]) & _lib.ST_REDO:
            assert flags & _lib.FWD_DEFER_REDO, (scale, flags)
            continue
        got = y.cpu().numpy()
        assert np.array_equal(got, c["ref"]), (scale, engine, flags, np.count_nonzero(got != c["ref"]))
        assert [int(st[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in c["rtr"]], flags
        assert [int(st[8 + 8 * i + 1]) for i in range(nl)] == [t["pre_s5_exp"] for t in c["rtr"]], flags


@pytest.mark.gpu
@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", CONTRACT)
def test_contract_families(name, engine, monkeypatch):
    import torch
    from sparsernns_amd import _lib

    c, rows = _contract(name)
    nl = c.dims["n_layers"]
    eng = _make_engine(c.export(), ENGINES[engine], monkeypatch)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    for kind, x, bits, exp, ref, out, rtr in rows:
        assert (eng.out_bits, eng.out_exp) == out
        xd = torch.from_numpy(x).cuda()
        for flags in _flag_sets():
            y = torch.empty((3, 333, c.dims["d_out"]), dtype=torch.int32, device="cuda")
            run = lambda: eng.enqueue(xd, bits, exp, y, 3, 333, flags=flags)
            if flags == _lib.FWD_DEFER_REDO:
                _same_heads((name, kind), _check_rows(_profiled(run)[0], engine == "default", nl, (name, engine, kind)))
            else:
                run()
            st = eng.lane_status(0).cpu().numpy()
            assert st[2] == _lib.PATH_FUSED
            if int(st[0]) & _lib.ST_REDO:
                assert flags & _lib.FWD_DEFER_REDO, (name, kind, flags)
                continue
            got = y.cpu().numpy()
            assert np.array_equal(got, ref), (name, engine, kind, flags, np.count_nonzero(got != ref))
            assert [int(st[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in rtr], (name, kind, flags)
            assert [int(st[8 + 8 * i + 1]) for i in range(nl)] == [t["pre_s5_exp"] for t in rtr], (name, kind, flags)


@pytest.mark.gpu
def test_traced_forward_keeps_bn16_x4():
    """The traced kernels store pre_s5, which the row chain never forms: ROW = false whatever the engine, and the traces are
    the oracle's."""
    from sparsernns_amd.engine import Engine
    from sparsernns_amd.fxparray import FxpArray

    work = _work("H_traced")
    nl = work["dims"]["n_layers"]
    eng = Engine(work["export"])
    out = {}
    kernels, _ = _profiled(lambda: out.update(r=eng.forward(FxpArray(work["x"], work["bits"], work["exp"]), traces=True)))
    bp = _bprojs(kernels)
    assert len(bp) == nl and all(a == ["3", "4", "true", "0", "4", "false"] for a in bp), bp
    y, tr = out["r"]
    assert np.array_equal(y.numpy(), work["ref"])
    for i in range(nl):
        for k, ck in (("pre_s5", "pre_s5"), ("u", "u"), ("Bu_re", "bu_re"), ("Bu_im", "bu_im")):
            assert np.array_equal(tr[i][k].cpu().numpy(), work["rtr"][i][ck]), (i, k)


# ---- no GPU
def test_no_bproj_kernel_uses_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_bproj_p"], capture_output=True, text=True,
                       timeout=1200)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    rows = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(k_bproj_p<[^>]*>)\s.*\bscratch\s+(\d+)", r.stdout, re.M)}
    row = [k for k in rows if k.endswith(", true>")]
    assert len(rows) >= 32 and len(row) >= 8, sorted(rows)   # the 32 kernels from before ROW, and H = 96's ROW forms (4 SM x 2 NC)
    assert all(k.startswith("k_bproj_p<3, 4, false,") for k in row), row
    assert not {k: v for k, v in rows.items() if v}, {k: v for k, v in rows.items() if v}
