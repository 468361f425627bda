"""The gate kernel that rebuilds the SSM input u = BatchNorm(layer input) in its tile staging (k_cgate_p<.., UREC>, the default
of the 32-frame form) against the C oracle, beside the kernels that move u through memory (S5FXP_GATE_BN=0):

  * the variant matrix's H = 96 workloads (ragged 3 x 333, 33 x 1, 1 x 7, the grouped call with a carry, BatchNorm scale / bias,
    the overflowing input) under all four forward flag sets, and one model of every contract family at dim_scale 0.5
    (tests/contract_models.py): outputs, output exponents and per-layer exponents are the oracle's, and the kernels the
    DEFER_REDO forward launched (torch.profiler) are the form the plan promises -- UREC = true on every 32-frame gate launch of
    a model without BatchNorm scale / bias, false under the switch, for scale / bias models and on every other gate form;
  * with flags 0 the in-forward exact re-run reads u from memory, so the B projection must have stored it: the overflowing input
    gives the oracle's bits, also under S5FXP_GATE_BN=1;
  * every arm of bn16_row8 equals bn16_x4 on all 65 536 inputs and every shift pattern (tools/probe_bn16_row8.hip).
"""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import contract_models as CM
from test_variant_matrix import WORKLOADS, _launched, _pre_s5_word, _profiled, _work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = {"default": {}, "no_gate_urec": {"S5FXP_GATE_BN": "0"}}
H96 = ("A_ragged", "B_frames33x1", "B_frames1x7", "C_grouped", "F_bnsb", "G_overflow")
SAME_MODEL_AS_A = ("A_ragged", "B_frames33x1", "B_frames1x7", "C_grouped")   # bench.py's configs[1] model: PK16, 32-frame tiles


def _flag_sets():
    from sparsernns_amd import _lib
    return (_lib.FWD_DEFER_REDO, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, 0, _lib.FWD_EXACT)


def _make_engine(export, env, monkeypatch):
    from sparsernns_amd.engine import Engine
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return Engine(export)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _gates(kernels):
    """Template arguments of the untraced, non-WIDE k_cgate_p launches: a[5] FTP, a[8] PK16, a[9] GBN, a[10] UREC."""
    return [a for a, _ in _launched(kernels, "k_cgate_p") if a[2] == "false" and a[6] == "false"]


def _check_forms(kernels, urec_ok, must_be_ft32, what):
    """Every gate launch is in the form the plan promises (s5fxp_fast.hpp plan_layer): rebuilt u on the 32-frame form when the
    engine allows it, the BatchNorm has no scale / bias (both in urec_ok) and the B projection derives and publishes the
    exponents -- which it does exactly when the forward runs no k_bn_reduce16 (models whose BatchNorm operands the per-channel
    extremes method does not take, s5fxp_fast.hpp fast_bn_ext, keep reading u).  Returns the gate launches."""
    gates = _gates(kernels)
    urec_ok = urec_ok and not _launched(kernels, "k_bn_reduce16")
    assert gates, what
    for a in gates:
        assert len(a) == 11, (what, a)
        ft32 = a[5] == "32"
        assert a[10] == ("true" if ft32 and urec_ok else "false"), (what, a)
        if ft32:
            assert a[8] == "true" and a[9] == "false", (what, a)
    if must_be_ft32:
        assert urec_ok == (what[1] == "default") and all(a[5] == "32" for a in gates), (what, gates)
    return gates


def _bproj_stores_u(export):
    """True if the model has a BatchNorm scale or bias stage (such models keep reading u)."""
    n = export["params"]["encoder"]["layers_0"]["norm"]
    return "scale" in n or "bias" in n


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("wname", H96)
def test_matrix_workloads_under_every_flag_set(wname, engine, monkeypatch):
    import torch
    from sparsernns_amd import _lib

    assert WORKLOADS[wname][0].get("dim_scale") == 0.5
    work = _work(wname)
    dims, B, L, G = work["dims"], work["B"], work["L"], work["G"]
    nl = dims["n_layers"]
    eng = _make_engine(work["export"], ENGINES[engine], monkeypatch)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    assert (eng.out_bits, eng.out_exp) == work["out"]
    urec_ok = engine == "default" and not _bproj_stores_u(work["export"])
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
        if flags == _lib.FWD_DEFER_REDO:
            kernels, _ = _profiled(run)
            _check_forms(kernels, urec_ok, wname in SAME_MODEL_AS_A, (wname, engine))
        else:
            run()
        st = eng.lane_status(0, G).cpu().numpy()
        redo = any(int(st[g * _lib.STATUS_WORDS]) & _lib.ST_REDO for g in range(G))
        if wname == "G_overflow":
            # the int16 rungs cannot hold this input's states: they say so, the other two flag sets compute it
            assert redo == bool(flags & _lib.FWD_DEFER_REDO), (flags, st[:8])
        # only the int16 rungs may find a state out of their range (the caller then repeats: the ladder below)
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
    # the caller's ladder, as the variant matrix runs it: starts on the top rung and must end on the oracle's bits
    if grouped:
        y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        s_out = torch.empty_like(s_in)
        eng.run_ladder(lambda fl: eng.enqueue(x, work["bits"], work["exp"], y, B, L, flags=fl, groups=G, state_in=s_in, state_out=s_out),
                       eng.check_status)
        assert np.array_equal(y.cpu().numpy(), work["ref"])
        assert np.array_equal(s_out.cpu().numpy(), work["state_out"])
    else:
        from sparsernns_amd.fxparray import FxpArray
        yl = eng.forward(FxpArray(work["x"], work["bits"], work["exp"]))
        assert (yl.bits, yl.exp) == work["out"]
        assert np.array_equal(yl.numpy(), work["ref"])
        rtr = work["rtr"]
        assert [e["residadd"] for e in eng.layer_exponents()] == [t["residadd_exp"] for t in rtr]
        assert [int(eng.status[8 + 8 * i + pre_words[i]].item()) for i in range(nl)] == [t["pre_s5_exp"] for t in rtr]


# one model of every contract family at H = 96 (the F4 live counts: none, one, the compaction boundary and all)
CONTRACT = ["F1_full_ds0.5", "F2_rails_ds0.5", "F3_D16_ds0.5", "F3_Bu24_ds0.5", "F3_out32_ds0.5", "F3_dims257x1_ds0.5",
            "F4_live0_ds0.5", "F4_live1_ds0.5", "F4_live32_ds0.5", "F4_live33_ds0.5", "F4_live64_ds0.5",
            "F5_y+4_ds0.5", "F5_y+3_l-y14_ds0.5", "F5_y+3_l-y15_ds0.5"]
REACHES_PK16 = ("F5_y+4_ds0.5", "F5_y+3_l-y14_ds0.5")   # asserted by tests/test_fast_contract.py as well


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", CONTRACT)
def test_contract_families(name, engine, monkeypatch):
    import torch
    from sparsernns_amd import _lib

    c = CM.case(name)
    nl = c.dims["n_layers"]
    cm = c.c_oracle()
    eng = _make_engine(c.export(), ENGINES[engine], monkeypatch)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    B, L = 3, 333
    for kind in ("ndns", "flip"):
        x, bits, exp = CM.input_for(c, kind, B, L, seed=L)
        ref, rb, re_, rtr = cm.forward(x, bits, exp, trace=True)
        assert (eng.out_bits, eng.out_exp) == (rb, re_)
        xd = torch.from_numpy(x).cuda()
        for flags in _flag_sets():
            y = torch.empty((B, L, c.dims["d_out"]), dtype=torch.int32, device="cuda")
            run = lambda: eng.enqueue(xd, bits, exp, y, B, L, flags=flags)
            if flags == _lib.FWD_DEFER_REDO:
                gates = _check_forms(_profiled(run)[0], engine == "default", False, (name, engine))
                pk16 = [a for a in gates if a[8] == "true"]
                if name in REACHES_PK16:   # ... in the 32-frame form
                    assert len(pk16) == nl and all(a[5] == "32" for a in pk16), gates
                if name == "F5_y+3_l-y15_ds0.5":   # one past the PK16 limit: the old kernels, whatever the engine
                    assert not pk16 and all(a[10] == "false" for a in gates), gates
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


@pytest.mark.parametrize("env", [{}, {"S5FXP_GATE_BN": "0"}, {"S5FXP_GATE_BN": "1"}], ids=["default", "no_gate_urec", "gate_bn"])
def test_in_forward_rerun_finds_u_in_memory(env, monkeypatch):
    """flags 0 on the overflowing input: the gated exact kernels re-run the layers inside the forward and read u from the
    workspace, so no form of the gate kernel may have told the B projection to leave it out."""
    import torch
    from sparsernns_amd import _lib

    work = _work("G_overflow")
    dims, B, L = work["dims"], work["B"], work["L"]
    nl = dims["n_layers"]
    eng = _make_engine(work["export"], env, monkeypatch)
    x = torch.from_numpy(work["x"]).cuda()
    y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
    kernels, _ = _profiled(lambda: eng.enqueue(x, work["bits"], work["exp"], y, B, L, flags=0))
    wide = [a for a, _ in _launched(kernels, "k_cgate_p") if a[6] == "true"]
    assert len(wide) == nl, kernels   # the re-run kernels are part of the forward
    st = eng.lane_status(0).cpu().numpy()
    assert not (int(st[0]) & _lib.ST_REDO), st[:8]
    got = y.cpu().numpy()
    assert np.array_equal(got, work["ref"]), np.count_nonzero(got != work["ref"])
    assert [int(st[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in work["rtr"]]
    # and the optimistic forward of the same engine takes the form its switch selects
    kernels, _ = _profiled(lambda: eng.enqueue(x, work["bits"], work["exp"], y, B, L, flags=_lib.FWD_DEFER_REDO))
    gates = _gates(kernels)
    if env.get("S5FXP_GATE_BN") == "1":
        assert gates and all(a[9] == "true" and a[10] == "false" for a in gates), gates
    else:
        _check_forms(kernels, not env, False, (env, "default"))


def test_row_chain_arms_equal_bn16_x4(tmp_path):
    """tools/probe_bn16_row8.hip: zero differences, every arm reached, every boundary pattern rejected."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "probe_bn16_row8")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "probe_bn16_row8.hip"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("ROW_")]
    assert [l[0] for l in lines] == ["ROW_GENERIC", "ROW_PACKED", "ROW_SHIFTED"], r.stdout
    for l in lines:
        assert int(l[2]) > 0 and int(l[4]) > 0 and int(l[6]) == 0, l
    assert "rejections wrong: 0" in r.stdout
