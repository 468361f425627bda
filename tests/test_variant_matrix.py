"""Every experiment switch of include/s5fxp.h ("Environment") against the CPU oracle on the workloads where the fused path's
kernel variants differ: ragged tiles, single frames, grouped calls with a carry, H = 192, w4a8, BatchNorm scale / bias, states
beyond 16 bits and traced forwards.  The header promises "Results do not depend on any of them": outputs, output exponents and
the per-layer exponents must be the oracle's bit for bit under every switch, and every switch must be seen to take effect --
in the status words, the queries, or the kernels and grids the forward launched (torch.profiler).

The switches are read once, by s5fxp_model_create (ModelCfg::from_env), so each case sets its variable, creates an engine
and removes the variable again; models, inputs and oracle results are built once per module.
"""
import ctypes as C
import json
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth

TRACE_MAP = dict(pre_s5="pre_s5", u="u", Bu_re="bu_re", Bu_im="bu_im", xs_re="xs_re", xs_im="xs_im", ys="ys",
                 out2="out2", out2_sigmoid="sigmoid", post_GLU="post_glu", residadd="residadd")
CFG1 = dict(dim_scale=0.5, calib_L=1024, state_headroom_bits=1)   # bench.py's configs[1] model
WGS = ("ENC", "DEC", "CGATE", "BPROJ", "RESID", "CGATE32")
PLANE_SKEW = (1 << 20) + 100   # not a multiple of 256: the library rounds it down; large enough to outgrow the generic layout

SWITCHES = {
    "default": {},
    "no_pair": {"S5FXP_NO_PAIR": "1"},
    "pair_global": {"S5FXP_PAIR_GLOBAL": "1"},
    "pairl_blocks16": {"S5FXP_PAIRL_BLOCKS": "16"},
    "no_pk16": {"S5FXP_NO_PK16": "1"},
    "cgate_ft64": {"S5FXP_CGATE_FT64": "1"},
    "gate_bn": {"S5FXP_GATE_BN": "1"},
    "no_compact": {"S5FXP_NO_COMPACT": "1"},
    "no_live_lanes": {"S5FXP_NO_LIVE_LANES": "1"},
    "no_dec_resid": {"S5FXP_NO_DEC_RESID": "1"},
    "no_bn_ext": {"S5FXP_NO_BN_EXT": "1"},
    "wgs1": {f"S5FXP_WGS_{k}": "1" for k in WGS},          # one workgroup walks every tile, the ragged last one included
    "wgs7": {f"S5FXP_WGS_{k}": "7" for k in WGS},          # divides no tile count here: a partial last round
    "plane_skew": {"S5FXP_PLANE_SKEW": str(PLANE_SKEW)},
    "debug_sync": {"S5FXP_DEBUG_SYNC": "1"},
    # two combinations, for the kernels only they reach: the 128-slot (uncompacted) forms of the H = 192 gate kernel's
    # unpacked epilogue and of the K-stream pair kernel's B projection
    "no_pk16+no_compact": {"S5FXP_NO_PK16": "1", "S5FXP_NO_COMPACT": "1"},
    "pair_global+no_compact": {"S5FXP_PAIR_GLOBAL": "1", "S5FXP_NO_COMPACT": "1"},
}
COMBOS = ("no_pk16+no_compact", "pair_global+no_compact")

WORKLOADS = {
    # name: (model config, B, L, input scale)
    "A_ragged": (CFG1, 3, 333, 1.0),                       # 333 = 1 mod 4, ragged against 32- and 64-frame tiles
    "B_frames33x1": (CFG1, 33, 1, 1.0),
    "B_frames1x7": (CFG1, 1, 7, 1.0),
    "C_grouped": (CFG1, 4, 203, None),                     # G = 3, own input scale per group, carry in and out
    "D_dim10": (dict(dim_scale=1.0, calib_L=256, state_headroom_bits=1), 2, 129, 0.5),
    "E_w4a8": (dict(dim_scale=0.5, quantization="w4a8", bn_stats="random", input_scale=300.0), 2, 100, 300.0),
    "F_bnsb": (dict(dim_scale=0.5, bn_scale_bias=True), 2, 150, 1.0),
    "G_overflow": (dict(dim_scale=0.5), 2, 512, 6.0),       # calibrated at scale 1: states leave 16 bits
    "H_traced": (CFG1, 1, 65, 1.0),
    # out2's output exponent 8 (sigmoid input exponent 6): the sigmoid input has 14 bits, more than the direct table's 12, so
    # the gate kernel's S16 arms run without it (DIRECT = false) -- at H = 96 and at H = 192
    "I_widesig05": (dict(dim_scale=0.5, calib_L=256, state_headroom_bits=1, out2_out_exp=8), 3, 333, 1.0),
    "J_widesig10": (dict(dim_scale=1.0, calib_L=256, state_headroom_bits=1, out2_out_exp=8), 2, 129, 0.5),
}
# workloads run under all four forward flag sets (DEFER_REDO, DEFER_REDO | NO_PAIR, 0, EXACT)
FLAG_SETS = ("A_ragged", "D_dim10", "I_widesig05", "J_widesig10")

# Switch x workload pairs the host code proves to be no-ops (s5fxp_fast.hpp forward_fast), left out of the matrix:
_NO_PK16_ARM = "the gate kernel's PK16 arm needs s16 && sigdir && !traces && 16-bit widths (pk16)"
NO_EFFECT = {
    ("gate_bn", "D_dim10"): "gate_bn = pk16 && fold && !big: H = 192",
    ("gate_bn", "H_traced"): "gate_bn needs pk16, and pk16 needs !traces",
    ("gate_bn", "E_w4a8"): _NO_PK16_ARM,
    ("cgate_ft64", "D_dim10"): "H = 192 runs the 64-frame gate tiles whatever the switch",
    ("cgate_ft64", "H_traced"): "the traced forward launches k_cgate_p<.., TRACE> only",
    ("cgate_ft64", "E_w4a8"): _NO_PK16_ARM,
    ("no_pk16", "H_traced"): "pk16 needs !traces",
    ("no_pk16", "E_w4a8"): _NO_PK16_ARM,
    ("no_compact", "H_traced"): "compact needs !traces",
    ("no_compact", "C_grouped"): "compact needs !state_in && !state_out",
    ("no_live_lanes", "H_traced"): "live lanes need a compacted layer: !traces",
    ("no_live_lanes", "C_grouped"): "live lanes need a compacted layer: !state_in && !state_out",
    ("no_dec_resid", "H_traced"): "dec_resid needs !traces",
    ("no_pair", "H_traced"): "a traced forward never takes the int16 rungs (select_rung: s16 needs !traced)",
    ("pair_global", "H_traced"): "a traced forward never takes the int16 rungs (select_rung: s16 needs !traced)",
    ("pairl_blocks16", "H_traced"): "a traced forward never takes the int16 rungs (select_rung: s16 needs !traced)",
}
for _w in ("I_widesig05", "J_widesig10"):
    for _s in ("gate_bn", "cgate_ft64", "no_pk16"):
        NO_EFFECT[(_s, _w)] = "pk16 needs direct = s16 && sigdir_bits > 0: no direct table for a 14-bit sigmoid input"
# the combination rows run on the flag-set workloads only (their single switches run everywhere)
CASES = [pytest.param(s, w, id=f"{s}-{w}") for s in SWITCHES for w in WORKLOADS
         if (s, w) not in NO_EFFECT and (s not in COMBOS or w in FLAG_SETS)]


def _input(qc, dims, B, L, seed, scale):
    x = synth.make_input(B, L, dims["d_in"], seed=seed, scale=scale)
    return O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)


def _pre_s5_word(export, i):
    """The status word that holds the exponent of the layer's BatchNorm output (mfma_bn.hpp status_exps[1..3])."""
    n = export["params"]["encoder"][f"layers_{i}"]["norm"]
    return 3 if "bias" in n else 2 if "scale" in n else 1


_MODELS, _WORK = {}, {}


def _model(cfg):
    from sparsernns_amd.fxpmodel import build_regression_model
    key = json.dumps(cfg, sort_keys=True)
    if key not in _MODELS:
        cfg = dict(cfg)
        out2_exp = cfg.pop("out2_out_exp", None)
        md, qc, dims = synth.make_model(**cfg)
        if out2_exp is not None:
            qc["blocks"]["out2"]["out_exp"] = out2_exp
        model = build_regression_model(md, qc, dims["n_layers"])
        export = model.export()
        _MODELS[key] = (qc, dims, export, cref.CModel(export))
    return _MODELS[key]


def _work(name):
    """Model, inputs and oracle results of a workload (built once; they do not depend on the switch)."""
    if name in _WORK:
        return _WORK[name]
    cfg, B, L, scale = WORKLOADS[name]
    qc, dims, export, cm = _model(cfg)
    P = dims["P"]
    live = [int(((np.asarray(export["params"]["encoder"][f"layers_{i}"]["mixer"]["B_real"]) != 0).any(axis=1) |
                 (np.asarray(export["params"]["encoder"][f"layers_{i}"]["mixer"]["B_imag"]) != 0).any(axis=1)).sum())
            for i in range(dims["n_layers"])]
    # s5fxp_fast.hpp pack_fast: a layer is compacted onto the fewest groups of 32 slots that hold its live states when that
    # is at most P / 2; stream_live_slots: the int16 rungs then keep whole live state pairs only
    pc = [max(32, (n + 31) // 32 * 32) for n in live]
    slots_c = [c if c <= P // 2 else P for c in pc]
    stream_c = [min(w, max(2, 2 * ((n + 1) // 2))) if w < P else w for n, w in zip(live, slots_c)]
    stream_c = [s if s < w else w for s, w in zip(stream_c, slots_c)]
    w = dict(qc=qc, dims=dims, export=export, B=B, L=L, slots_c=slots_c, stream_c=stream_c)
    if name == "C_grouped":
        G, scales = 3, (1.0, 0.25, 2.0)
        nl, P = dims["n_layers"], dims["P"]
        parts = [_input(qc, dims, B, L, seed=170 + g, scale=scales[g]) for g in range(G)]
        state = np.zeros((G, nl, 2, B, P), dtype=np.int32)
        for g in range(G):   # the carry: what a first chunk of 37 frames leaves behind
            first = _input(qc, dims, B, 37, seed=190 + g, scale=scales[g])
            cm.forward(first.data, first.bits, first.exp, state=state[g])
        w["state_in"] = state.copy()
        refs, exps = [], []
        for g in range(G):
            r, rb, re_, rtr = cm.forward(parts[g].data, parts[g].bits, parts[g].exp, trace=True, state=state[g])
            refs.append(r)
            exps.append([t["residadd_exp"] for t in rtr])
        assert len({tuple(e) for e in exps}) > 1   # the groups really choose different exponents
        w.update(G=G, x=np.concatenate([p.data for p in parts]), bits=parts[0].bits, exp=parts[0].exp, ref=np.concatenate(refs),
                 out=(rb, re_), res_exps=exps, state_out=state)
    else:
        fx = _input(qc, dims, B, L, seed=11 + L, scale=scale)
        ref, rb, re_, rtr = cm.forward(fx.data, fx.bits, fx.exp, trace=True)
        w.update(G=1, x=fx.data, bits=fx.bits, exp=fx.exp, ref=ref, out=(rb, re_), rtr=rtr)
        tops = [max(int(np.abs(t["xs_re"]).max()), int(np.abs(t["xs_im"]).max())) for t in rtr]
        if name == "G_overflow":
            assert max(tops) > 32767, "the workload must take states beyond 16 bits to mean anything"
        w["tops"] = tops
    _WORK[name] = w
    return w


def _engine(work, switch, monkeypatch):
    from sparsernns_amd.engine import Engine
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    try:
        return Engine(work["export"])
    finally:
        for k in SWITCHES[switch]:
            monkeypatch.delenv(k)


def _profiled(fn):
    """Runs fn() under torch.profiler; returns [(kernel name, grid)] of the kernels it launched, in order, and the number of
    hipStreamSynchronize calls it made."""
    import os
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
    syncs = sum(1 for e in ev if e.get("name") == "hipStreamSynchronize")
    return [(e["name"], tuple(e["args"]["grid"])) for e in ks], syncs


def _targs(name):
    """'void s5::k_cgate_p<1, 3, false, ...>(...)' -> ('k_cgate_p', ['1', '3', 'false', ...])"""
    m = re.search(r"s5::(\w+)(?:<([^>]*)>)?\(", name)
    return m.group(1), [a.strip() for a in m.group(2).split(",")] if m.group(2) else []


def _launched(kernels, base):
    return [(_targs(n)[1], g) for n, g in kernels if _targs(n)[0] == base]


def _check_launches(switch, wname, work, profiled):
    """The kernels of one forward show the switch took effect (names, template arguments, grids)."""
    kernels, syncs = profiled
    G = work["G"]
    nl = work["dims"]["n_layers"]
    if "debug_sync" in switch:   # forward_fast synchronises after the encoder, each stage of a layer and the decoder
        assert syncs >= 2 + 3 * nl, syncs
    else:
        assert syncs == 0, syncs
    # a grouped call runs as ONE set of launches (gridDim.y = G) when nothing couples its groups on the host; without the
    # BatchNorm-extremes method s5fxp_model_forward runs it group by group
    per_group_loop = G > 1 and switch == "no_bn_ext"
    assert all(g[1] == (1 if per_group_loop else G) for _, g in kernels), kernels
    big = work["dims"]["H"] == 192
    traced = wname == "H_traced"
    gates = [a for a, _ in _launched(kernels, "k_cgate_p") if a[2] == "false" and a[6] == "false"]   # !TRACE, !WIDE
    # the tile kernels whose workgroups per launch the S5FXP_WGS_* caps set (the exact gate kernel's is fixed)
    capped = [(n, g) for n, g in kernels if _targs(n)[0] in ("k_enc_p", "k_dec_p", "k_bproj_p", "k_cgate_p", "k_resid_minmax16")
              and not (_targs(n)[0] == "k_cgate_p" and _targs(n)[1][6] == "true")]
    if switch == "wgs1":
        if G == 1:   # every tile kernel of the fused path walks all its tiles with one workgroup
            assert capped and all(g[0] == 1 for _, g in capped), capped
        else:        # per_group floors the caps at 64 / 128 workgroups per group, but not the 32-frame gate kernel's
            for a, g in _launched(kernels, "k_cgate_p"):
                if a[5] == "32":
                    assert g[0] == 1, (a, g)
    if switch == "wgs7" and G == 1:
        assert capped and all(g[0] <= 7 for _, g in capped), capped
    if wname not in FLAG_SETS:
        return
    # the flag-set workloads' DEFER_REDO forward: the pair rung, int16 streams, decoder-carried residual pass, and PK16 gate
    # epilogues where the direct sigmoid table exists (32-frame tiles at H = 96, 64-frame ones at H = 192)
    assert not traced
    direct = not wname.startswith(("I_", "J_"))
    assert gates and all(a[3] == "true" and a[4] == str(direct).lower() for a in gates), gates   # S16, DIRECT
    if switch == "cgate_ft64":
        assert all(a[5] == "64" and a[8] == "true" for a in gates), gates
    elif switch == "gate_bn":
        assert all(a[8] == "true" and a[9] == "true" for a in gates), gates
    elif "no_pk16" in switch or not direct:
        assert all(a[8] == "false" and a[5] == "64" for a in gates), gates
    else:
        assert all(a[8] == "true" and a[9] == "false" and a[5] == ("64" if big else "32") for a in gates), gates
    if "no_compact" in switch:
        assert all(a[0] == str(work["dims"]["P"] // 32) for a in gates), gates
    nt = "6" if big else "3"
    decs = [a for a, _ in _launched(kernels, "k_dec_p")]
    resids = _launched(kernels, "k_resid_minmax16") + _launched(kernels, "k_resid16")
    if switch == "no_dec_resid":
        assert decs == [[nt, "false"]] and len(resids) == nl, (decs, len(resids))
    elif switch == "no_bn_ext":
        assert _launched(kernels, "k_bn_reduce16"), kernels
    else:
        assert decs == [[nt, "true"]] and len(resids) == nl - 1, (decs, len(resids))
        assert not _launched(kernels, "k_bn_reduce16")
    scans = {_targs(n)[0] + ("<%s>" % _targs(n)[1][0] if _targs(n)[1] else "") for n, _ in kernels if "k_scan" in n}
    want = {"no_pair": {"k_scan_quad_asm16"}, "pair_global": {"k_scan_pair_asm"}, "pair_global+no_compact": {"k_scan_pair_asm"},
            "pairl_blocks16": {"k_scan_pairl_asm<16>"}}.get(switch, {"k_scan_pairl_asm<32>"})
    assert scans == want, scans
    if switch == "pair_global+no_compact":   # the K-stream B projection over all P state slots
        sm = [a for a, _ in _launched(kernels, "k_bproj_p")]
        assert sm and all(a[3] == "2" and a[4] == ("8" if big else "4") for a in sm), sm


@pytest.mark.parametrize("switch,wname", CASES)
def test_switch_matches_oracle(switch, wname, monkeypatch):
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import FxpArray

    work = _work(wname)
    dims, B, L = work["dims"], work["B"], work["L"]
    nl, P = dims["n_layers"], dims["P"]
    eng = _engine(work, switch, monkeypatch)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1
    assert (eng.out_bits, eng.out_exp) == work["out"]
    rk = [_lib.lib.s5fxp_model_recurrence_kernel(eng._h, i) for i in range(nl)]
    pre_words = [_pre_s5_word(work["export"], i) for i in range(nl)]
    st_words = lambda k: [int(v) for v in eng.lane_status(0).cpu().numpy()[8 + k:8 + 8 * nl:8]]

    def check_exponents():
        exps = eng.layer_exponents()
        rtr = work["rtr"]
        assert [e["residadd"] for e in exps] == [t["residadd_exp"] for t in rtr]
        got = [int(eng.status[8 + 8 * i + pre_words[i]].item()) for i in range(nl)]
        assert got == [t["pre_s5_exp"] for t in rtr]

    x = torch.from_numpy(work["x"]).cuda()
    if switch == "plane_skew":
        # s5fxp_workspace_bytes is the larger of the generic and the fused layout; only the fused one has the skewed planes
        base = _engine(work, "default", monkeypatch)
        monkeypatch.setenv("S5FXP_PLANE_SKEW", str(PLANE_SKEW + 256))
        wider = _engine(work, "default", monkeypatch)
        monkeypatch.delenv("S5FXP_PLANE_SKEW")
        ws = lambda e: _lib.lib.s5fxp_workspace_bytes(e._h, B, L)
        assert ws(eng) > ws(base), (ws(eng), ws(base))
        assert ws(wider) - ws(eng) == 7 * 256, ws(wider) - ws(eng)   # five activation planes, two recurrence streams
    if switch in ("no_pair", "pair_global", "pairl_blocks16", "default") and wname != "H_traced":
        want = {"no_pair": 2, "pair_global": 3}.get(switch, 4)
        if wname in ("A_ragged", "B_frames33x1", "B_frames1x7", "C_grouped") + FLAG_SETS:
            assert rk == [want] * nl, rk

    if wname == "C_grouped":
        G = work["G"]
        y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        s_in = torch.from_numpy(work["state_in"]).cuda()
        s_out = torch.empty_like(s_in)
        launch = lambda fl: eng.enqueue(x, work["bits"], work["exp"], y, B, L, flags=fl, groups=G, state_in=s_in, state_out=s_out)
        _check_launches(switch, wname, work, _profiled(lambda: eng.run_ladder(launch, eng.check_status)))
        assert np.array_equal(y.cpu().numpy(), work["ref"])
        assert np.array_equal(s_out.cpu().numpy(), work["state_out"])
        st = eng.lane_status(0, G).cpu().numpy()
        for g in range(G):
            w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
            assert w[2] == _lib.PATH_FUSED
            assert [int(w[8 + 8 * i + 4]) for i in range(nl)] == work["res_exps"][g], g
            assert [int(w[8 + 8 * i + 6]) for i in range(nl)] == [P] * nl   # a carried forward never compacts
        return

    if wname in FLAG_SETS:
        # the four forward flag sets: LDS-fed pair kernel (or what the switch picks), quad16, self-contained, exact
        for flags in (_lib.FWD_DEFER_REDO, _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR, 0, _lib.FWD_EXACT):
            y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
            run = lambda: eng.enqueue(x, work["bits"], work["exp"], y, B, L, flags=flags)
            if flags == _lib.FWD_DEFER_REDO:
                _check_launches(switch, wname, work, _profiled(run))
            else:
                run()
            st = eng.check_status()
            assert not (st[0] & (_lib.ST_REDO | _lib.ST_WIDE_STATE)), (switch, flags, st[:8])
            assert np.array_equal(y.cpu().numpy(), work["ref"]), (switch, flags)
            check_exponents()
            slots, stream = st_words(6), st_words(7)
            rung = {_lib.FWD_DEFER_REDO: rk[0], _lib.FWD_DEFER_REDO | _lib.FWD_NO_PAIR: 2, 0: 1, _lib.FWD_EXACT: 5}[flags]
            assert st_words(5) == [rung] * nl, (flags, st_words(5))
            assert slots == ([P] * nl if "no_compact" in switch else work["slots_c"]), (flags, slots)
            assert any(s < P for s in work["slots_c"])   # the workload has a compacted layer to lose
            # the rungs whose streams keep only the live slots: LDS-fed pair kernel and quad16 (not the K-stream pair kernel)
            int16_rung = rung == 2 or rung == 4
            if switch == "no_live_lanes" or not int16_rung or "no_compact" in switch:
                assert stream == slots, (flags, stream, slots)
            else:
                assert stream == work["stream_c"], (flags, stream, work["stream_c"])
                assert any(s < w for s, w in zip(stream, slots)), (flags, stream, slots)
        return

    fx = FxpArray(work["x"], work["bits"], work["exp"])
    if wname == "H_traced":
        out = {}
        profiled = _profiled(lambda: out.update(r=eng.forward(fx, traces=True)))
        y, tr = out["r"]
        gates = _launched(profiled[0], "k_cgate_p")
        assert gates and all(a[2] == "true" for a, _ in gates)
        for i in range(nl):
            for k, ck in TRACE_MAP.items():
                got = tr[i][k].cpu().numpy()
                assert np.array_equal(got, work["rtr"][i][ck]), f"layer {i} {k}: {np.count_nonzero(got != work['rtr'][i][ck])} mismatches"
    else:
        out = {}
        profiled = _profiled(lambda: out.update(y=eng.forward(fx)))
        y = out["y"]
    _check_launches(switch, wname, work, profiled)
    assert int(eng.status[2].item()) == _lib.PATH_FUSED
    assert (y.bits, y.exp) == work["out"]
    assert np.array_equal(y.numpy(), work["ref"]), f"{np.count_nonzero(y.numpy() != work['ref'])} mismatches"
    check_exponents()


def _group_loop_forward(hook_counts=None):
    """s5fxp_model_forward with hand-built ForwardOpts: G = 2, G * n_layers trace entries and a carry in and out, which
    s5fxp_model_forward serves with its per-group loop (a traced or hooked grouped call is not one launch set)."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine

    work = _work("A_ragged")
    qc, dims = work["qc"], work["dims"]
    cm = cref.CModel(work["export"])
    G, B, L = 2, 2, 97
    nl, P, H = dims["n_layers"], dims["P"], dims["H"]
    eng = Engine(work["export"])
    parts = [_input(qc, dims, B, L, seed=230 + g, scale=(1.0, 0.5)[g]) for g in range(G)]
    bits, exp = parts[0].bits, parts[0].exp
    state = np.zeros((G, nl, 2, B, P), dtype=np.int32)
    for g in range(G):
        first = _input(qc, dims, B, 29, seed=250 + g, scale=1.0)
        cm.forward(first.data, first.bits, first.exp, state=state[g])
    s_in = torch.from_numpy(state.copy()).cuda()
    refs = [cm.forward(parts[g].data, bits, exp, trace=True, state=state[g]) for g in range(G)]
    x = torch.from_numpy(np.concatenate([p.data for p in parts])).cuda()
    y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
    s_out = torch.empty_like(s_in)
    ws = torch.empty(G * _lib.lib.s5fxp_workspace_bytes(eng._h, B, L), dtype=torch.uint8, device="cuda")
    status = torch.zeros(G * _lib.STATUS_WORDS, dtype=torch.int32, device="cuda")
    bufs = []
    tr = (_lib.LayerTrace * (G * nl))()
    for g in range(G):
        bufs.append([])
        for i in range(nl):
            d = {}
            for k in _lib.TRACE_FIELDS:
                d[k] = torch.full((B, L, P if k in ("Bu_re", "Bu_im", "xs_re", "xs_im") else H), -7, dtype=torch.int32, device="cuda")
                setattr(tr[g * nl + i], k, d[k].data_ptr())
            bufs[g].append(d)
    opts = _lib.ForwardOpts()
    opts.groups, opts.flags = G, 0
    opts.state_in, opts.state_out = s_in.data_ptr(), s_out.data_ptr()
    if hook_counts is not None:
        def _hook(ctx, dev_ptr, n, stream):   # identity at one rank: the maxima are already global
            hook_counts.append(int(n))
            return 0
        opts.allreduce = _lib.ALLREDUCE_FN(_hook)
    rc = _lib.lib.s5fxp_model_forward(eng._h, x.data_ptr(), bits, exp, B, L, y.data_ptr(), ws.data_ptr(), ws.numel(),
                                      status.data_ptr(), C.cast(tr, C.POINTER(_lib.LayerTrace)), C.byref(opts),
                                      torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "s5fxp_model_forward")
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    yy = y.cpu().numpy().reshape(G, B, L, -1)
    for g in range(G):
        ref, rb, re_, rtr = refs[g]
        w = st[g * _lib.STATUS_WORDS:(g + 1) * _lib.STATUS_WORDS]
        assert w[2] == _lib.PATH_FUSED and not (w[0] & (_lib.ST_REDO | _lib.ST_NEGSHIFT | _lib.ST_NEGEXP)), w[:8]
        assert (eng.out_bits, eng.out_exp) == (rb, re_)
        assert np.array_equal(yy[g], ref), g
        assert [int(w[8 + 8 * i + 4]) for i in range(nl)] == [t["residadd_exp"] for t in rtr], g
        for i in range(nl):
            for k, ck in TRACE_MAP.items():
                got = bufs[g][i][k].cpu().numpy()
                assert np.array_equal(got, rtr[i][ck]), f"group {g} layer {i} {k}: {np.count_nonzero(got != rtr[i][ck])} mismatches"
    assert np.array_equal(s_out.cpu().numpy(), state)
    return dims


def test_grouped_call_with_traces_and_carry_runs_per_group():
    _group_loop_forward()


def test_grouped_call_with_a_hook_calls_it_per_group():
    calls = []
    dims = _group_loop_forward(hook_counts=calls)
    # per group and layer (test_exponent_hook_is_called_per_compute_best_op): the 2H per-channel extremes, then the three
    # maxima of the residual add
    assert calls == [2 * dims["H"], 3] * dims["n_layers"] * 2, calls


# (H, P, d_out) of one-layer models off the fused path (d_in = 5): together they take the generic kernels' column budget
# mw_for(M) (s5fxp_api.hip) through every bucket -- 4, 8, 16, 24, 32, 48 for H, up to 64 and 68 for 2P and d_out
GENERIC_DIMS = [(12, 6, 5), (32, 16, 30), (64, 32, 60), (96, 48, 90), (128, 64, 120), (192, 96, 180), (64, 128, 256),
                (32, 136, 270)]


def _mw(M):
    return ((M + 3) // 4 + 3) // 4 * 4


@pytest.mark.parametrize("engine", ["default", "force_generic"])
@pytest.mark.parametrize("H,P,d_out", GENERIC_DIMS)
def test_generic_kernels_at_every_column_budget(H, P, d_out, engine):
    """The generic int32 path dispatches its dense, B projection, C projection and out2 / gate kernels on a compile-time
    column budget, each with a 24-bit-multiply form (weights that fit 24 bits) and an exact one (MODEL_FORCE_GENERIC).
    Every form must give the oracle's bits."""
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine
    from sparsernns_amd.fxparray import FxpArray
    from sparsernns_amd.fxpmodel import build_regression_model

    md, qc, dims = synth.make_model(dims=synth.tiny_dims(H=H, P=P, d_in=5, d_out=d_out, n_layers=1), calib_L=64)
    export = build_regression_model(md, qc, 1).export()
    eng = Engine(export, flags=_lib.MODEL_FORCE_GENERIC if engine == "force_generic" else 0)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 0
    fx = _input(qc, dims, 2, 37, seed=H + P, scale=1.0)
    ref, rb, re_, _ = cref.CModel(export).forward(fx.data, fx.bits, fx.exp)
    out = {}
    kernels, _ = _profiled(lambda: out.update(y=eng.forward(FxpArray(fx.data, fx.bits, fx.exp))))
    y = out["y"]
    assert (y.bits, y.exp) == (rb, re_)
    assert np.array_equal(y.numpy(), ref), f"{np.count_nonzero(y.numpy() != ref)} mismatches"
    x24 = "false" if engine == "force_generic" else "true"
    got = {(_targs(n)[0], tuple(_targs(n)[1])) for n, _ in kernels}
    want = {("k_dense", (str(_mw(H)), x24)), ("k_dense", (str(_mw(d_out)), x24)), ("k_bproj", (str(_mw(2 * P)), x24)),
            ("k_out2gate", (str(_mw(H)), x24)), ("k_cproj", (str(_mw(H)), "false", "1", "int"))}
    if engine == "default":
        want.add(("k_cproj", (str(_mw(H)), "true", "0", "int")))
    assert want <= got, sorted(want - got)
