"""Randomised parity stress (GPU): fused forward vs the scalar C oracle over random shapes, scales and models, any sequence
length (ragged last recurrence blocks and tiles), an experiment switch of include/s5fxp.h per case (the engine is created with
it set), and now and then a grouped call of several batches with a carried state.
Not part of the test suite (minutes); run by hand:  python tools/stress_parity.py [n_cases] [seed]"""
import os, sys, time
import numpy as np
sys.path.insert(0, ".")
import torch
import __graft_entry__ as g
g.build()
from oracle import cref, fxp_oracle as O
from sparsernns_amd import synth, _lib
from sparsernns_amd.engine import InflightRunner
from sparsernns_amd.fxparray import FxpArray
from sparsernns_amd.fxpmodel import build_regression_model

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
# third argument: comma-separated input scales to draw from (large ones push the states out of the 16-bit fast range
# and exercise the exact kernels)
SCALES = [float(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0.3, 1.0, 1.0, 2.5, 6.0]
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
sys.path.insert(0, "tests")
from test_variant_matrix import SWITCHES  # noqa: E402  (the switch settings of the variant-matrix tests)
bad = 0
rungs = {}
t0 = time.time()
for case in range(n_cases):
    dim = float(rng.choice([0.5, 0.5, 0.5, 1.0]))
    cfg = dict(dim_scale=dim, seed=int(rng.integers(1, 10_000)), sparsity=float(rng.choice([0.0, 0.0, 0.9])),
               calib_L=int(rng.choice([64, 128, 256])), state_headroom_bits=int(rng.choice([0, 1])))
    if rng.random() < 0.25:
        cfg.update(bn_scale_bias=True)
    md, qc, dims = synth.make_model(**cfg)
    model = build_regression_model(md, qc, dims["n_layers"])
    switch = str(rng.choice(sorted(SWITCHES)))
    os.environ.update(SWITCHES[switch])
    try:
        eng = model.engine()    # ModelCfg::from_env reads the switches here, once
    finally:
        for k in SWITCHES[switch]:
            del os.environ[k]
    cm = cref.CModel(model.export())
    B = int(rng.integers(1, 5))
    L = int(rng.integers(1, 640 if dim == 0.5 else 240))
    scale = float(rng.choice(SCALES))
    if rng.random() < 0.3:
        # a grouped call: G batches in one set of launches, each with its own carry in and out
        G = int(rng.integers(2, 5))
        nl, P = dims["n_layers"], dims["P"]
        fxs = [O.from_fp(synth.make_input(B, L, dims["d_in"], seed=int(rng.integers(1, 10_000)), scale=scale * float(rng.choice([0.5, 1.0, 2.0]))),
                         qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR) for _ in range(G)]
        state = rng.integers(-300, 300, size=(G, nl, 2, B, P)).astype(np.int32)
        s_in = torch.from_numpy(state.copy()).cuda()
        s_out = torch.empty_like(s_in)
        xd = torch.from_numpy(np.concatenate([f.data for f in fxs])).cuda()
        y = torch.empty((G * B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        try:
            eng.run_ladder(lambda fl: eng.enqueue(xd, fxs[0].bits, fxs[0].exp, y, B, L, flags=fl, groups=G, state_in=s_in,
                                                  state_out=s_out), eng.check_status)
            refs = [cm.forward(fxs[g].data, fxs[g].bits, fxs[g].exp, state=state[g])[0] for g in range(G)]
            same = np.array_equal(y.cpu().numpy(), np.concatenate(refs)) and np.array_equal(s_out.cpu().numpy(), state)
        except Exception as e:   # a grouped call has no legitimate error outcome here: count it
            bad += 1
            print(f"FAILED case {case}: grouped G={G} switch={switch} B={B} L={L} scale={scale} cfg={cfg} raised {e!r}")
            continue
        bad += 0 if same else 1
        print(f"{'MISMATCH ' if not same else ''}case {case}: grouped G={G} carry switch={switch} dim={dim} B={B} L={L} "
              f"scale={scale} cfg={cfg} {'ok' if same else ''}   [{time.time() - t0:.0f}s]", flush=True)
        continue
    runner = InflightRunner(eng, depth=int(rng.integers(1, 4)))
    jobs = []
    for j in range(3):
        x = synth.make_input(B, L, dims["d_in"], seed=int(rng.integers(1, 10_000)), scale=scale)
        fx = O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
        xd = torch.from_numpy(fx.data).cuda()
        y = torch.empty((B, L, dims["d_out"]), dtype=torch.int32, device="cuda")
        try:
            runner.submit(xd, fx.bits, fx.exp, y, B, L)
        except Exception as e:  # ValueError / OverflowError are legitimate outcomes: the oracle must agree
            jobs.append((fx, None, e)); continue
        jobs.append((fx, y, None))
    try:
        runner.drain()
        err = None
    except Exception as e:
        err = e
    for j, (fx, y, e) in enumerate(jobs):
        if y is None or err is not None:
            print(f"case {case}.{j}: dim={dim} B={B} L={L} scale={scale} cfg={cfg} raised {e or err!r} (not compared)")
            continue
        ref, _, _, _ = cm.forward(fx.data, fx.bits, fx.exp)
        same = np.array_equal(y.cpu().numpy(), ref)
        if not same:
            bad += 1
            print(f"MISMATCH case {case}.{j}: switch={switch} dim={dim} B={B} L={L} scale={scale} cfg={cfg} "
                  f"diff={np.count_nonzero(y.cpu().numpy() != ref)}")
    st = int(eng.status[0].item())
    rung = ("pair", "quad16", "exact")[eng.level]
    rungs[rung] = rungs.get(rung, 0) + 1
    print(f"case {case}: switch={switch} dim={dim} B={B} L={L} scale={scale} sparsity={cfg['sparsity']} fast={bool(_lib.lib.s5fxp_model_is_fast(eng._h))} "
          f"recurrence rung after the case={rung} status=0x{st:x} ok   [{time.time() - t0:.0f}s]", flush=True)
print("cases that ended on each recurrence rung:", rungs)
print("mismatches:", bad)
sys.exit(1 if bad else 0)
