#!/usr/bin/env python3
"""What s5fxp_stage_err costs against the same figures as torch ops, and what it reports.

  cost         32 x 4096 frames, dim_scale 0.5 and 1.0, the w8a8 recipe.  Both traced forwards run once; the planes stay where
               they are.  Two arms on the same tensors, alternating in one process, device-event ms:
                 call    ONE s5fxp_stage_err over all rows of verify.compare_engines (by="stage"), descriptors prepared
                 torch   the only device-side way without the entry: per row the same sums, counts, maxima and the two
                         exponent histograms as torch ops in float64
               next to them the call with by="time", 8 buckets (8 x the pairs, the same elements), and the algorithmic bytes
               (8 per element: 4 from each side) over the call's time.
               Equal results at the timed size: per kind of pair (int32, int32 with RELU_A, a strided complex half, float32)
               the whole-plane record and a seeded subsample of slabs of rows against verify.stage_errors_host, to the bounds
               of tests/test_stage_err.py.
  attribution  the synthetic w8a8 and w4a8 models at dim_scale 0.5, calibrated on 8 x 512 (seed 31), evaluated on 8 x 512
               (seed 32), the batches of §4u / §4v: per stage SQNR and exact share of the integer model against the plain
               float model and against the fully quantised one (every site, step mode, all weight groups), and mixer.xs of
               layer 0 over 8 time buckets.

Writes the JSON given with --out and prints one summary line.  Exit status 1 if the call takes more than half the torch
chain's median or a record misses its bound.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (32, 4096)
DIMS = (0.5, 1.0)
RECIPE = dict(bn_stats="random", input_scale=300.0)
HBM_ROWS_TBS = 6.3  # rows streaming from HBM
EPS = 2.0 ** -53
EXACT = ("n", "n_nonfinite", "n_equal", "n_ref_nonzero", "max_abs", "max_rel", "hist_abs", "hist_rel")
SUMS = ("sum_abs", "sum_sq", "sum_ref_sq", "sum_rel")


def _stats(v):
    v = [float(x) for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), reps=v)


def _time(arms, reps, warmup):
    import torch

    for _ in range(warmup):
        for run in arms.values():
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, run in arms.items():  # alternating arms
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {f"{k}_ms": _stats(v) for k, v in times.items()}


def torch_row(a, b, a_exp, relu):
    """The figures of one record as torch ops on the device (float64), histograms included."""
    import torch

    def hist(v):
        e = ((v.float().view(torch.int32) >> 23) & 0xff) - 87
        return torch.bincount(e.clamp_(0, 63).flatten(), minlength=64)

    va = a.double() * 2.0 ** -a_exp if a.dtype == torch.int32 else a.double()
    vb = b.double()
    fin = torch.isfinite(va) & torch.isfinite(vb)
    if relu:
        va = va.clamp_min(0.0)
    n_nonfin = fin.numel() - fin.sum()
    va, vb = va[fin], vb[fin]
    e = (va - vb).abs()
    nz = vb != 0
    rel = e[nz] / vb[nz].abs()
    return (n_nonfin, (e == 0).sum(), nz.sum(), e.sum(), (e * e).sum(), e.max(), (vb * vb).sum(), rel.sum(), rel.max(), hist(e), hist(rel))


def same(got, want, what, problems):
    n = want["n"]
    nf = n - want["n_nonfinite"]
    var = lambda r: r["sum_sq"] / nf - (r["sum_abs"] / nf) ** 2 if nf else 0.0
    for k in EXACT:
        if not np.array_equal(np.asarray(got[k]), np.asarray(want[k])):
            problems.append(f"{what}: {k} {got[k]} != {want[k]}")
    for k in SUMS:
        if abs(got[k] - want[k]) > 2 * n * EPS * abs(want[k]):
            problems.append(f"{what}: {k} {got[k]!r} vs {want[k]!r} beyond 2 n 2^-53")
    if abs(var(got) - var(want)) > 4 * EPS * want["sum_sq"]:
        problems.append(f"{what}: variance {var(got)!r} vs {var(want)!r}")


def equal_check(rows, frows, problems) -> dict:
    """One plane pair per kind at the timed size: the whole plane and 16 seeded slabs of 64 frames against the host statement."""
    from sparsernns_amd import verify

    pick = {"int32": rows[1], "int32 relu": next(r for r in rows if r[4]), "complex half": next(r for r in rows if "xs (imag)" in r[0]),
            "float32": next(r for r in frows if r[0] == "l0.y")}
    rng = np.random.default_rng(28)
    pairs, names = [], []
    for kind, (name, a, b, a_exp, relu) in pick.items():
        pairs.append(verify.pair(a, b, a_exp, relu))
        names.append(f"{kind}: {name}, whole plane")
        for _ in range(16):
            s, t0 = int(rng.integers(0, a.shape[0])), int(rng.integers(0, a.shape[1] - 64))
            pairs.append(verify.pair(a[s, t0:t0 + 64], b[s, t0:t0 + 64], a_exp, relu))
            names.append(f"{kind}: {name}, sequence {s} frames {t0}..{t0 + 63}")
    got, want = verify.stage_errors(pairs), verify.stage_errors_host(pairs)
    for n, g, w in zip(names, got, want):
        same(g, w, n, problems)
    return dict(pairs=len(pairs), kinds={k: v[0] for k, v in pick.items()})


def cost(args, problems) -> dict:
    import torch
    from sparsernns_amd import floatmodel, synth, verify
    from sparsernns_amd.fxpmodel import build_regression_model

    out = {}
    B, L = SHAPE
    for dim in DIMS:
        md, qc, dims = synth.make_model(dim, quantization="w8a8", **RECIPE)
        nl = dims["n_layers"]
        eng, feng = build_regression_model(md, qc, nl).engine(), floatmodel.FloatEngine(md, nl)
        assert feng.on_device
        x = torch.from_numpy(synth.make_input(B, L, dims["d_in"], seed=3, scale=RECIPE["input_scale"])).to(feng.device)
        rows = verify.engine_rows(eng, feng, x, qc)
        stage = verify.StageCall(verify._split(rows, "stage", 8)[0])
        buckets = verify.StageCall(verify._split(rows, "time", 8)[0])
        elements = sum(p.n for p in stage.pairs)
        r = dict(dim_scale=dim, B=B, L=L, rows=len(rows), pairs_by_time=len(buckets.pairs), elements=elements, bytes=8 * elements)
        r.update(_time(dict(call=stage.enqueue, torch=lambda: [torch_row(a, b, e, relu) for _, a, b, e, relu in rows],
                            call_by_time=buckets.enqueue), args.reps, args.warmup))
        r["call_over_torch"] = r["call_ms"]["median"] / r["torch_ms"]["median"]
        r["by_time_over_stage"] = r["call_by_time_ms"]["median"] / r["call_ms"]["median"]
        r["algorithmic_tb_per_s"] = r["bytes"] / (r["call_ms"]["median"] * 1e-3) / 1e12
        r["hbm_rows_tb_per_s"] = HBM_ROWS_TBS
        if r["call_over_torch"] > 0.5:
            problems.append(f"dim {dim}: the call takes {r['call_over_torch']:.3f} of the torch chain (bar 0.5)")
        # the torch chain computes the call's figures: counts and maxima of the first rows, exactly
        recs = stage.records()
        for (name, a, b, e, relu), rec in list(zip(rows, recs))[:4]:
            t = torch_row(a, b, e, relu)
            if (int(t[0]), int(t[1]), int(t[2]), float(t[5])) != (rec["n_nonfinite"], rec["n_equal"], rec["n_ref_nonzero"], rec["max_abs"]):
                problems.append(f"dim {dim}: {name}: the torch chain and the call disagree")
        sums = {k: sum(rr[k] for rr in buckets.records()) for k in ("n", "n_equal")}
        if sums["n"] != elements or sums["n_equal"] != sum(rr["n_equal"] for rr in recs):
            problems.append(f"dim {dim}: the time buckets do not add up to the stages")
        frows = verify.float_rows(feng, x, floatmodel.fq_spec(qc, nl))
        r["equal_check"] = equal_check(rows, frows, problems)
        out[f"dim{dim}_B{B}_L{L}"] = r
        print(f"[bench_stage_err] dim {dim} {B} x {L}: {len(rows)} rows, {elements / 1e6:.1f} M elements: call "
              f"{r['call_ms']['median']:.3f} ms ({r['call_ms']['min']:.3f}-{r['call_ms']['max']:.3f}), torch "
              f"{r['torch_ms']['median']:.3f} ms ({r['torch_ms']['min']:.3f}-{r['torch_ms']['max']:.3f}): x{r['call_over_torch']:.4f}; "
              f"{r['algorithmic_tb_per_s']:.2f} TB/s algorithmic; by time, 8 buckets: {r['call_by_time_ms']['median']:.3f} ms "
              f"(x{r['by_time_over_stage']:.3f})", flush=True)
        del x, rows, frows, stage, buckets
        torch.cuda.empty_cache()
    return out


def attribution() -> dict:
    from sparsernns_amd import floatmodel, synth, verify
    from sparsernns_amd.fxpmodel import build_regression_model

    out = {}
    keep = ("n", "sqnr_db", "equal_share", "abs_error_mean", "abs_error_max", "abs_error_med_lo", "abs_error_med_hi")
    for q in ("w8a8", "w4a8"):
        md, _, dims = synth.make_model(0.5, quantization=q, **RECIPE)
        nl, scale = dims["n_layers"], RECIPE["input_scale"]
        feng = floatmodel.FloatEngine(md, nl)
        xc = synth.make_input(8, 512, dims["d_in"], seed=31, scale=scale)
        xe = synth.make_input(8, 512, dims["d_in"], seed=32, scale=scale)
        _, qc = floatmodel.calibrate(md, [xc], nl, quantization=q, engine=feng)
        eng = build_regression_model(md, qc, nl).engine()
        full = floatmodel.FloatEngine(floatmodel.quantised_modeldict(md, qc, nl), nl)
        spec = floatmodel.fq_spec(qc, nl, recurrence="step")
        plain = verify.compare_engines(eng, feng, xe, qc)
        quant = verify.compare_engines(eng, full, xe, qc, fq=spec)
        name = "encoder.layers_0.mixer.xs"
        by_time = {side: [r for r in verify.compare_engines(eng, fe, xe, qc, fq=fq, by="time") if r["name"].startswith(name)]
                   for side, fe, fq in (("plain", feng, None), ("quantised", full, spec))}
        slim = lambda rows, extra=(): [{k: r[k] for k in ("name",) + tuple(extra) + keep} for r in rows]
        out[q] = dict(dim_scale=0.5, calibration="8 x 512, seed 31", evaluation="8 x 512, seed 32", input_scale=scale,
                      against_plain_float=slim(plain), against_fully_quantised_float=slim(quant),
                      layer0_xs_by_time={k: slim(v, ("t0", "t1")) for k, v in by_time.items()})
        for p, u in zip(plain, quant):
            print(f"[bench_stage_err] {q} {p['name']:<40} plain {p['sqnr_db']:7.2f} dB {100 * p['equal_share']:6.2f} %   "
                  f"quantised {u['sqnr_db']:7.2f} dB {100 * u['equal_share']:6.2f} %", flush=True)
        for side, rows in by_time.items():
            for r in rows:
                print(f"[bench_stage_err] {q} {side} {r['name']} t {r['t0']}..{r['t1'] - 1}: {r['sqnr_db']:.2f} dB, "
                      f"{100 * r['equal_share']:.2f} %, mean |e| {r['abs_error_mean']:.3e}", flush=True)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-attribution", action="store_true")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("[bench_stage_err] no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    torch.cuda.set_device(0)
    problems: list = []

    def plain(v):
        if isinstance(v, float) and not np.isfinite(v):
            return str(v)
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, list):
            return [plain(x) for x in v]
        return v

    res = dict(tool="tools/bench_stage_err.py", reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               unit="ms of device time", cost=cost(args, problems),
               attribution=None if args.skip_attribution else attribution(), problems=problems)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(plain(res), f, indent=1)
    print(json.dumps({"tool": res["tool"], "problems": problems,
                      "cost": {k: dict(call_ms=w["call_ms"]["median"], torch_ms=w["torch_ms"]["median"], ratio=w["call_over_torch"],
                                       tb_per_s=w["algorithmic_tb_per_s"], by_time_ms=w["call_by_time_ms"]["median"])
                               for k, w in res["cost"].items()}}))
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main())
