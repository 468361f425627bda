#!/usr/bin/env python3
"""bench_validate.py: the N-DNS validation step (fxprun.py:63-88) around BASELINE configs[1]'s model (dim_scale 0.5, w8a16), on
B clips of T = 480000 samples (3751 STFT frames, the N-DNS clip), per batch:
  (a) audio.validate_batch of the tree given with --parent-root (the parent commit, built there), loaded next to this one:
      stft_mag -> model -> mask_istft(cleaned_mag) -> stft_mag(clean, 0) -> torch mean / si_snr;
  (b) audio.validate_fused: stft_mag -> model -> k_mask_istft_score -> k_score_finalize;
  (c) the tail of (a) behind the forward, on a fixed mask: mask_istft(cleaned_mag=True) + stft_mag(clean, 0) + the torch loss
      and si_snr (the parent tree's functions);
  (d) the tail of (b): audio.score_fused on the same mask, the two new launches.
Every shape is warmed up first; then the arms alternate in one process, each timed with device events, for --reps repetitions.
Reports median, p10, p90, min, max in us per batch, the bar of each pair (the slowest repetition of the new arm below the
fastest of the parent's), max |si_snr_a - si_snr_b| and the same for the loss, and for (c) / (d) the algorithmic bytes per frame
of their kernels' reads and writes (the torch ops of (c) counted once per operand).
  python tools/bench_validate.py --parent-root DIR [--reps 16] [--B 32,1] [--only abcd] [--out FILE.json]"""
import argparse
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# (d): noisy 512 + clean 512 (staged) + clean 512 (second read, L2) + mask 1028 in, 48 B per 13-hop tile out
BYTES_PER_FRAME_D = 512 + 512 + 512 + 1028 + 48.0 / 13.0
# (c): mask_istft 512 + 1028 in, 512 + 1028 out; stft_mag(clean) 512 in, 1028 out; the mean reads both planes (2056); si_snr's
# element-wise passes over two audio tensors are left out: a lower bound
BYTES_PER_FRAME_C = (512 + 1028 + 512 + 1028) + (512 + 1028) + 2056


def _load_package(root: str, name: str):
    """The sparsernns_amd package of another tree under another module name (its imports are all relative)."""
    path = os.path.join(root, "sparsernns_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _stats(t):
    t = np.asarray(t)
    return dict(median=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)),
                min=float(t.min()), max=float(t.max()))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="abcd")
    ap.add_argument("--B", default="32,1")
    ap.add_argument("--T", type=int, default=480000)
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out and args.reps < 16:
        ap.error("a recorded result (--out) needs --reps >= 16")

    import torch
    from sparsernns_amd import audio, synth
    from sparsernns_amd.fxpmodel import build_regression_model

    assert torch.cuda.is_available(), "bench_validate.py needs a GPU"
    torch.cuda.set_device(0)
    mk = dict(quantization="w8a16", calib_L=1024, state_headroom_bits=1)   # bench.py's configs[1]
    md, qc, dims = synth.make_model(0.5, **mk)
    model = build_regression_model(md, qc, dims["n_layers"])
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    _load_package(args.parent_root, "sparsernns_amd_parent")
    p_audio = importlib.import_module("sparsernns_amd_parent.audio")
    p_synth = importlib.import_module("sparsernns_amd_parent.synth")
    p_fxpmodel = importlib.import_module("sparsernns_amd_parent.fxpmodel")
    pmd, pqc, pdims = p_synth.make_model(0.5, **mk)
    p_model = p_fxpmodel.build_regression_model(pmd, pqc, pdims["n_layers"])

    n_seg = audio.stft_frames(args.T)
    res = dict(tool="tools/bench_validate.py", workload=f"configs[1] model (dim_scale 0.5 w8a16), T={args.T} ({n_seg} frames)",
               reps=args.reps, order="arms alternating per repetition, one process", lam=0.001,
               a_is="parent tree's audio.validate_batch", c_is="parent tree's mask_istft + stft_mag + torch loss and si_snr",
               unit="us per batch (device events around each arm)", bytes_per_frame_c=BYTES_PER_FRAME_C,
               bytes_per_frame_d=BYTES_PER_FRAME_D, batches={})
    for B in [int(b) for b in args.B.split(",")]:
        g = torch.Generator().manual_seed(B)
        clean = (0.05 * torch.randn(B, args.T, generator=g)).cuda()
        noisy = clean + (0.02 * torch.randn(B, args.T, generator=g)).cuda()
        mask = (0.6 * torch.rand(B, n_seg, 257, generator=g) - 0.3).cuda()

        def run_a():
            return p_audio.validate_batch(p_model, ib, ie, noisy, clean)

        def run_b():
            return audio.validate_fused(model, ib, ie, noisy, clean)

        def run_c():   # validate_batch behind its forward
            cleaned, cleaned_mag = p_audio.mask_istft(noisy, mask, cleaned_mag=True)
            clean_mag = p_audio.stft_mag(clean, sub=0.0)
            score = p_audio.si_snr(cleaned[..., : clean.shape[-1]], clean)
            return 0.001 * torch.mean((cleaned_mag - clean_mag) ** 2, dim=(1, 2)) + (100.0 - score), score

        def run_d():
            return audio.score_fused(noisy, clean, mask)[:2]

        runs = {k: v for k, v in (("a", run_a), ("b", run_b), ("c", run_c), ("d", run_d)) if k in args.only}
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)] for k in runs}
        for r in range(args.reps):
            for k, fn in runs.items():
                ev[k][r][0].record()
                fn()
                ev[k][r][1].record()
        torch.cuda.synchronize()
        out = {}
        for k in runs:
            s = _stats([a.elapsed_time(b) * 1e3 for a, b in ev[k]])
            s["frames_per_s"] = B * n_seg / (s["median"] * 1e-6)
            out[k] = s
        for k, nbytes in (("c", BYTES_PER_FRAME_C), ("d", BYTES_PER_FRAME_D)):
            if k in out:
                out[k]["algorithmic_TB_per_s"] = B * n_seg * nbytes / (out[k]["median"] * 1e-6) / 1e12
        for new, old in (("b", "a"), ("d", "c")):
            if new in out and old in out:
                out[f"{new}_over_{old}"] = out[new]["median"] / out[old]["median"]
                out[f"{new}_slowest_below_{old}_fastest"] = bool(out[new]["max"] < out[old]["min"])
                (l_old, s_old), (l_new, s_new) = runs[old](), runs[new]()
                out[f"max_abs_si_snr_{old}_minus_{new}"] = float((s_old - s_new).abs().max())
                out[f"max_abs_loss_{old}_minus_{new}"] = float((l_old - l_new).abs().max())
                out[f"si_snr_{new}"] = [float(v) for v in s_new[:4]]
        res["batches"][str(B)] = out
        print(f"[bench_validate] B={B}: " + ", ".join(f"{k} {v['median']:.1f} us" for k, v in out.items() if isinstance(v, dict)), flush=True)
        del noisy, clean, mask
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
