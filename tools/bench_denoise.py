#!/usr/bin/env python3
"""bench_denoise.py: the N-DNS denoising loop (fxprun.py:63-78) around BASELINE configs[1]'s model (dim_scale 0.5, w8a16), on
B clips of T = 480000 samples (3751 STFT frames, the N-DNS clip), per batch:
  (a) audio.denoise: rocFFT + torch ops either side of the model.  With --parent-root DIR it is the package of that tree (the
      parent commit, built there) loaded next to this one, otherwise this tree's -- the function is the same text in both;
  (b) audio.denoise_fused: k_stft_mag -> model -> k_mask_istft;
  (c) the two new launches alone (stft_mag, mask_istft with cleaned_mag, on a fixed mask);
  (d) (a) without its model call (the torch chain alone, on a fixed mask);
  (e) audio.denoise_fused(boundary="int16"): k_stft_mag_i16 -> the int16 forward -> k_mask_istft_i16, 2 bytes per value across
      the model's boundary instead of 4 -- the same cleaned audio as (b) bit for bit, which the tool checks.
Every shape is warmed up first; then the variants alternate in one process, each timed with device events, for --reps
repetitions.  Reports median, p10, p90 in us per batch, frames/s, and for (c) the achieved bytes/s on the algorithmic bytes
(front 512 + 1028, back 512 + 1028 + 512 + 1028 per frame) and its share of the 8 TB/s HBM peak.
  python tools/bench_denoise.py [--reps 14] [--B 32,1] [--only abcde] [--parent-root DIR] [--out FILE.json]
--only a or b with few reps is the workload of a rocprofv3 --kernel-trace --stats run (launch counts)."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BYTES_PER_FRAME_C = (512 + 1028) + (512 + 1028 + 512 + 1028)
HBM_PEAK = 8.0e12


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
    ap.add_argument("--reps", type=int, default=14)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="abcde")
    ap.add_argument("--B", default="32,1")
    ap.add_argument("--T", type=int, default=480000)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out and args.reps < 14:
        ap.error("a recorded result (--out) needs --reps >= 14")

    import importlib
    import torch
    from sparsernns_amd import audio, synth
    from sparsernns_amd.fxpmodel import build_regression_model

    assert torch.cuda.is_available(), "bench_denoise.py needs a GPU"
    torch.cuda.set_device(0)
    mk = dict(quantization="w8a16", calib_L=1024, state_headroom_bits=1)   # bench.py's configs[1]
    md, qc, dims = synth.make_model(0.5, **mk)
    model = build_regression_model(md, qc, dims["n_layers"])
    ib, ie = qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"]
    if args.parent_root:
        _load_package(args.parent_root, "sparsernns_amd_parent")
        p_audio = importlib.import_module("sparsernns_amd_parent.audio")
        p_synth = importlib.import_module("sparsernns_amd_parent.synth")
        p_fxpmodel = importlib.import_module("sparsernns_amd_parent.fxpmodel")
        pmd, pqc, pdims = p_synth.make_model(0.5, **mk)
        p_model = p_fxpmodel.build_regression_model(pmd, pqc, pdims["n_layers"])
    else:
        p_audio, p_model = audio, model

    n_seg = audio.stft_frames(args.T)
    res = dict(tool="tools/bench_denoise.py", workload=f"configs[1] model (dim_scale 0.5 w8a16), T={args.T} ({n_seg} frames)",
               reps=args.reps, order="variants alternating per repetition, one process",
               a_is="parent tree's audio.denoise" if args.parent_root else "this tree's audio.denoise (same text as the parent's)",
               unit="us per batch (device events around each variant)", bytes_per_frame_c=BYTES_PER_FRAME_C, batches={})
    for B in [int(b) for b in args.B.split(",")]:
        g = torch.Generator().manual_seed(B)
        noisy = (0.05 * torch.randn(B, args.T, generator=g)).cuda()
        mask = (2.0 * torch.rand(B, n_seg, 257, generator=g) - 1.0).cuda()
        mask_t = mask.transpose(-1, -2)

        def run_a():
            return p_audio.denoise(p_model, ib, ie, noisy)

        def run_b():
            return audio.denoise_fused(model, ib, ie, noisy)

        def run_c():
            x = audio.stft_mag(noisy)
            return x, audio.mask_istft(noisy, mask, cleaned_mag=True)

        def run_d():   # audio.denoise with the model call taken out
            mag, phase = p_audio.stft_splitter(noisy)
            x = (mag - p_audio.STFT_MAG_MEAN).transpose(-1, -2).contiguous()
            cleaned_mag = mag * (1.0 + mask_t)
            return x, p_audio.stft_mixer(cleaned_mag, phase), cleaned_mag

        def run_e():
            return audio.denoise_fused(model, ib, ie, noisy, boundary="int16")

        runs = {k: v for k, v in (("a", run_a), ("b", run_b), ("c", run_c), ("d", run_d), ("e", run_e)) if k in args.only}
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
        if "c" in out:
            out["c"]["achieved_TB_per_s"] = B * n_seg * BYTES_PER_FRAME_C / (out["c"]["median"] * 1e-6) / 1e12
            out["c"]["share_of_hbm_peak"] = out["c"]["achieved_TB_per_s"] * 1e12 / HBM_PEAK
        if "c" in out and "d" in out:
            out["c_over_d"] = out["c"]["median"] / out["d"]["median"]
            out["c_within_half_of_d"] = bool(out["c"]["median"] <= 0.5 * out["d"]["median"])
        if "a" in out and "b" in out:
            out["b_over_a"] = out["b"]["median"] / out["a"]["median"]
            out["b_faster_than_a"] = bool(out["b"]["median"] < out["a"]["median"])
            # not bit-identical by design: how many FLOOR-quantised input words differ between the two STFTs, and what
            # the fixed-point model (data-dependent exponents, a recurrence) makes of them
            (ca, _, mag), (cb, _, xb, mb) = run_a(), run_b()
            xa = (mag - p_audio.STFT_MAG_MEAN).transpose(-1, -2).contiguous()
            out["max_abs_x_a_minus_b"] = float((xa - xb).abs().max())
            out["input_words"] = xa.numel()
            out["input_words_differing"] = int((torch.floor(xa.double() * 2.0 ** ie) != torch.floor(xb.double() * 2.0 ** ie)).sum())
            out["max_abs_mask_a_minus_b"] = float((model.forward_float(xa) - mb).abs().max())
            out["max_abs_cleaned_a_minus_b"] = float((ca - cb[..., : ca.shape[-1]]).abs().max())
        if "b" in out and "e" in out:
            out["e_over_b"] = out["e"]["median"] / out["b"]["median"]
            (cb, mb_, _, _), (ce, me_, _, _) = run_b(), run_e()
            out["e_equals_b_bitwise"] = bool(torch.equal(cb, ce) and torch.equal(mb_, me_))
            assert out["e_equals_b_bitwise"], f"B={B}: the int16 boundary changed the cleaned audio"
        res["batches"][str(B)] = out
        print(f"[bench_denoise] B={B}: " + ", ".join(f"{k} {v['median']:.1f} us" for k, v in out.items() if isinstance(v, dict)), flush=True)
        del noisy, mask, mask_t
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
