#!/bin/bash
# ab_cgate_ft32.sh: the gate kernel on 32-frame tiles with three-wave workgroups (the default at dim_scale 0.5) against the 64-frame
# six-wave form it replaced (S5FXP_CGATE_FT64=1).  With the sigmoid table sized exactly, five 32-frame workgroups fit a CU's LDS
# and registers (15 waves instead of 12).  Parity first, then kernel durations per grid size of the 32-frame kernel
# (S5FXP_WGS_CGATE32), then the 64-frame kernel.
python3 -m pytest tests/test_variant_matrix.py -x -q -m gpu -k "default or cgate_ft64 or wgs" 2>&1 | tail -1
for w in 1024 1280 1536 2048; do export S5FXP_WGS_CGATE32=$w; echo "== FT32, $w workgroups per launch"; BENCH_ARGS="--steps 48 --no-one-batch-pass" bash tools/run_variants.sh base 2>&1 | grep -E "cgate_p"; done
unset S5FXP_WGS_CGATE32
export S5FXP_CGATE_FT64=1
echo "== FT64"; BENCH_ARGS="--steps 48 --no-one-batch-pass" bash tools/run_variants.sh base 2>&1 | grep -E "cgate_p"
unset S5FXP_CGATE_FT64
