#!/usr/bin/env python3
"""kernel_coverage.py: which of the kernels libs5fxp.so registers does the GPU test suite launch?

  python tools/kernel_coverage.py [TRACE_DIR]

(a) the registered kernels: the `.kd` symbols of the gfx950 code object embedded in the built library (no GPU needed);
(b) the launched ones: every *kernel_trace.csv under TRACE_DIR, written by one
      rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python3 -m pytest -m gpu tests
    (gpu_jobs are the place for that run; never combine it with --pmc);
(c) prints every registered kernel that no test launched and is not on ALLOW below, and exits 1 if there is one.
Without TRACE_DIR it lists (a) only."""
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsernns_amd", "libs5fxp.so")
LLVM = "/opt/rocm/llvm/bin"

# Kernels no forward can launch, each with the host condition (s5fxp_api.hip) that rules it out.
# Keys are regular expressions over the demangled name without its parameter list: instantiations that a dispatch
# (S5_DISPATCH_MW) makes for every branch of a runtime `if` whose condition can never hold for them.
ALLOW = [
    (r"k_out2gate<(64|68), (true|false)>",
     "k_out2gate's column budget is mw_for(H), and s5fxp_model_create refuses mw_for(H) > MW_LIMIT_C = 48 (s5fxp_api.hip)"),
]


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return out[:len(names)]


def _key(name: str) -> str:
    """Comparable form of a demangled kernel name: no leading return type, no parameter list, single spaces."""
    name = re.sub(r"^void ", "", name.strip())
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            cut = i
            break
    return re.sub(r"\s+", " ", name[:cut])


def registered(lib: str = LIB):
    """(a): the demangled names of the kernels in the gfx950 code object of `lib`."""
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fb}", lib, os.path.join(d, "junk")])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        syms = subprocess.run([f"{LLVM}/llvm-readelf", "--syms", "--wide", co], capture_output=True, text=True, check=True).stdout
    mangled = sorted({m.group(1) for m in re.finditer(r"\s(\S+)\.kd\s*$", syms, re.M)})
    return sorted({_key(n) for n in _demangle(mangled)})


def launched(trace_dir: str):
    """(b): name -> dispatches over every kernel trace under trace_dir."""
    seen = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                k = _key(r["Kernel_Name"])
                seen[k] = seen.get(k, 0) + 1
    return seen


def main(argv) -> int:
    reg = registered()
    if len(argv) < 2:
        print("\n".join(reg))
        print(f"{len(reg)} kernels registered")
        return 0
    seen = launched(argv[1])
    ours = [k for k in reg if k in seen]
    allowed, missing = [], []
    for k in reg:
        if k in seen:
            continue
        why = next((w for p, w in ALLOW if re.fullmatch(r"s5::" + p, k)), None)
        (allowed if why else missing).append((k, why))
    print(f"launched by the GPU suite: {len(ours)} of {len(reg)} registered kernels")
    print(f"\nnot launched, unreachable from the host (allow-list, {len(allowed)}):")
    for k, why in allowed:
        print(f"  {k}  -- {why}")
    print(f"\nnot launched and not allow-listed ({len(missing)}):")
    for k, _ in missing:
        print(f"  {k}")
    print(f"\nlaunched, with dispatches:")
    for k in ours:
        print(f"  {seen[k]:8d}  {k}")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
