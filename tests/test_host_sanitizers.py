"""The library's host code and the C oracle under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU only.

Three stand-alone programs under tests/host/, each with its own main -- nothing here loads sanitized code into python:
  host_san.cpp   linked against sparsernns_amd/csrc/s5fxp_api.hip with the host half compiled -fsanitize=address,undefined: descriptor
                 validation, the packers, the size queries, s5fxp_push_desc_check, s5fxp_stage_err's validation loop and the argument
                 checks of every launching entry.  It hands the library an address that is not device memory, so it must never meet
                 a device: it leaves with status 77 when it sees one, this module hides the devices from it, and every test here
                 skips where torch sees a GPU.
  abi_layout.c   include/s5fxp.h read by a C11 compiler: the layout it prints must be the one sparsernns_amd/_lib.py declares.
  oracle_san.c   oracle/s5fxp_ref.c with the flags of the Makefile's asan target, on the committed fixtures, against the plain
                 library through oracle/cref.py.
The sanitized compile of the library is the expensive step (minutes: the device code is compiled with it).  It is done once per state
of csrc/ and the header, into oracle/_build/host_san/<hash>/, and reused by every later run.
"""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
CSRC = os.path.join(ROOT, "sparsernns_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "s5fxp.h")
SAN_ROOT = os.path.join(ROOT, "oracle", "_build", "host_san")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
LIB_FLAGS = ["--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-value"] + [a for f in SAN for a in ("-Xarch_host", f)]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:halt_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
REPORTS = ("runtime error:", "ERROR: AddressSanitizer", "LeakSanitizer")
DEVICE_SEEN = 77

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="the host driver must never meet a device")


def _sha(paths, extra=""):
    h = hashlib.sha256(extra.encode())
    for p in paths:
        h.update(os.path.relpath(p, ROOT).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _run(cmd, timeout, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, **kw)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    return r


def _clean(stderr):
    found = [line for line in stderr.splitlines() if any(k in line for k in REPORTS)]
    assert not found, "\n".join(found) + "\n--- whole stderr ---\n" + stderr[-20000:]


@pytest.fixture(scope="module")
def host_san_exe():
    """The driver linked against the sanitized library object; both cached by content hash."""
    assert os.path.exists(HIPCC), f"{HIPCC} not found: the sanitized host build needs hipcc"
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".inc"))) + [HEADER]
    key = _sha(srcs, " ".join(LIB_FLAGS))
    out = os.path.join(SAN_ROOT, key)
    if os.path.isdir(SAN_ROOT):
        for stale in os.listdir(SAN_ROOT):   # one state of the sources at a time: the object is tens of megabytes
            if stale != key:
                shutil.rmtree(os.path.join(SAN_ROOT, stale), ignore_errors=True)
    os.makedirs(out, exist_ok=True)
    obj = os.path.join(out, "s5fxp_api.o")
    if not os.path.exists(obj):
        tmp = obj + f".{os.getpid()}.tmp"
        _run([HIPCC] + LIB_FLAGS + ["-c", os.path.join(CSRC, "s5fxp_api.hip"), "-o", tmp], timeout=2400)
        os.replace(tmp, obj)
    driver = os.path.join(HOST, "host_san.cpp")
    exe = os.path.join(out, "host_san_" + _sha([driver], key))
    if not os.path.exists(exe):
        rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(HIPCC))), "include")
        dobj, tmp = exe + ".o", exe + f".{os.getpid()}.tmp"
        _run([HIPCC, "-x", "c++", "-I" + rocm_inc, "-D__HIP_PLATFORM_AMD__", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + SAN +
             ["-c", driver, "-o", dobj], timeout=300)
        _run([HIPCC, "--offload-arch=gfx950"] + SAN + [obj, dobj, "-o", tmp], timeout=300)
        os.replace(tmp, exe)
    return exe


def _host_san(exe, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", **SAN_ENV)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=env)


@pytest.fixture(scope="module")
def host_san_run(host_san_exe, tmp_path_factory):
    out = tmp_path_factory.mktemp("host_san")
    r = _host_san(host_san_exe, "--out", str(out))
    if r.returncode == DEVICE_SEEN:
        pytest.skip("the driver saw a device and left")
    return r, out


def test_host_paths_are_clean_under_asan_and_ubsan(host_san_run):
    r, _ = host_san_run
    cases = re.findall(r"^case (\S+)$", r.stderr, re.M)
    _clean(r.stderr)
    assert r.returncode == 0, r.stderr[-20000:]
    assert "FAIL" not in r.stderr and "host_san: 0 unexpected return codes" in r.stderr, r.stderr[-5000:]
    # every family of cases ran (a driver that returned early would be clean too)
    for prefix in ("create_recipe_H", "create_live_", "create_w4", "create_rails", "validate_", "float_pack_ds", "float_validate_",
                   "stft_frames", "score_workspace_bytes", "score_clips_workspace_bytes", "stage_err_workspace_bytes",
                   "stream_frames_out_hops", "strerror", "push_desc_", "stage_err_refusals", "stage_err_4096_pairs", "entries_ops",
                   "entries_scans", "entries_audio", "entries_stream", "entries_step_clips", "entries_forwards"):
        assert any(c.startswith(prefix) for c in cases), prefix
    assert len(cases) >= 100 and len(set(cases)) == len(cases), len(cases)


def test_guard_leaves_before_the_first_case(host_san_exe):
    r = _host_san(host_san_exe, "--expect-device")
    assert r.returncode == DEVICE_SEEN, (r.returncode, r.stderr[-2000:])
    assert "case " not in r.stderr and r.stdout == "", r.stderr
    _clean(r.stderr)


def test_sanitized_float_packer_writes_the_bytes_the_library_writes(host_san_run):
    """The blob the driver packed in a malloc of exactly blob_bytes == the plain libs5fxp.so's for the same descriptor (the route of
    test_float_model.py::test_packed_blob_layout: s5fxp_float_model_blob_bytes + s5fxp_float_model_pack through _lib)."""
    from sparsernns_amd import _lib

    r, out = host_san_run
    assert r.returncode == 0, r.stderr[-5000:]
    raw = np.fromfile(os.path.join(out, "float_desc.bin"), dtype=np.int32)
    n_layers, d_in, H, P, d_out, has_scale, has_bias = (int(v) for v in raw[:7])
    assert (n_layers, d_in, H, P, d_out) == (1, 257, 48, 32, 257)
    data = raw[7:].view(np.float32)
    off = 0
    keep = []

    def take(n):
        nonlocal off
        a = np.ascontiguousarray(data[off:off + n])
        assert a.size == n
        off += n
        keep.append(a)
        return a.ctypes.data_as(_lib.F32P)

    desc = _lib.FloatModelDesc(n_layers=n_layers, d_in=d_in, H=H, P=P, d_out=d_out)
    desc.enc_w, desc.enc_b = take(d_in * H), take(H)
    layers = (_lib.FloatLayerDesc * n_layers)()
    for l in layers:
        l.mean, l.var = take(H), take(H)
        l.scale = take(H) if has_scale else None
        l.bias = take(H) if has_bias else None
        l.lambda_bar, l.B_bar, l.C, l.D, l.w2, l.b2 = take(2 * P), take(P * H * 2), take(H * P * 2), take(H), take(H * H), take(H)
    desc.layers = C.cast(layers, C.POINTER(_lib.FloatLayerDesc))
    desc.dec_w, desc.dec_b = take(H * d_out), take(d_out)
    assert off == data.size
    nbytes = _lib.lib.s5fxp_float_model_blob_bytes(C.byref(desc))
    want = np.full(nbytes, 0x5a, dtype=np.uint8)
    assert _lib.lib.s5fxp_float_model_pack(C.byref(desc), want.ctypes.data, nbytes) == _lib.S5FXP_OK
    got = np.fromfile(os.path.join(out, "float_blob.bin"), dtype=np.uint8)
    assert got.size == nbytes > 4 * (260 * H + H * 272)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {nbytes} bytes differ, first at {int(np.argmax(got != want))}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the header, read by a C compiler
# ---------------------------------------------------------------------------------------------------------------------------------
def _twins():
    from sparsernns_amd import _lib
    return {"s5fxp_dense_desc": _lib.DenseDesc, "s5fxp_ssm_desc": _lib.SSMDesc, "s5fxp_norm_desc": _lib.NormDesc,
            "s5fxp_layer_desc": _lib.LayerDesc, "s5fxp_model_desc": _lib.ModelDesc, "s5fxp_layer_trace": _lib.LayerTrace,
            "s5fxp_forward_opts": _lib.ForwardOpts, "s5fxp_push_desc": _lib.PushDesc, "s5fxp_float_layer_desc": _lib.FloatLayerDesc,
            "s5fxp_float_model_desc": _lib.FloatModelDesc, "s5fxp_float_fq_site": _lib.FloatFqSite, "s5fxp_stage_pair": _lib.StagePair,
            "s5fxp_stage_err_rec": _lib.StageErrRec}


@pytest.fixture(scope="module")
def abi(tmp_path_factory):
    gcc = shutil.which("gcc")
    assert gcc, "gcc not found: the header must be read by a C compiler"
    exe = str(tmp_path_factory.mktemp("abi") / "abi_layout")
    _run([gcc, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HOST, "abi_layout.c")], timeout=120)
    structs, enums, macros = {}, {}, {}
    for line in _run([exe], timeout=60).stdout.splitlines():
        w = line.split()
        if w[0] == "struct":
            structs[w[1]] = (int(w[2]), [])
        elif w[0] == "field":
            structs[w[1]][1].append((w[2], int(w[3]), int(w[4])))
        else:
            assert w[0] in ("enum", "macro"), line
            (enums if w[0] == "enum" else macros)[w[1]] = int(w[2])
    return structs, enums, macros


def test_header_structs_have_the_layout_ctypes_declares(abi):
    from sparsernns_amd import _lib

    structs, _, _ = abi
    twins = _twins()
    hdr = open(HEADER).read()
    in_header = set(re.findall(r"\}\s*(s5fxp_\w+)\s*;", hdr))
    assert in_header == set(structs), f"structs of the header that abi_layout.c does not print, or the reverse: {sorted(in_header ^ set(structs))}"
    assert in_header == set(twins), f"header structs without a ctypes twin, or the reverse: {sorted(in_header ^ set(twins))}"
    declared = {c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, C.Structure) and c.__module__ == _lib.__name__}
    assert declared == set(twins.values()), f"ctypes structures without a header struct: {sorted(c.__name__ for c in declared ^ set(twins.values()))}"
    for name, cls in twins.items():
        size, fields = structs[name]
        assert size == C.sizeof(cls), (name, size, C.sizeof(cls))
        assert [f for f, _, _ in fields] == [f[0] for f in cls._fields_], name
        for f, off, fsize in fields:
            d = getattr(cls, f)
            assert (off, fsize) == (d.offset, d.size), (name, f, (off, fsize), (d.offset, d.size))
    # the sizes the header's comments promise
    assert structs["s5fxp_push_desc"][0] == 32 and structs["s5fxp_stage_pair"][0] == 88 and structs["s5fxp_stage_err_rec"][0] == 1104


def test_header_constants_have_the_values_ctypes_uses(abi):
    from sparsernns_amd import _lib

    _, enums, macros = abi
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    in_header = {m.split("=")[0].strip() for body in re.findall(r"\benum\s*\{(.*?)\}", hdr, re.S) for m in body.split(",") if m.strip()}
    assert in_header == set(enums), f"enumerators abi_layout.c does not print, or the reverse: {sorted(in_header ^ set(enums))}"
    numeric = set(re.findall(r"^#define\s+(S5FXP_\w+)\s+\(?-?\d+\)?\s*$", hdr, re.M))
    assert numeric == set(macros), sorted(numeric ^ set(macros))
    matched = 0
    for name, value in {**enums, **macros}.items():
        for py in (name, name[len("S5FXP_"):]):
            have = getattr(_lib, py, None)
            if isinstance(have, int) and not isinstance(have, bool):
                assert have == value, (name, value, py, have)
                matched += 1
                break
    assert matched >= 30, matched   # the error codes, status bits, flags, paths, push and stage constants all have a twin
    assert macros["S5FXP_VERSION"] == _lib.lib.s5fxp_version()


# ---------------------------------------------------------------------------------------------------------------------------------
# the C oracle
# ---------------------------------------------------------------------------------------------------------------------------------
ORACLE_MAGIC = 0x53354F52


@pytest.fixture(scope="module")
def oracle_san_exe():
    _run(["make", "-C", os.path.join(ROOT, "oracle"), "asan-exe"], timeout=300)
    return os.path.join(ROOT, "oracle", "_build", "oracle_san")


def _int_fields(s, skip=()):
    return [getattr(s, n) for n, t in s._fields_ if t is C.c_int32 and n not in skip]


def _oracle_input(cm, x, x_bits, x_exp):
    """The marshalled model of a cref.CModel, field by field in the order of its structs (the format of tests/host/oracle_san.c)."""
    words = []
    put = lambda *v: words.append(np.asarray(v, dtype=np.int32))
    arr = lambda ptr, n: words.append(np.ctypeslib.as_array(ptr, shape=(n,)).astype(np.int32))

    def dense(d):
        put(d.K, d.M)
        arr(d.w, d.K * d.M)
        put(1 if d.bias else 0)
        if d.bias:
            arr(d.bias, d.M)
        put(*_int_fields(d, ("K", "M")))

    B, L = x.shape[:2]
    put(ORACLE_MAGIC, cm.n_layers, x_bits, x_exp, B, L)
    dense(cm.model.enc)
    H = cm.H
    for i in range(cm.n_layers):
        l = cm.layers[i]
        put(1 if l.bn.scale else 0, 1 if l.bn.bias else 0)
        for p in (l.bn.minus_mean, l.bn.invsq_var, l.bn.scale, l.bn.bias):
            if p:
                arr(p, H)
        put(*_int_fields(l.bn))
        s = l.ssm
        put(s.H, s.P)
        for p, n in ((s.a_re, s.P), (s.a_im, s.P), (s.b_re, s.P * H), (s.b_im, s.P * H), (s.c_re, H * s.P), (s.c_im, H * s.P), (s.d, H)):
            arr(p, n)
        put(*_int_fields(s, ("H", "P")))
        dense(l.out2)
        put(*_int_fields(l))
        put(*list(l.lut))
    dense(cm.model.dec)
    words.append(np.ascontiguousarray(x, dtype=np.int32).ravel())
    return np.concatenate([w.ravel() for w in words])


def _fixture(name):
    if name.startswith("ref_"):
        from reference_fixtures import load_model_fixture
        meta, export, x, _, _, _ = load_model_fixture(name)
    else:
        from test_cpu_suite import load_golden
        _, meta, export, x, _, _ = load_golden(name)
    return export, x, int(meta["x_bits"]), int(meta["x_exp"])


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b_bnscale", "ref_tiny_w4a8", "ref_ndns05_b2"])
def test_c_oracle_is_clean_and_gives_the_plain_library_s_bits(oracle_san_exe, tmp_path, name):
    export, x, x_bits, x_exp = _fixture(name)
    if name == "ref_ndns05_b2":
        assert x.shape == (2, 33, 257)
    cm = cref.CModel(export)
    y, yb, ye, traces = cm.forward(x, x_bits, x_exp, trace=True)      # the unsanitized libs5fxp_ref.so
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    _oracle_input(cm, x, x_bits, x_exp).tofile(fin)
    r = subprocess.run([oracle_san_exe, str(fin), str(fout)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    _clean(r.stderr)
    assert r.returncode == 0, r.stderr[-5000:]
    got = np.fromfile(fout, dtype=np.int32)
    assert tuple(got[:3]) == (0, yb, ye)
    off = 3

    def take(shape):
        nonlocal off
        n = int(np.prod(shape))
        a = got[off:off + n]
        assert a.size == n
        off += n
        return a.reshape(shape)

    assert np.array_equal(take(y.shape), y)
    for i, t in enumerate(traces):
        for k in cref.TRACE_KEYS:
            assert np.array_equal(take(t[k].shape), t[k]), (i, k)
        assert (int(take(())), int(take(()))) == (t["pre_s5_exp"], t["residadd_exp"]), i
    assert off == got.size
