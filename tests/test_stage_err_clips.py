"""s5fxp_stage_err_clips and verify.compare_clips: the stage comparison over clips of different lengths.

The reference of every record is ``verify.stage_errors_clips_host``, the NumPy float64 statement (gather the rows inside, scale
clip by clip, then ``stage_errors_host``'s arithmetic), itself held against ``stage_errors_host`` on the per-clip slices.  The
bounds are tests/test_stage_err.py's, stated by the arithmetic:
  * counts, both histograms, max_abs and max_rel: exact;
  * each of the four sums adds n non-negative doubles, so any summation order is within (n - 1) * 2^-53 relative of the exact
    value: two orders differ by at most 2 n 2^-53 relative;
  * the variance sum_sq / n - mean^2: 4 n 2^-53 * sum_sq / n absolute.
Every masked row of both sides holds NaN or 0x7F7F7F7F poison: it must be invisible.
"""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_stage_err import make_values

gpu = pytest.mark.gpu
EPS = 2.0 ** -53
EXACT = ("n", "n_nonfinite", "n_equal", "n_ref_nonzero", "max_abs", "max_rel")
SUM_KEYS = ("sum_abs", "sum_sq", "sum_ref_sq", "sum_rel")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x7F7F7F7F


def variance(r):
    nf = r["n"] - r["n_nonfinite"]
    return r["sum_sq"] / nf - (r["sum_abs"] / nf) ** 2 if nf else 0.0


def assert_record(got, want, what):
    """A device record against the host record of the same values, to the bounds of the module docstring (a copy of
    tests/test_stage_err.py's)."""
    for k in EXACT:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("hist_abs", "hist_rel"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    n = want["n"]
    for k in SUM_KEYS:
        assert abs(got[k] - want[k]) <= 2 * n * EPS * abs(want[k]), (what, k, got[k], want[k])
    assert abs(variance(got) - variance(want)) <= 4 * EPS * want["sum_sq"], (what, variance(got), variance(want))
    for k in ("abs_error_med_lo", "abs_error_med_hi", "rel_error_med_lo", "rel_error_med_hi", "equal_share"):
        assert got[k] == want[k], (what, k)


def poisoned(a, b, lens, row0=0):
    """Copies of (a, b) whose rows outside ``row0 + r < lens[e]`` hold poison: NaN in b, NaN (float32 a) or 0x7F7F7F7F in a."""
    a, b = a.copy(), b.copy()
    for e, n in enumerate(lens):
        m = min(max(int(n) - row0, 0), a.shape[1])
        b[e, m:] = np.nan if e % 2 else np.float32(np.array(POISON, dtype=np.uint32).view(np.float32))
        a[e, m:] = np.nan if a.dtype == np.float32 else POISON
    return a, b


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_at_version_115():
    from sparsernns_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "s5fxp.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("s5fxp_stage_err_clips", "s5fxp_stage_err_clips_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name) and hasattr(_lib.lib, name), name
    assert _lib.lib.s5fxp_version() == 115 and "#define S5FXP_VERSION 115" in hdr


def test_pair_struct_has_the_layout_the_header_declares(tmp_path):
    """120 bytes (the static_assert of the .hip states the same), and every field where a C compiler puts it."""
    from sparsernns_amd import _lib, verify

    S = verify.StagePairClips
    assert C.sizeof(S) == 120 and C.sizeof(_lib.StagePair) == 88 and S.box.offset == 0
    gcc = shutil.which("gcc")
    assert gcc, "gcc not found: the header must be read by a C compiler"
    fields = [f[0] for f in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "s5fxp.h"\nint main(void) {\n'
                   '    printf("size %zu\\n", sizeof(s5fxp_stage_pair_clips));\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(s5fxp_stage_pair_clips, {f}), sizeof(((s5fxp_stage_pair_clips *)0)->{f}));\n'
                             for f in fields) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([gcc, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True, timeout=120)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert lines[0] == "size 120"
    for f, line in zip(fields, lines[1:]):
        d = getattr(S, f)
        assert line == f"{f} {d.offset} {d.size}", (line, d.offset, d.size)
    assert "static_assert(sizeof(s5fxp_stage_pair_clips) == 120" in open(os.path.join(ROOT, "sparsernns_amd", "csrc", "s5fxp_api.hip")).read()


def test_entry_refuses_bad_arguments_before_the_device():
    from sparsernns_amd import _lib, verify
    from sparsernns_amd._lib import lib

    FAKE = 1 << 20

    def one(**kw):
        arr = (verify.StagePairClips * 1)()
        d = arr[0]
        b = d.box
        b.a, b.b, b.a_kind, b.a_exp, b.nb, b.rows, b.cols, b.flags = FAKE, FAKE, _lib.STAGE_I32, 15, 2, 3, 4, 0
        for k in range(3):
            b.a_stride[k] = b.b_stride[k] = (12, 4, 1)[k]
        d.lens, d.a_exp_dev, d.a_exp_stride, d.row0, d.reserved = FAKE, None, 0, 0, 0
        for k, v in kw.items():
            setattr(d if hasattr(type(d), k) and k != "box" else b, k, v)
        return arr

    need = lib.s5fxp_stage_err_clips_workspace_bytes(1)
    assert need == 256 + 512 * C.sizeof(_lib.StageErrRec)
    assert lib.s5fxp_stage_err_clips_workspace_bytes(0) == 0 and lib.s5fxp_stage_err_clips_workspace_bytes(4097) == 0
    assert lib.s5fxp_stage_err_clips_workspace_bytes(4096) == 4096 * 128 + 4096 * 4 * 1104
    call = lambda arr, n=1, out=FAKE, ws=FAKE, nbytes=need: lib.s5fxp_stage_err_clips(arr, n, out, ws, nbytes, None)
    assert call(None) == _lib.S5FXP_EBADARG
    assert call(one(), out=None) == _lib.S5FXP_EBADARG and call(one(), ws=None) == _lib.S5FXP_EBADARG
    assert call(one(), n=0) == _lib.S5FXP_EBADARG and call(one(), n=4097) == _lib.S5FXP_EBADARG
    for kw in (dict(a_kind=2), dict(a_kind=-1), dict(flags=2), dict(flags=-1), dict(a_exp=-1), dict(a_exp=41), dict(nb=-1),
               dict(rows=-1), dict(cols=-1), dict(a=None), dict(b=None), dict(lens=None), dict(row0=-1), dict(reserved=1),
               dict(nb=2 ** 31 - 1, rows=2 ** 31 - 1, cols=2 ** 31 - 1),   # the wrap rule on the padded box, far beyond 64 bits
               dict(nb=512, rows=2 ** 31 - 1, cols=2)):                    # ... and just beyond it
        assert call(one(**kw)) == _lib.S5FXP_EBADARG, kw
    # everything legal, but no room: refused on the host as well
    for kw in (dict(), dict(a_kind=_lib.STAGE_F32, a_exp=99), dict(flags=_lib.STAGE_RELU_A), dict(row0=2 ** 31 - 1),
               dict(a_exp=99, a_exp_dev=FAKE, a_exp_stride=128),           # the device exponent replaces a_exp
               dict(rows=0, a=None, b=None, lens=None), dict(nb=511, rows=2 ** 31 - 1, cols=2)):
        assert call(one(**kw), nbytes=need - 1) == _lib.S5FXP_EWORKSPACE, kw


HOST_LENS = (41, 0, 1, 31, 32, 33, 50, 7)   # clip 0 is whole: make_values' NaN and infinities are inside


@pytest.mark.parametrize("kind,relu,row0", [("i32", False, 0), ("i32", True, 0), ("i32", False, 16), ("f32", False, 0), ("f32", True, 5)])
def test_host_statement_is_the_fold_of_the_per_clip_host_statement(kind, relu, row0):
    """Counts and histograms add, maxima take the max, sums agree to 2 n 2^-53 relative."""
    from sparsernns_amd import verify

    rows = 41
    a, b = make_values((len(HOST_LENS), rows, 37), kind, 0, seed=61)
    exps = [3, 40, 0, 15, 15, 31, 7, 22]
    ap, bp = poisoned(a, b, HOST_LENS, row0)
    whole = verify.stage_errors_clips_host([(ap, bp, np.array(HOST_LENS, dtype=np.int32), exps, relu, row0)])[0]
    parts = []
    for e, n in enumerate(HOST_LENS):
        m = min(max(n - row0, 0), rows)
        parts.append(verify.stage_errors_host([(a[e, :m], b[e, :m], exps[e], relu)])[0])
    n = sum(p["n"] for p in parts)
    assert whole["n"] == n == sum(min(max(v - row0, 0), rows) for v in HOST_LENS) * 37 > 0
    for k in ("n", "n_nonfinite", "n_equal", "n_ref_nonzero", "hist_abs", "hist_rel"):
        assert np.array_equal(np.asarray(whole[k]), sum(np.asarray(p[k]) for p in parts)), k
    for k in ("max_abs", "max_rel"):
        assert whole[k] == max(p[k] for p in parts), k
    for k in SUM_KEYS:
        s = sum(p[k] for p in parts)
        assert abs(whole[k] - s) <= 2 * n * EPS * abs(s), (k, whole[k], s)
    assert whole["n_nonfinite"] > 0
    # one exponent for all clips is the per-clip list of that exponent
    one = verify.stage_errors_clips_host([(ap, bp, np.array(HOST_LENS, dtype=np.int32), 9, relu, row0)])[0]
    lst = verify.stage_errors_clips_host([(ap, bp, np.array(HOST_LENS, dtype=np.int32), [9] * 8, relu, row0)])[0]
    assert all(np.array_equal(np.asarray(one[k]), np.asarray(lst[k])) for k in one)


def test_host_statement_edges():
    from sparsernns_amd import verify

    a, b = make_values((3, 9, 8), "i32", 4, seed=62)
    ap, bp = poisoned(a, b, (0, 0, 0))
    zero = verify.stage_errors_clips_host([(ap, bp, np.zeros(3, dtype=np.int32), 4)])[0]
    assert all(not np.any(zero[k]) for k in EXACT + SUM_KEYS + ("hist_abs", "hist_rel")) and zero["abs_error_mean"] == 0.0
    neg = verify.stage_errors_clips_host([(ap, bp, np.array([-5, 0, -1], dtype=np.int32), 4)])[0]
    assert neg["n"] == 0
    # an exponent outside 0..40 sends the clip's elements to n and n_nonfinite and to nothing else
    lens = np.array([9, 4, 9], dtype=np.int32)
    for bad in (-1, 41, 2 ** 31 - 1, -2 ** 31):
        r = verify.stage_errors_clips_host([(a, b, lens, [4, bad, 4])])[0]
        keep = verify.stage_errors_clips_host([(a, b, np.array([9, 0, 9], dtype=np.int32), [4, 4, 4])])[0]
        assert r["n"] == keep["n"] + 4 * 8 and r["n_nonfinite"] == keep["n_nonfinite"] + 4 * 8
        for k in ("n_equal", "n_ref_nonzero", "max_abs", "max_rel", "sum_abs", "sum_sq", "sum_ref_sq", "sum_rel", "hist_abs", "hist_rel"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(keep[k])), (bad, k)
    # a float32 a has no exponent: the list is ignored
    af, bf = make_values((3, 9, 8), "f32", 0, seed=63)
    assert verify.stage_errors_clips_host([(af, bf, lens, [99, -3, 41])])[0]["n_nonfinite"] == \
        verify.stage_errors_clips_host([(af, bf, lens)])[0]["n_nonfinite"]
    # lens beyond the box are the whole box
    full = verify.stage_errors_clips_host([(a, b, np.array([100, 9, 2 ** 31 - 1], dtype=np.int32), 4)])[0]
    plain = verify.stage_errors_host([(a, b, 4)])[0]
    assert all(np.array_equal(np.asarray(full[k]), np.asarray(plain[k])) for k in EXACT + ("hist_abs", "hist_rel"))
    with pytest.raises(ValueError):
        verify.stage_errors_clips_host([(a[0], b[0], lens[:1], 4)])


def test_clip_pair_describes_padded_views_without_a_copy():
    import torch
    from sparsernns_amd import _lib, verify

    n, L, H = 4, 10, 6
    plane, ref = torch.zeros(n, L, H, dtype=torch.int32), torch.ones(n, L, H)
    lens = torch.tensor([10, 0, 3, 7], dtype=torch.int32)
    status = torch.arange(n * _lib.STATUS_WORDS, dtype=torch.int32)
    d = verify.StagePairClips()
    p = verify.clip_pair(plane, ref, lens, relu_a=True, a_exp_dev=status[8 + 8 * 1 + 4:], a_exp_stride=_lib.STATUS_WORDS)
    p.fill(d)
    assert (d.box.nb, d.box.rows, d.box.cols, d.box.flags, d.row0, d.reserved) == (n, L, H, _lib.STAGE_RELU_A, 0, 0)
    assert d.lens == lens.data_ptr() and d.a_exp_dev == status.data_ptr() + 4 * 20 and d.a_exp_stride == 128
    assert p.host()[3] == [20, 148, 276, 404]
    one = verify.clip_pair(plane[2:3], ref[2:3], lens[2:3], a_exp=5)      # one clip
    one.fill(d)
    assert d.box.nb == 1 and d.box.a == plane.data_ptr() + 4 * 2 * L * H and d.lens == lens.data_ptr() + 8 and d.a_exp_dev is None
    t = verify.clip_pair(plane[:, 4:8], ref[:, 4:8], lens, a_exp=5, row0=4)   # one time bucket
    t.fill(d)
    assert (d.box.rows, d.row0) == (4, 4) and d.box.b == ref.data_ptr() + 4 * 4 * H and list(d.box.a_stride) == [L * H, H, 1]
    for bad in (lambda: verify.clip_pair(plane[0], ref[0], lens[:1], 5), lambda: verify.clip_pair(plane, ref, lens[:3], 5),
                lambda: verify.clip_pair(plane, ref, lens.long(), 5), lambda: verify.clip_pair(plane, ref, lens),
                lambda: verify.clip_pair(plane, ref, lens, 5, row0=-1),
                lambda: verify.clip_pair(plane, ref, lens, a_exp_dev=status[:200], a_exp_stride=128)):
        with pytest.raises(ValueError):
            bad()
    # pairs that are not on a GPU take the host statement
    a, b = make_values((n, L, H), "i32", 9, seed=1)
    got = verify.stage_errors_clips([verify.clip_pair(torch.from_numpy(a), torch.from_numpy(b), lens, 9)])
    want = verify.stage_errors_clips_host([(a, b, lens.numpy(), 9)])
    assert all(np.array_equal(np.asarray(got[0][k]), np.asarray(want[0][k])) for k in want[0])
    assert "| x | clip 3 |" in verify.table_markdown([dict(name="x", clip=3, **want[0])])


# ----------------------------------------------------------------------------------------------------------------------
# MI355X: records against the host statement
# ----------------------------------------------------------------------------------------------------------------------
LENS8 = (0, 1, 31, 32, 33, 64, 65, 100)


@functools.lru_cache(maxsize=None)
def _suite():
    """Every case in ONE call, run twice -> {name: (device record, host record, second run, pair)}."""
    import torch
    from sparsernns_amd import _lib, verify

    names, pairs = [], []
    cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    lens8 = np.array(LENS8, dtype=np.int32)
    # int32 with a per-clip device exponent at stride 128 (one of them outside 0..40), inside fake status words
    a, b = make_values((8, 100, 96), "i32", 15, 71)   # b equals a * 2^-15 on part of the elements
    ap, bp = poisoned(a, b, LENS8)
    status = np.full(8 * _lib.STATUS_WORDS, 12345, dtype=np.int32)
    exps = [0, 7, 40, 41, 15, 31, -1, 22]
    status[8 + 8 * 2 + 4::_lib.STATUS_WORDS] = exps
    sd, ld = cuda(status), cuda(lens8)
    for relu in (False, True):
        names.append(f"8x100x96 i32 device exponents relu={relu}")
        pairs.append(verify.clip_pair(cuda(ap), cuda(bp), ld, relu_a=relu, a_exp_dev=sd[8 + 8 * 2 + 4:], a_exp_stride=_lib.STATUS_WORDS))
    # a static exponent; one clip of the box; time buckets (row0 > 0)
    apd, bpd = cuda(ap), cuda(bp)
    names.append("8x100x96 i32 exp15")
    pairs.append(verify.clip_pair(apd, bpd, ld, 15))
    for e in (0, 4, 7):
        names.append(f"clip {e} of 8x100x96")
        pairs.append(verify.clip_pair(apd[e:e + 1], bpd[e:e + 1], ld[e:e + 1], a_exp_dev=sd[e * _lib.STATUS_WORDS + 28:], a_exp_stride=_lib.STATUS_WORDS))
    for t0, t1 in ((13, 26), (32, 64), (91, 100)):
        a2, b2 = poisoned(a, b, LENS8, t0)   # poison where THIS bucket is masked; inside, the values of the box's rows t0..
        a3, b3 = a.copy(), b.copy()
        a3[:, t0:t1], b3[:, t0:t1] = a2[:, :t1 - t0], b2[:, :t1 - t0]
        names.append(f"time bucket {t0}..{t1}")
        pairs.append(verify.clip_pair(cuda(a3)[:, t0:t1], cuda(b3)[:, t0:t1], ld, 9, True, row0=t0))
    # float32 a
    a, b = make_values((5, 40, 257), "f32", 0, 72)
    l5 = np.array([40, 0, 33, 7, 100], dtype=np.int32)
    ap, bp = poisoned(a, b, l5)
    names.append("5x40x257 f32")
    pairs.append(verify.clip_pair(cuda(ap), cuda(bp), cuda(l5)))
    # the halves of an interleaved complex64 plane: column stride 2 on b
    a, b = make_values((3, 33, 32), "i32", 12, 73)
    _, b2 = make_values((3, 33, 32), "i32", 12, 74)
    l3 = np.array([33, 1, 32], dtype=np.int32)
    ap, bp = poisoned(a, b, l3)
    _, b2p = poisoned(a, b2, l3)
    z = torch.view_as_complex(cuda(np.stack([bp, b2p], axis=-1)))
    for half in (0, 1):
        names.append(f"3x33x32 complex half {half}")
        pairs.append(verify.clip_pair(cuda(ap), torch.view_as_real(z)[..., half], cuda(l3), 12))
    # lens all zero; a zero extent
    names += ["lens all zero", "zero extent"]
    pairs += [verify.clip_pair(apd, bpd, cuda(np.zeros(8, dtype=np.int32)), 15), verify.clip_pair(apd[:, 5:5], bpd[:, 5:5], ld, 15)]
    # many workgroups: 64 shares over a box whose clips end inside them
    a, b = make_values((5, 600, 128), "i32", 15, 75)
    l600 = np.array([600, 3, 0, 511, 257], dtype=np.int32)
    ap, bp = poisoned(a, b, l600)
    names.append("5x600x128 i32")
    pairs.append(verify.clip_pair(cuda(ap), cuda(bp), cuda(l600), 15))
    got = verify.stage_errors_clips(pairs)
    again = verify.stage_errors_clips(pairs)
    want = verify.stage_errors_clips_host(pairs)   # the same device tensors, copied back
    return {n: (g, w, g2, p) for n, g, w, g2, p in zip(names, got, want, again, pairs)}


SUITE_NAMES = (["8x100x96 i32 device exponents relu=False", "8x100x96 i32 device exponents relu=True", "8x100x96 i32 exp15"]
               + [f"clip {e} of 8x100x96" for e in (0, 4, 7)] + [f"time bucket {a}..{b}" for a, b in ((13, 26), (32, 64), (91, 100))]
               + ["5x40x257 f32", "3x33x32 complex half 0", "3x33x32 complex half 1", "lens all zero", "zero extent", "5x600x128 i32"])


@gpu
@pytest.mark.parametrize("name", SUITE_NAMES)
def test_records_equal_the_host_statement(name):
    got, want, again, p = _suite()[name]
    print(name, {k: (got[k], want[k]) for k in SUM_KEYS + EXACT})
    assert_record(got, want, name)
    if name in ("lens all zero", "zero extent", "clip 0 of 8x100x96"):
        assert got["n"] == 0 and all(not np.any(got[k]) for k in EXACT + SUM_KEYS + ("hist_abs", "hist_rel"))
    elif name.startswith("8x100x96 i32 device"):
        assert got["n"] == sum(LENS8) * 96 and got["n_nonfinite"] >= (32 + 65) * 96   # the clips with exponents 41 and -1
        assert 0 < got["n_equal"] < got["n"] - got["n_nonfinite"]                      # clip 4's exponent is the values' own
    elif name == "8x100x96 i32 exp15":
        assert got["n"] == sum(LENS8) * 96 and got["n_nonfinite"] < 96 and 0 < got["n_equal"] < got["n"]
    elif name.startswith("time bucket"):
        t0, t1 = (int(v) for v in name.split()[-1].split(".."))
        assert got["n"] == sum(min(max(v - t0, 0), t1 - t0) for v in LENS8) * 96 > 0
    elif name == "5x40x257 f32":
        assert got["n"] == (40 + 33 + 7 + 40) * 257 and got["n_nonfinite"] >= 3
    # two runs of the same call: identical bits
    for k in EXACT + SUM_KEYS + ("hist_abs", "hist_rel"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(again[k])), (name, k)


@gpu
def test_two_hundred_pairs_of_different_sizes_in_one_call():
    import torch
    from sparsernns_amd import verify

    rng = np.random.default_rng(81)
    pairs = []
    for i in range(200):
        shape = (int(rng.integers(1, 5)), int(rng.integers(1, 40)), int(rng.integers(1, 300)))
        kind = "f32" if i % 5 == 0 else "i32"
        a_exp = int(rng.integers(0, 41))
        lens = rng.integers(-2, shape[1] + 3, size=shape[0]).astype(np.int32)
        row0 = int(rng.integers(0, 4)) if i % 4 == 0 else 0
        a, b = poisoned(*make_values(shape, kind, a_exp, 200 + i), lens, row0)
        pairs.append(verify.clip_pair(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(lens).cuda(), a_exp,
                                      relu_a=bool(i % 3 == 0), row0=row0))
    got, want = verify.stage_errors_clips(pairs), verify.stage_errors_clips_host(pairs)
    assert len(got) == 200 and sum(w["n"] for w in want) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert_record(g, w, f"pair {i} {pairs[i].shape}")


# ----------------------------------------------------------------------------------------------------------------------
# MI355X: end to end
# ----------------------------------------------------------------------------------------------------------------------
E2E_LENS = (1, 33, 64, 97)
RECIPES = ("w8a16", "w8a8")


@functools.lru_cache(maxsize=None)
def _e2e(recipe):
    """compare_clips in its three modes and compare_engines on every clip alone, at dim_scale 0.5; shared, never modified."""
    import test_stage_err as ST
    from sparsernns_amd import verify

    md, qc, dims, eng, feng = ST._model(0.5, recipe)
    x = ST._x(dims, recipe, (len(E2E_LENS), max(E2E_LENS)))
    clips = [x[e, :L] for e, L in enumerate(E2E_LENS)]
    out = {by: verify.compare_clips(eng, feng, clips, qc, by=by) for by in ("stage", "clip", "time")}
    out["alone"] = [verify.compare_engines(eng, feng, c[None], qc, by="stage") for c in clips]
    return out, clips, (md, qc, dims, eng, feng)


@gpu
@pytest.mark.parametrize("recipe", RECIPES)
def test_by_clip_equals_compare_engines_on_the_clip_alone(recipe):
    out, clips, (md, qc, dims, eng, feng) = _e2e(recipe)
    rows = 2 + 10 * dims["n_layers"]
    assert len(out["clip"]) == rows * len(clips) and all(r["skipped"] == [] for r in out["clip"])
    for e in range(len(clips)):
        mine = [r for r in out["clip"] if r["clip"] == e]
        assert [r["name"] for r in mine] == [r["name"] for r in out["alone"][e]]
        for g, w in zip(mine, out["alone"][e]):
            print(recipe, e, g["name"], {k: (g[k], w[k]) for k in SUM_KEYS + EXACT})
            assert_record(g, w, (recipe, e, g["name"]))
        assert mine[0]["n"] == E2E_LENS[e] * dims["d_in"] and mine[-1]["n"] == E2E_LENS[e] * dims["d_out"]


@gpu
@pytest.mark.parametrize("recipe", RECIPES)
def test_by_stage_is_the_fold_of_by_clip_and_time_rows_equal_the_host_statement(recipe):
    from sparsernns_amd import verify

    out, clips, (md, qc, dims, eng, feng) = _e2e(recipe)
    names = [r["name"] for r in out["stage"]]
    assert names[0] == "inputs" and names[-1] == "decoder" and len(set(names)) == len(names) == 2 + 10 * dims["n_layers"]
    for by in ("clip", "time"):
        for s in out["stage"]:
            parts = [r for r in out[by] if r["name"] == s["name"]]
            n = s["n"]
            assert n == sum(E2E_LENS) * {"inputs": dims["d_in"], "decoder": dims["d_out"]}.get(
                s["name"], dims["P"] if ("Bu" in s["name"] or "xs" in s["name"]) else dims["H"])
            for k in ("n", "n_nonfinite", "n_equal", "n_ref_nonzero", "hist_abs", "hist_rel"):
                assert np.array_equal(sum(np.asarray(r[k]) for r in parts), np.asarray(s[k])), (by, s["name"], k)
            for k in ("max_abs", "max_rel"):
                assert max(r[k] for r in parts) == s[k], (by, s["name"], k)
            for k in SUM_KEYS:
                f = sum(r[k] for r in parts)
                assert abs(f - s[k]) <= 2 * n * EPS * abs(s[k]), (by, s["name"], k, f, s[k])
    # the time rows against the host statement of the same pairs
    x, lens = verify._padded_clips(feng, clips)
    rows, status = verify.clip_rows(eng, feng, x, lens, qc)
    pairs, keys = verify._split_clips(rows, lens, "time", 8)
    want = verify.stage_errors_clips_host(pairs)
    assert len(want) == len(out["time"]) and len(keys) == len(names) * len(range(0, 97, -(-97 // 8)))
    for k, g, w in zip(keys, out["time"], want):
        assert {kk: g[kk] for kk in k} == k
        assert_record(g, w, (recipe, k))


@gpu
def test_a_wide_input_clip_is_skipped_and_listed():
    import test_stage_err as ST
    import torch
    from sparsernns_amd import verify

    """compare_clips quantises its float input to the encoder's input width, which the 16-bit planes hold, so ST_WIDE_INPUT is
    planted one level down: an int32 launch with a value beyond 16 bits.  The masked lengths leave that clip's untouched
    (poisoned) trace rows out of every count."""
    from sparsernns_amd import _lib
    from sparsernns_amd.fxparray import RoundingMode, fxp_from_fp

    md, qc, dims, eng, feng = ST._model(0.5, "w8a16")
    x = torch.from_numpy(ST._x(dims, "w8a16", (3, 40))).cuda()
    fx = fxp_from_fp(x, bits=eng.inp_bits, exp=eng.inp_exp, signed=True, round_mode=RoundingMode.FLOOR, warn_on_clip=False)
    data = fx.data.contiguous().clone()
    data[1, 20, 5] = 40000
    lens = torch.tensor([40, 33, 7], dtype=torch.int32, device="cuda")
    planes = [{k: torch.full((3, 40, eng.P if k[:2] in ("Bu", "xs") else eng.H), POISON, dtype=torch.int32, device="cuda")
               for k in _lib.TRACE_FIELDS} for _ in range(eng.n_layers)]
    y, tr = eng.clips_traced(data, lens, x_bits=fx.bits, x_exp=fx.exp, traces=planes)
    status = eng.lane_status(0, 3)[:3 * _lib.STATUS_WORDS].view(3, _lib.STATUS_WORDS)
    masked = verify.lens_without_wide(status, lens)
    ft = feng.forward_clips_traced(x, lens)
    pairs = [verify.clip_pair(tr[0]["u"][e:e + 1], ft["l0.u"][e:e + 1], masked[e:e + 1], int(qc["blocks"].get("layers_0", qc["blocks"])["ssm"]["activations"]["u"]["exp"]))
             for e in range(3)]
    got = verify.stage_errors_clips(pairs)
    assert masked.cpu().tolist() == [40, 0, 7] and int(status[1, 0].item()) & _lib.ST_WIDE_INPUT
    assert [g["n"] for g in got] == [40 * eng.H, 0, 7 * eng.H] and got[0]["n_nonfinite"] == got[2]["n_nonfinite"] == 0
    assert bool((tr[0]["u"][1] == POISON).all())
    for g, w in zip(got, verify.stage_errors_clips_host(pairs)):
        assert_record(g, w, "masked lengths")


@gpu
@pytest.mark.parametrize("recipe", RECIPES)
def test_fake_quantised_float_side_agrees_on_at_least_as_much_of_Bu(recipe):
    """tests/test_stage_err.py::test_fake_quantised_float_side_agrees_on_more_of_Bu, ragged: the float side carries the integer
    model's weights, and with every site on its layer-0 Bu (real) equals the integer model's on no fewer elements."""
    import test_stage_err as ST
    from sparsernns_amd import floatmodel, verify

    _, clips, (md, qc, dims, eng, _) = _e2e(recipe)
    qeng = ST._quantised_weights_engine(0.5, recipe)
    plain = {r["name"]: r for r in verify.compare_clips(eng, qeng, clips, qc)}
    quant = {r["name"]: r for r in verify.compare_clips(eng, qeng, clips, qc, fq=floatmodel.fq_spec(qc, dims["n_layers"]))}
    name = "encoder.layers_0.mixer.Bu (real)"
    print(name, "n_equal with fq=None", plain[name]["n_equal"], "all sites", quant[name]["n_equal"], "of", quant[name]["n"])
    assert quant[name]["n"] == plain[name]["n"] == sum(E2E_LENS) * dims["P"]
    assert quant[name]["equal_share"] >= plain[name]["equal_share"], name


@gpu
def test_compare_float_clips_is_exact_upstream_of_the_one_site():
    from sparsernns_amd import floatmodel, verify

    _, clips, (md, qc, dims, eng, feng) = _e2e("w8a16")
    fq = floatmodel.fq_spec(qc, dims["n_layers"], ["l1.y"])
    rows = verify.compare_float_clips(feng, clips, fq)
    names = [r["name"] for r in rows]
    assert names[0] == "h_enc" and names[-1] == "out" and len(rows) == 2 + 9 * dims["n_layers"]
    cut = names.index("l1.y")
    for r in rows[:cut]:
        assert r["n_equal"] == r["n"] > 0 and r["sum_sq"] == 0.0 and r["n_nonfinite"] == 0, r["name"]
    assert rows[cut]["n_equal"] < rows[cut]["n"] and rows[cut]["sum_sq"] > 0.0 and rows[-1]["n_nonfinite"] == 0
    per = verify.compare_float_clips(feng, clips, fq, by="clip")
    for e, c in enumerate(clips):
        alone = verify.compare_float(feng, c[None], fq)
        for g, w in zip([r for r in per if r["clip"] == e], alone):
            assert g["name"] == w["name"]
            assert_record(g, w, ("compare_float_clips", e, g["name"]))
