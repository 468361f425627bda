"""Holds the CPU oracle's two halves and the host-side setup to what the REFERENCE's own integer code computes.

Three parts:
  * known answers for every arithmetic rule of the NumPy stand-in (oracle/jaxlike.py) -- no reference needed;
  * the LIVE differential, which runs the reference checkout under the stand-in: every committed ref_* fixture must
    regenerate byte for byte, and a seeded fuzz of the FxpArray ops must equal the oracle.  It skips only when there is no
    checkout (environment variable SPARSERNNS_REFERENCE, oracle/refload.py);
  * the FIXTURE checks, which read tests/golden/ref_* only and never skip: oracle/fxp_oracle.py, oracle/s5fxp_ref.c,
    sparsernns_amd.fxputils.derive and the integer export against what the reference wrote.
"""
import importlib.util
import os

import numpy as np
import pytest

from oracle import cref, jaxlike, refload
from oracle import fxp_oracle as O
from tests import reference_fixtures as RF

J = jaxlike.numpy
I32, F32, C64 = np.int32, np.float32, np.complex64


def _recorder():
    spec = importlib.util.spec_from_file_location("make_reference_golden", os.path.join(RF.GOLD, "make_reference_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _np(x):
    return jaxlike.to_numpy(x)


# ---------------------------------------------------------------------------------------------------------------------
# the stand-in, rule by rule (numbers as in the docstring of oracle/jaxlike.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_standin_is_strict():
    a = J.asarray(np.arange(4, dtype=I32))
    with pytest.raises(jaxlike.JaxlikeError):
        J.cumsum                                     # a function outside the allow-list
    with pytest.raises(jaxlike.JaxlikeError):
        J.stack([a, a], axis=0, out=None)            # a keyword outside it
    with pytest.raises(jaxlike.JaxlikeError):
        a.astype(np.int16)                           # a dtype outside it
    with pytest.raises(jaxlike.JaxlikeError):
        J.asarray(np.arange(4, dtype=np.uint8))
    with pytest.raises(jaxlike.JaxlikeError):
        a ** 2                                       # a ufunc outside it
    with pytest.raises(jaxlike.JaxlikeError):
        a.sum()                                      # a method outside it
    with pytest.raises(jaxlike.JaxlikeError):
        np.cumsum(a)                                 # NumPy itself on a stand-in array: no silent fall-through
    with pytest.raises(jaxlike.JaxlikeError):
        jaxlike.lax.associative_scan
    with pytest.raises(ValueError):
        a >> 32                                      # undefined in XLA
    with pytest.raises(ValueError):
        a << -1


def test_standin_is_32_bit_throughout():
    a = J.asarray(np.array([1, 2], dtype=np.int64))
    assert a.dtype == I32 and J.asarray(np.array([1.5])).dtype == F32 and J.asarray(np.array([1j])).dtype == C64
    assert a.astype(int).dtype == I32 and a.astype(np.int64).dtype == I32 and a.astype(float).dtype == F32
    assert J.zeros((2,), dtype=np.int64).dtype == I32 and J.ones((2,)).dtype == F32 and J.linspace(0, 8, 9).dtype == F32
    f = J.asarray(np.array([0.5, 2.0], dtype=F32))
    assert (a + f).dtype == F32 and (a * f).dtype == F32          # int32 with float32 stays 32 bits wide
    assert (a / a).dtype == F32 and _np(a / a).tolist() == [1.0, 1.0]
    assert J.log2(a).dtype == F32 and J.ceil(J.log2(a)).dtype == F32 and J.abs(a).max().dtype == I32
    assert J.stack([a, a], axis=-1).dtype == I32 and isinstance(a[0:1], jaxlike.Array)


def test_standin_python_scalars_are_weak():
    a, f = J.asarray(np.array([3, -4], dtype=I32)), J.asarray(np.array([0.5], dtype=F32))
    assert (a * 2).dtype == I32 and (a + 1.5).dtype == F32 and (f * 3).dtype == F32 and (f + 2.5).dtype == F32
    assert (1j * a).dtype == C64 and _np(a + 1j * a).tolist() == [3 + 3j, -4 - 4j]
    b = a > 0
    assert b.dtype == np.bool_ and (2 * b - 1).dtype == I32 and _np(2 * b - 1).tolist() == [1, -1]
    assert _np(f + 1e-8).tolist() == [0.5]                         # the eps is added in float32: 0.5 + 1e-8 == 0.5
    assert _np(J.asarray(np.array([1e-7], dtype=F32)) + 1e-8)[0] == F32(F32(1e-7) + F32(1e-8))


def test_standin_integer_arithmetic_wraps():
    big = J.asarray(np.array([2 ** 31 - 1, -(2 ** 31), 65536], dtype=I32))
    assert _np(big + 1).tolist() == [-(2 ** 31), -(2 ** 31) + 1, 65537]
    assert _np(big - 2).tolist() == [2 ** 31 - 3, 2 ** 31 - 2, 65534]
    assert _np(big * big).tolist() == [1, 0, 0]
    assert _np(big * 3).tolist() == [2 ** 31 - 3, -(2 ** 31), 196608]
    assert _np(-big).tolist() == [-(2 ** 31) + 1, -(2 ** 31), -65536] and _np(J.abs(big)).tolist() == [2 ** 31 - 1, -(2 ** 31), 65536]
    assert _np(big << 16).tolist() == [-65536, 0, 0]
    # NumPy raises OverflowError for an out-of-range Python int against int32; JAX wraps it
    assert _np(big + (1 << 31)).tolist() == [-1, 0, 65536 - 2 ** 31] and _np(big + ((1 << 32) + 5)).tolist()[2] == 65541
    assert _np(J.clip(big, -(1 << 15), (1 << 15) - 1)).tolist() == [32767, -32768, 32767]
    m = J.asarray(np.array([[2 ** 30, 2 ** 30, 3]], dtype=I32))
    assert _np(m @ J.asarray(np.array([[2], [2], [5]], dtype=I32))).tolist() == [[15]]          # 2**32 + 15
    w = J.asarray(np.array([7], dtype=I32))
    w *= 2 ** 31 - 1                                                                              # in place, as ys.data *= 2
    assert _np(w).tolist() == [2 ** 31 - 7] and w.dtype == I32


def test_standin_right_shift_is_arithmetic():
    a = J.asarray(np.array([-1, -5, 5, -(2 ** 31)], dtype=I32))
    assert _np(a >> 1).tolist() == [-1, -3, 2, -(2 ** 30)] and _np(a >> 31).tolist() == [-1, -1, 0, -1] and _np(a >> 0).tolist() == _np(a).tolist()
    assert _np(J.bitwise_and(a, 3)).tolist() == [3, 3, 1, 0]


def test_standin_float_to_int32_truncates_saturates_and_zeroes_nan():
    f = J.asarray(np.array([1.9, -1.9, -0.5, 0.5, 3e9, -3e9, np.inf, -np.inf, np.nan, 2147483520.0, -0.0], dtype=F32))
    want = [1, -1, 0, 0, 2 ** 31 - 1, -(2 ** 31), 2 ** 31 - 1, -(2 ** 31), 0, 2147483520, 0]
    assert _np(f.astype(np.int32)).tolist() == want and _np(f.astype(int)).tolist() == want
    c = (J.asarray(np.array([2 ** 24 + 1, -7], dtype=I32)) * 1j).imag            # int32 -> complex64 goes through float32
    assert _np(c.astype(np.int32)).tolist() == [2 ** 24, -7]
    assert _np(J.asarray(np.array([2 ** 24 + 1, 2 ** 24 + 3], dtype=I32)).astype(np.float32)).tolist() == [2.0 ** 24, 2.0 ** 24 + 4]


def test_standin_round_is_half_to_even():
    f = J.asarray(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.4999, 1e9], dtype=F32))
    assert _np(J.round(f)).tolist() == [0.0, 2.0, 2.0, -0.0, -2.0, -2.0, 2.0, 1e9]
    assert _np(J.ceil(f))[:4].tolist() == [1.0, 2.0, 3.0, -0.0] and _np(J.floor(f))[:4].tolist() == [0.0, 1.0, 2.0, -1.0]


def test_standin_complex_maximum_is_lexicographic():
    z = J.asarray(np.array([5 - 9j, 0 + 4j, 0 + 0j, 0 - 4j, -3 + 8j, 1e-3 - 1e6j], dtype=C64))
    want = [5 - 9j, 4j, 0, 0, 0, C64(1e-3 - 1e6j)]
    assert _np(jaxlike.nn.relu(z)).tolist() == want and _np(J.maximum(z, 0)).tolist() == want
    assert _np(J.minimum(z, 0)).tolist() == [0, 0, 0, -4j, -3 + 8j, 0]
    r = J.asarray(np.array([-2, 0, 7], dtype=I32))
    assert _np(jaxlike.nn.relu(r)).tolist() == [0, 0, 7] and _np(J.maximum(r, 0)).dtype == I32


def test_standin_log2_and_friends():
    v = J.asarray(np.array([8.0, 8.000001, 0.25, 3.0], dtype=F32))
    assert _np(J.ceil(J.log2(v))).tolist() == [3.0, 4.0, -2.0, 2.0]
    assert _np(J.log2(v))[3] == F32(np.log2(3.0))                   # float64 log2, rounded once
    assert _np(jaxlike.lax.rsqrt(J.asarray(np.array([4.0, 2.0], dtype=F32)))).tolist() == [0.5, float(F32(1) / np.sqrt(F32(2)))]
    assert _np(J.where(J.isnan(J.asarray(np.array([np.nan, 2.0], dtype=F32))), 1.0, v[:2])).tolist() == [1.0, float(F32(8.000001))]
    assert _np(J.linspace(0, 512, 9)[:-1].astype(int)).tolist() == list(range(0, 512, 64))
    a, b = J.unstack(J.asarray(np.arange(6, dtype=I32).reshape(3, 2)), axis=-1)
    assert _np(a).tolist() == [0, 2, 4] and _np(b).tolist() == [1, 3, 5]


def test_standin_scan_and_vmap_are_sequential_loops():
    def step(c, xs):
        a, b = xs
        n = c * a + b
        return n, n

    xs = (J.asarray(np.array([2, 3, 4], dtype=I32)), J.asarray(np.array([1, 1, 1], dtype=I32)))
    last, ys = jaxlike.lax.scan(step, J.asarray(np.array(1, dtype=I32)), xs)
    assert _np(ys).tolist() == [3, 10, 41] and int(last) == 41
    # in_axes as the recurrence uses them: mapped arrays, shared arrays (None) and plain Python numbers (None)
    f = lambda x, w, k: x * w + k
    got = jaxlike.vmap(f, in_axes=(0, None, None))(J.asarray(np.arange(6, dtype=I32).reshape(2, 3)), J.asarray(np.array([1, 10, 100], dtype=I32)), 7)
    assert _np(got).tolist() == [[7, 17, 207], [10, 47, 507]]
    with pytest.raises(jaxlike.JaxlikeError):
        jaxlike.vmap(f, in_axes=(1, None, None))(J.zeros((2, 3), dtype=np.int32), J.zeros((3,), dtype=np.int32), 7)
    tree = jaxlike.tree_util.tree_map_with_path(lambda p, x: str(p[-1]), dict(a=dict(act_scale=1, kernel=2)))
    assert tree == dict(a=dict(act_scale="['act_scale']", kernel="['kernel']"))


# ---------------------------------------------------------------------------------------------------------------------
# live differential: needs the reference checkout
# ---------------------------------------------------------------------------------------------------------------------
needs_reference = pytest.mark.skipif(not refload.available(), reason=f"no reference checkout at {refload.reference_path()!r}")


@pytest.fixture(scope="module")
def ref():
    import sys
    before = set(sys.modules)
    r = refload.load()
    assert not {m for m in set(sys.modules) - before if m.split(".")[0] in ("jax", "jaxtyping", "sparseRNNs")}   # sys.modules restored
    return r


@needs_reference
def test_live_every_fixture_regenerates_byte_for_byte(ref):
    """The committed ref_* files are what the reference writes today: same json text, same npz members with the same bytes
    (the zip container itself carries timestamps and a zlib's choices, which are not content).  No file beyond them."""
    rec = _recorder()
    made = rec.generate(ref)
    on_disk = sorted(f[:-4] for f in os.listdir(RF.GOLD) if f.startswith("ref_") and f.endswith(".npz"))
    assert on_disk == sorted(made), (on_disk, sorted(made))
    n_members = 0
    for name, (arrays, meta) in made.items():
        with open(os.path.join(RF.GOLD, name + ".json"), "rb") as f:
            assert f.read() == rec.json_text(meta).encode(), f"{name}.json is not what the reference writes"
        want, have = rec.member_bytes(arrays), rec.file_member_bytes(os.path.join(RF.GOLD, name + ".npz"))
        assert sorted(want) == sorted(have), f"{name}.npz members differ"
        for k in want:
            assert want[k] == have[k], f"{name}.npz member {k} is not what the reference writes"
        n_members += len(want)
    print(f"\n[reference pin] regenerated {len(made)} fixtures, {n_members} npz members, byte for byte")


@needs_reference
@pytest.mark.parametrize("n", [600], ids=["600_cases_generated_0_filtered"])
def test_live_seeded_op_fuzz_equals_the_oracle(ref, n):
    """Random add / sub / mul / change_exp / change_cfg / matmul / from_fp configurations, fixed and compute_best, in all
    three rounding modes, generated inside each op's contract: the reference and the oracle must agree on every one."""
    rec = _recorder()
    rng = np.random.default_rng(777)
    seen = {}
    for i in range(n):
        cfg, ins = rec.random_arith_case(rng)
        want, want_cfg = rec.run_reference(ref, cfg, ins)
        got, got_cfg = RF.run_oracle(cfg, ins)
        RF.assert_case_equal(f"fuzz {i} {cfg}", got, got_cfg, want, want_cfg)
        key = (cfg["op"], cfg["mode"], cfg.get("result_exp") == "compute_best")
        seen[key] = seen.get(key, 0) + 1
    for op in ("add", "sub", "mul", "change_exp", "change_cfg", "matmul", "from_fp"):
        for mode in rec.MODES:
            assert seen.get((op, mode, False), 0) > 0, (op, mode)
    assert all(seen.get((op, "FLOOR", True), 0) > 0 for op in ("add", "sub", "mul"))
    print(f"\n[reference pin] op fuzz: {n} cases generated, 0 filtered, {n} equal to the oracle")


@needs_reference
def test_live_reference_leaves_the_standin_loudly(ref):
    """A reference path outside what the stand-in pins fails instead of computing something: the undefined negative shift
    of fxp_matmul (the oracle and the build raise there as well)."""
    R = ref.fxparray
    a = R.FxpArray(J.asarray(np.ones((2, 3), dtype=I32)), 16, 2)
    w = R.FxpArray(J.asarray(np.ones((3, 2), dtype=I32)), 16, 2)
    with pytest.raises(ValueError):
        R.fxp_matmul(a, w, result_bits=16, result_exp=9)
    with pytest.raises(ValueError):
        O.matmul(O.Fx(np.ones((2, 3), I32), 16, 2), O.Fx(np.ones((3, 2), I32), 16, 2), 16, 9)


# ---------------------------------------------------------------------------------------------------------------------
# fixture checks: read tests/golden/ref_* only, never skip
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_ops_numpy_oracle():
    cases = RF.op_cases()
    ops = {c[1]["op"] for c in cases}
    assert ops == {"from_fp", "to_float", "change_exp", "change_cfg", "add", "sub", "mul", "matmul", "complex_add", "complex_mul",
                   "clip", "relu", "relu_complex", "sigmoid", "scan"}
    for i, cfg, ins, want in cases:
        got, got_cfg = RF.run_oracle(cfg, ins)
        RF.assert_case_equal(f"ref_ops case {i} {cfg}", got, got_cfg, want, cfg["out_cfg"])


def test_fixture_ops_cover_the_quirks():
    """The recorded table really holds the edges the issue names (so a regenerated table cannot quietly lose them)."""
    cases = RF.op_cases()
    by = lambda op: [c for c in cases if c[1]["op"] == op]
    # a left shift that saturates at the OLD width although the value fits int32, in change_exp and inside change_cfg
    for op in ("change_exp", "change_cfg"):
        hit = 0
        for _, cfg, ins, out in by(op):
            bits, exp = cfg["a_cfg"]
            if cfg["new_exp"] > exp and cfg.get("new_bits", bits) >= bits:
                shifted = ins["a"].astype(np.int64) << (cfg["new_exp"] - exp)
                hit += int(np.any((np.abs(shifted) < 2 ** 31) & (shifted > (1 << (bits - 1)) - 1) & (out["out"] == (1 << (bits - 1)) - 1)))
        assert hit > 0, op
    assert {c[1]["mode"] for c in by("change_exp")} == {c[1]["mode"] for c in by("from_fp")} == {"FLOOR", "CEIL", "ROUND"}
    x = by("from_fp")[0][2]["x"]
    assert np.isnan(x).any() and np.signbit(x[x == 0]).any() and (np.abs(x) > 2.0 ** 31).any()
    assert any(np.abs(c[2]["a"].astype(np.int64) @ c[2]["b"].astype(np.int64)).max() >= 2 ** 31 for c in by("matmul"))     # wraps
    assert any(np.abs(c[3]["out_re"]).max() > 2 ** 30 for c in by("scan")) and any(c[1]["batched"] for c in by("scan"))
    assert sorted(len(c[2]["a"]) for c in by("sigmoid")) == [256, 65536, 65536, 65536]
    best = [c for c in by("add") + by("mul") if c[1]["result_exp"] == "compute_best"]
    assert len({c[1]["out_cfg"][0][1] for c in best}) >= 6 and any(c[2]["a"].shape != c[2]["b"].shape for c in best)


def _oracle_intermediates(name):
    meta, export, x, y, inter, md = RF.load_model_fixture(name)
    n_layers = meta["dims"]["n_layers"]
    model = RF.oracle_from_export(export)
    it = {}
    yo = model(O.Fx(x, meta["x_bits"], meta["x_exp"]), it)
    return meta, export, x, y, inter, md, n_layers, yo, O.flatten_intermediates(it)


@pytest.mark.parametrize("name", RF.MODEL_FIXTURES)
def test_fixture_model_numpy_oracle(name):
    """Output, every recorded intermediate by name, and the (bits, exp) of EVERY intermediate (the json keeps those for the
    tensors whose arrays a wide fixture drops): all the compute_best exponents of the run."""
    meta, export, x, y, inter, md, n_layers, yo, fl = _oracle_intermediates(name)
    assert (yo.bits, yo.exp) == (meta["y_bits"], meta["y_exp"]) and np.array_equal(yo.data, y)
    # the name map is total in both directions
    mapped = {k: RF.oracle_name(k, n_layers) for k in meta["inter"]}
    layer_only = {f"layers_{i}.{k}" for i in range(n_layers) for k in RF.ORACLE_ONLY}
    assert set(mapped.values()) | layer_only == set(fl), sorted(set(fl) ^ (set(mapped.values()) | layer_only))
    assert not set(mapped.values()) & layer_only
    assert set(inter) <= set(meta["inter"]) and len(inter) >= 6
    for k, (bits, exp) in meta["inter"].items():
        assert (fl[mapped[k]].bits, fl[mapped[k]].exp) == (bits, exp), (k, mapped[k])
    for k, v in inter.items():
        assert np.array_equal(fl[mapped[k]].data, v), f"{k} -> {mapped[k]}: {np.count_nonzero(fl[mapped[k]].data != v)} values differ"
    if x.shape[0] > 1:   # the compute_best scope is the whole batch: alone, a sequence chooses its own exponents somewhere
        alone = RF.oracle_from_export(export)
        its = [{} for _ in range(x.shape[0])]
        for b in range(x.shape[0]):
            alone(O.Fx(x[b:b + 1], meta["x_bits"], meta["x_exp"]), its[b])
        exps = [{k: v.exp for k, v in O.flatten_intermediates(i).items()} for i in its]
        batch = {k: v.exp for k, v in fl.items()}
        assert any(e != batch for e in exps), "the fixture cannot tell a per-sequence scope from a per-batch one"


@pytest.mark.parametrize("name", RF.MODEL_FIXTURES)
def test_fixture_model_c_oracle(name):
    meta, export, x, y, inter, md = RF.load_model_fixture(name)
    yc, yb, ye, tr = cref.CModel(export).forward(x, meta["x_bits"], meta["x_exp"], trace=True)
    assert (yb, ye) == (meta["y_bits"], meta["y_exp"]) and np.array_equal(yc, y)
    checked = 0
    for i, t in enumerate(tr):
        for ck, rk in RF.CREF_TRACE.items():
            key = f"encoder.layers_{i}.{rk}"
            if key in inter:
                assert np.array_equal(t[ck], inter[key]), key
                checked += 1
        assert t["pre_s5_exp"] == meta["inter"][f"encoder.layers_{i}.pre_s5"][1]
        assert t["residadd_exp"] == meta["inter"][f"encoder.layers_{i}.residadd"][1]
    assert checked >= 2


@pytest.mark.parametrize("name", [n for n in RF.MODEL_FIXTURES if RF.load_model_fixture(n)[5] is not None])
def test_fixture_integer_export_from_float_parameters(name):
    """float parameters + fxp_qconfig -> integers: the oracle's setup and the product's host-side setup against the
    reference's export(), params and qconfig."""
    from sparsernns_amd.fxpmodel import build_regression_model

    meta, export, x, y, inter, md = RF.load_model_fixture(name)
    n_layers = meta["dims"]["n_layers"]
    for who, ex in (("oracle", O.RegressionModel(md, meta["qconfig"], n_layers).export()),
                    ("product", build_regression_model(md, meta["qconfig"], n_layers).export())):
        RF.tree_assert_equal(ex["params"], export["params"], f"{name} {who} params")
        signed_free = lambda t: {k: (signed_free(v) if isinstance(v, dict) else v) for k, v in t.items() if not k.endswith("_signed")}
        RF.tree_assert_equal(signed_free(ex["qconfig"]), signed_free(export["qconfig"]), f"{name} {who} qconfig")


def test_fixture_qconfig_derivation():
    """sparsernns_amd.fxputils.derive on the recorded calibration trees against what the reference's load_modeldict /
    create_fxp_qconfig / add_target_bits_exp made of them, key for key."""
    from sparsernns_amd import fxputils

    arrays, meta = RF.load_packed("ref_qconfig")
    assert set(meta["cases"]) == {"shared", "shared_bnscale", "separate_bnscale"}
    for name, c in meta["cases"].items():
        tree = RF.unflatten({k[len(name) + 1:]: v for k, v in arrays.items() if k.startswith(name + "/")})
        _, qc = fxputils.derive(tree["params"], tree["stats"], "w8a16", separate_exponents=c["separate_exponents"])
        plain = lambda t: {k: plain(v) for k, v in t.items()} if isinstance(t, dict) else (np.asarray(t).tolist())
        RF.tree_assert_equal(plain(qc), c["fxp_qconfig"], f"ref_qconfig {name}")
