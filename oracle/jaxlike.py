"""A strict NumPy stand-in for the slice of JAX that the reference's fixed-point files use  --  TEST INFRASTRUCTURE ONLY.

``oracle/refload.py`` installs the modules built here under the names ``jax``, ``jax.numpy``, ``jax.lax``, ``jax.nn``,
``jax.tree_util`` and ``jaxtyping`` and then executes the reference's ``fxparray.py`` / ``fxputils.py`` / ``fxpmodel.py``
in place.  That runs the reference's own PROGRAM LOGIC (which exponent, which order of shift / clip / wrap, which wiring);
it does not run XLA.  The arithmetic below is this file's definition of "JAX with jax_enable_x64 off", the same list
``DESIGN.md`` §2 calls "JAX semantics encoded", and it remains unverified against a real JAX:

  1. 32-bit throughout: the only dtypes are bool, int32, float32 and complex64; every 64-bit request or result (``int``,
     ``float``, ``np.int64`` ...) becomes its 32-bit kind.  A binary op promotes to the widest KIND among its operands
     (bool < int < float < complex), never to a wider size: int32 with float32 gives float32.
  2. Python scalars are weak: they take the dtype of the array they meet; a scalar of a wider kind than the array makes
     the result that kind's 32-bit dtype (bool array * 2 -> int32, int32 array * 1j -> complex64).
  3. Integer + - * negate << and matmul wrap modulo 2**32 and never raise; an out-of-range Python int wraps as well.
  4. ``>>`` on int32 is arithmetic.  A shift count outside [0, 31] is undefined in XLA and raises here.
  5. float -> int32 (``astype``) truncates toward zero, saturates at the int32 range and maps NaN to 0.
  6. int32 -> float32 rounds to nearest even; int32 -> complex64 goes through float32.
  7. ``round`` is half to even.
  8. ``maximum`` / ``minimum`` / ``relu`` on complex values are lexicographic (real part first, then imaginary).
  9. ``log2`` is the correctly rounded float32 function (float64 log2 rounded once); ``exp`` and ``sqrt`` are NumPy's
     float32 ones; ``lax.rsqrt`` is 1 / sqrt in float32; ``linspace`` is computed in float64 and rounded to float32.
 10. ``lax.scan`` and ``vmap`` are plain sequential loops (integer code: order cannot matter).

STRICT: a function, keyword, ufunc, dtype or ufunc method outside the explicit allow-lists below raises.  Nothing falls
through to NumPy, so a reference path that leaves the surface pinned here fails loudly instead of silently computing
something else.
"""
from __future__ import annotations

import types

import numpy as _np

_KINDS = {"b": 0, "i": 1, "f": 2, "c": 3}
_BY_KIND = [_np.dtype(_np.bool_), _np.dtype(_np.int32), _np.dtype(_np.float32), _np.dtype(_np.complex64)]


class JaxlikeError(NotImplementedError):
    """Raised for anything outside the allow-lists."""


def canonical_dtype(dtype) -> _np.dtype:
    """Rule 1: the 32-bit dtype of the requested kind."""
    if dtype is None:
        raise JaxlikeError("dtype=None is not part of the stand-in")
    dt = _np.dtype(dtype)
    if dt.kind == "b":
        return _BY_KIND[0]
    if dt in (_np.dtype(_np.int32), _np.dtype(_np.int64)):
        return _BY_KIND[1]
    if dt in (_np.dtype(_np.float32), _np.dtype(_np.float64)):
        return _BY_KIND[2]
    if dt in (_np.dtype(_np.complex64), _np.dtype(_np.complex128)):
        return _BY_KIND[3]
    raise JaxlikeError(f"dtype {dt} is outside the stand-in's allow-list (bool, int32, float32, complex64)")


def _f2i(x: _np.ndarray) -> _np.ndarray:
    """Rule 5."""
    with _np.errstate(all="ignore"):
        y = _np.trunc(x.astype(_np.float64))
        y = _np.where(_np.isnan(y), 0.0, _np.clip(y, -(2.0 ** 31), 2.0 ** 31 - 1))
        return y.astype(_np.int64).astype(_np.int32)


def _cast(raw: _np.ndarray, dt: _np.dtype) -> _np.ndarray:
    """Conversion of a canonical raw array between the four dtypes."""
    if raw.dtype == dt:
        return raw
    src, dst = raw.dtype.kind, dt.kind
    if src == "c" and dst != "c":
        raise JaxlikeError("complex -> real conversion is not part of the stand-in")
    if src == "f" and dst == "i":
        return _f2i(raw)
    if src == "i" and dst == "c":
        return raw.astype(_np.float32).astype(_np.complex64)
    with _np.errstate(all="ignore"):
        return raw.astype(dt)


def _canon(raw) -> _np.ndarray:
    """A NumPy array or scalar entering the stand-in: 64-bit becomes 32-bit (integers wrap)."""
    raw = _np.asarray(raw)
    dt = canonical_dtype(raw.dtype)
    if raw.dtype == dt:
        return raw
    with _np.errstate(all="ignore"):
        return raw.astype(dt)


def _wrap_int(v: int) -> _np.ndarray:
    """Rule 3 for a Python int."""
    return _np.array(int(v) & 0xFFFFFFFF, dtype=_np.uint32).astype(_np.int32)


def _is_pyscalar(x) -> bool:
    return isinstance(x, (bool, int, float, complex)) and not isinstance(x, _np.generic)


def _pykind(x) -> int:
    return 0 if isinstance(x, bool) else 1 if isinstance(x, int) else 2 if isinstance(x, float) else 3


def _raw(x) -> _np.ndarray:
    if isinstance(x, Array):
        return x.view(_np.ndarray)
    if isinstance(x, (_np.ndarray, _np.generic)):
        return _canon(x)
    if isinstance(x, (list, tuple)):
        return _promote(*x)[0] if not x else _np.stack(_promote(*x))
    raise JaxlikeError(f"operand of type {type(x).__name__} is not part of the stand-in")


def _promote(*xs, min_kind: int = 0):
    """Rules 1 and 2: all operands as raw arrays of one common dtype."""
    kinds = [_pykind(x) if _is_pyscalar(x) else _KINDS[_raw(x).dtype.kind] for x in xs]
    dt = _BY_KIND[max(max(kinds), min_kind)]
    out = []
    for x in xs:
        if _is_pyscalar(x):
            if dt.kind == "i":
                out.append(_wrap_int(x))
            else:
                out.append(_np.array(x, dtype=dt))
        else:
            out.append(_cast(_raw(x), dt))
    return out


def _wrap(raw) -> "Array":
    return _canon(raw).view(Array)


def _u(a: _np.ndarray) -> _np.ndarray:
    return a.view(_np.uint32)


def _lex_keep_first(a: _np.ndarray, b: _np.ndarray) -> _np.ndarray:
    """a > b in lexicographic order, for complex operands."""
    return (a.real > b.real) | ((a.real == b.real) & (a.imag > b.imag))


# ---------------------------------------------------------------------------------------------------------------------
# the operations, each on canonical raw arrays of one common dtype
# ---------------------------------------------------------------------------------------------------------------------
def _arith(name):
    uf = getattr(_np, name)

    def op(a, b):
        if a.dtype.kind == "i":  # rule 3
            return uf(_u(a), _u(b)).view(_np.int32)
        if a.dtype.kind == "b":
            raise JaxlikeError(f"{name} on two bool operands is not part of the stand-in")
        with _np.errstate(all="ignore"):
            return uf(a, b)
    return op


def _shift(name):
    def op(a, b):
        if a.dtype.kind != "i":
            raise JaxlikeError(f"{name} needs integer operands")
        if _np.any(b < 0) or _np.any(b > 31):
            raise ValueError(f"{name} by {b.tolist()}: a shift count outside [0, 31] is undefined in XLA")
        if name == "left_shift":
            return _np.left_shift(_u(a), _u(b)).view(_np.int32)
        return _np.right_shift(a, b)  # rule 4: arithmetic on a signed type
    return op


def _extreme(name):
    uf = getattr(_np, name)

    def op(a, b):
        if a.dtype.kind == "c":  # rule 8
            first = _lex_keep_first(a, b) if name == "maximum" else _lex_keep_first(b, a)
            return _np.where(first, a, b)
        return uf(a, b)
    return op


def _compare(name):
    uf = getattr(_np, name)

    def op(a, b):
        if a.dtype.kind == "c" and name not in ("equal", "not_equal"):
            raise JaxlikeError(f"{name} on complex operands is not part of the stand-in")
        return uf(a, b)
    return op


def _matmul(a, b):
    if a.dtype.kind == "i":  # rule 3: products and the accumulation wrap
        return _np.matmul(_u(a), _u(b)).view(_np.int32)
    if a.dtype.kind == "b":
        raise JaxlikeError("matmul on bool operands is not part of the stand-in")
    return _np.matmul(a, b)


def _true_divide(a, b):
    with _np.errstate(all="ignore"):
        return _np.true_divide(a, b)


def _bitwise_and(a, b):
    if a.dtype.kind not in "bi":
        raise JaxlikeError("bitwise_and needs integer operands")
    return _np.bitwise_and(a, b)


_BINARY = {
    "add": (_arith("add"), 0), "subtract": (_arith("subtract"), 0), "multiply": (_arith("multiply"), 0),
    "divide": (_true_divide, 2), "left_shift": (_shift("left_shift"), 0), "right_shift": (_shift("right_shift"), 0),
    "bitwise_and": (_bitwise_and, 0), "maximum": (_extreme("maximum"), 0), "minimum": (_extreme("minimum"), 0),
    "matmul": (_matmul, 0),
}
_BINARY.update({n: (_compare(n), 0) for n in ("greater", "less", "greater_equal", "less_equal", "equal", "not_equal")})


def _float_only(fn):
    def op(a):
        with _np.errstate(all="ignore"):
            return fn(a)
    return op, 2  # integer input is promoted to float32 first


def _refuse_complex(name):
    raise JaxlikeError(f"{name} of complex values is not part of the stand-in")


def _negative(a):
    if a.dtype.kind == "i":
        return _np.negative(_u(a)).view(_np.int32)
    if a.dtype.kind == "b":
        raise JaxlikeError("negative of bool is not part of the stand-in")
    return _np.negative(a)


def _absolute(a):
    if a.dtype.kind == "i":
        return _np.where(a < 0, _np.negative(_u(a)).view(_np.int32), a)  # |INT_MIN| wraps to INT_MIN
    if a.dtype.kind == "b":
        raise JaxlikeError("abs of bool is not part of the stand-in")
    return _np.absolute(a)


def _keep_ints(fn):
    """round / ceil / floor: integers pass through, floats use fn (float32 in, float32 out)."""
    def op(a):
        if a.dtype.kind in "bi":
            return _cast(a, _BY_KIND[2])
        if a.dtype.kind == "c":
            raise JaxlikeError("rounding of complex values is not part of the stand-in")
        return fn(a)
    return op, 0


_UNARY = {
    "negative": (_negative, 0), "absolute": (_absolute, 0),
    "rint": _keep_ints(_np.rint), "ceil": _keep_ints(_np.ceil), "floor": _keep_ints(_np.floor),   # rule 7: rint is half-to-even
    "exp": _float_only(_np.exp), "sqrt": _float_only(_np.sqrt),
    "log2": _float_only(lambda a: _np.log2(a.real.astype(_np.float64)).astype(_np.float32) if a.dtype.kind == "f" else _refuse_complex("log2")),  # rule 9
    "isnan": (_np.isnan, 2),
}


def _binary(name, a, b) -> "Array":
    fn, min_kind = _BINARY[name]
    ra, rb = _promote(a, b, min_kind=min_kind)
    return _wrap(fn(ra, rb))


def _unary(name, a) -> "Array":
    fn, min_kind = _UNARY[name]
    (ra,) = _promote(a, min_kind=min_kind)
    return _wrap(fn(ra))


# ---------------------------------------------------------------------------------------------------------------------
# the array type: the reference calls .astype / .max / .any / .item / .copy / .T / .real / .imag / indexing as methods
# ---------------------------------------------------------------------------------------------------------------------
class Array(_np.ndarray):
    __array_priority__ = 1000

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kwargs):
        name = ufunc.__name__
        if method != "__call__" or kwargs:
            raise JaxlikeError(f"ufunc {name}.{method}({', '.join(kwargs)}) is outside the stand-in's allow-list")
        if name in _BINARY and len(inputs) == 2:
            res = _binary(name, *inputs)
        elif name in _UNARY and len(inputs) == 1:
            res = _unary(name, *inputs)
        else:
            raise JaxlikeError(f"ufunc {name} is outside the stand-in's allow-list")
        if out is not None:  # in-place operators (x *= 2)
            (target,) = out
            if not isinstance(target, Array) or target.dtype != res.dtype or target.shape != res.shape:
                raise JaxlikeError(f"in-place {name} would change dtype or shape")
            target.view(_np.ndarray)[...] = res.view(_np.ndarray)
            return target
        return res

    def __array_function__(self, func, types_, args, kwargs):
        raise JaxlikeError(f"numpy.{func.__name__} was called on a stand-in array: only jax.numpy names are allowed")

    def astype(self, dtype, **kwargs):
        if kwargs:
            raise JaxlikeError(f"astype keywords {sorted(kwargs)} are outside the stand-in's allow-list")
        return _wrap(_cast(self.view(_np.ndarray), canonical_dtype(dtype)).copy())

    def max(self, **kwargs):
        return amax(self, **kwargs)

    def min(self, **kwargs):
        return amin(self, **kwargs)

    def any(self, **kwargs):
        return any_(self, **kwargs)

    def copy(self):
        return _wrap(self.view(_np.ndarray).copy())

    def _refuse(self, *a, **k):
        raise JaxlikeError("this array method is outside the stand-in's allow-list")

    sum = mean = prod = all = std = var = cumsum = cumprod = argmax = argmin = dot = round = clip = _refuse
    sort = argsort = tolist = tobytes = fill = put = resize = squeeze = ravel = flatten = repeat = take = _refuse


def to_numpy(x) -> _np.ndarray:
    """A plain ndarray copy of a stand-in array (for code outside the stand-in: recorders and tests)."""
    return _np.array(_raw(x))


# ---------------------------------------------------------------------------------------------------------------------
# jax.numpy
# ---------------------------------------------------------------------------------------------------------------------
def _only(kwargs, *names):
    extra = set(kwargs) - set(names)
    if extra:
        raise JaxlikeError(f"keyword(s) {sorted(extra)} are outside the stand-in's allow-list")


def amax(x, **kwargs):
    _only(kwargs)
    r = _raw(x)
    if r.dtype.kind == "c" or r.size == 0:
        raise JaxlikeError("max of a complex or empty array is not part of the stand-in")
    return _wrap(r.max())


def amin(x, **kwargs):
    _only(kwargs)
    r = _raw(x)
    if r.dtype.kind == "c" or r.size == 0:
        raise JaxlikeError("min of a complex or empty array is not part of the stand-in")
    return _wrap(r.min())


def any_(x, **kwargs):
    _only(kwargs)
    return _wrap(_np.any(_raw(x)))


def array(x, dtype=None, **kwargs):
    _only(kwargs)
    if _is_pyscalar(x):
        raw = _BY_KIND[_pykind(x)].type(x) if not isinstance(x, int) or isinstance(x, bool) else _wrap_int(x)
    else:
        raw = _raw(x)
    raw = _np.array(raw)
    return _wrap(raw if dtype is None else _cast(_canon(raw), canonical_dtype(dtype)))


def stack(arrays, axis=0, dtype=None, **kwargs):
    _only(kwargs)
    raw = _np.stack(_promote(*list(arrays)), axis=axis)
    return _wrap(raw if dtype is None else _cast(raw, canonical_dtype(dtype)))


def unstack(x, axis=0, **kwargs):
    _only(kwargs)
    r = _raw(x)
    return tuple(_wrap(_np.take(r, i, axis=axis)) for i in range(r.shape[axis]))


def ones(shape, dtype=_np.float32, **kwargs):
    _only(kwargs)
    return _wrap(_np.ones(shape, dtype=canonical_dtype(dtype)))


def zeros(shape, dtype=_np.float32, **kwargs):
    _only(kwargs)
    return _wrap(_np.zeros(shape, dtype=canonical_dtype(dtype)))


def linspace(start, stop, num, **kwargs):
    _only(kwargs)
    if not (_is_pyscalar(start) and _is_pyscalar(stop) and isinstance(num, int)):
        raise JaxlikeError("linspace takes Python scalars only")
    return _wrap(_np.linspace(start, stop, num, dtype=_np.float64).astype(_np.float32))  # rule 9


def where(cond, a, b, **kwargs):
    _only(kwargs)
    ra, rb = _promote(a, b)
    return _wrap(_np.where(_raw(cond).astype(bool), ra, rb))


def clip(x, a_min, a_max, **kwargs):
    _only(kwargs)
    return _binary("minimum", _binary("maximum", x, a_min), a_max)


def array_equal(a, b, **kwargs):
    _only(kwargs)
    ra, rb = _raw(a), _raw(b)
    return bool(ra.shape == rb.shape and _np.all(_promote(ra, rb)[0] == _promote(ra, rb)[1]))


def issubdtype(a, b):
    return _np.issubdtype(a, b)


def relu(x):
    return _binary("maximum", x, 0)


def rsqrt(x):
    return _binary("divide", 1.0, _unary("sqrt", x))  # rule 9


class _StrictModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__") and name.endswith("__"):  # the import machinery probes __path__, __spec__, ...
            raise AttributeError(name)
        raise JaxlikeError(f"{self.__name__}.{name} is outside the stand-in's allow-list")


def _module(name: str, **members) -> types.ModuleType:
    m = _StrictModule(name)
    m.__dict__.update(members)
    return m


def _un(name):
    return lambda x, **kw: (_only(kw), _unary(name, x))[1]


def _bin(name):
    return lambda a, b, **kw: (_only(kw), _binary(name, a, b))[1]


numpy = _module(
    "jax.numpy",
    ndarray=Array, int32=_np.int32, int64=_np.int64, float32=_np.float32, floating=_np.floating, bool_=_np.bool_,
    complex64=_np.complex64,
    array=array, asarray=array, stack=stack, unstack=unstack, ones=ones, zeros=zeros, linspace=linspace, where=where,
    clip=clip, array_equal=array_equal, issubdtype=issubdtype, max=amax, min=amin, any=any_,
    abs=_un("absolute"), round=_un("rint"), ceil=_un("ceil"), floor=_un("floor"), exp=_un("exp"), sqrt=_un("sqrt"),
    log2=_un("log2"), isnan=_un("isnan"),
    maximum=_bin("maximum"), minimum=_bin("minimum"), bitwise_and=_bin("bitwise_and"),
)


# ---------------------------------------------------------------------------------------------------------------------
# jax.lax.scan, jax.vmap, jax.tree_util  (rule 10)
# ---------------------------------------------------------------------------------------------------------------------
def _leaves(tree):
    return list(tree) if isinstance(tree, (tuple, list)) else [tree]


def _index(tree, i, axis=0):
    if isinstance(tree, (tuple, list)):
        return tuple(_index(t, i, axis) for t in tree)
    return _wrap(_np.take(_raw(tree), i, axis=axis))


def _stack_tree(items):
    if isinstance(items[0], (tuple, list)):
        return tuple(_stack_tree([it[j] for it in items]) for j in range(len(items[0])))
    return stack(items)


def scan(f, init, xs, **kwargs):
    _only(kwargs)
    n = {_raw(leaf).shape[0] for leaf in _leaves(xs)}
    if len(n) != 1:
        raise JaxlikeError(f"scan over leaves of different lengths {sorted(n)}")
    carry, ys = init, []
    for i in range(n.pop()):
        carry, y = f(carry, _index(xs, i))
        ys.append(y)
    if not ys:
        raise JaxlikeError("scan over an empty sequence is not part of the stand-in")
    return carry, _stack_tree(ys)


def vmap(f, in_axes=0, **kwargs):
    _only(kwargs)

    def mapped(*args):
        axes = tuple(in_axes) if isinstance(in_axes, (tuple, list)) else (in_axes,) * len(args)
        if len(axes) != len(args) or any(a not in (0, None) for a in axes):
            raise JaxlikeError(f"vmap in_axes={in_axes!r} for {len(args)} arguments is not part of the stand-in")
        n = {_raw(a).shape[0] for a, ax in zip(args, axes) if ax == 0}
        if len(n) != 1:
            raise JaxlikeError(f"vmap over mapped axes of different sizes {sorted(n)}")
        outs = [f(*[_index(a, i) if ax == 0 else a for a, ax in zip(args, axes)]) for i in range(n.pop())]
        return _stack_tree(outs)
    return mapped


class DictKey:
    """What tree_map_with_path hands over for a dict entry; str() is "['key']" as in JAX."""

    def __init__(self, key):
        self.key = key

    def __str__(self):
        return f"[{self.key!r}]"

    __repr__ = __str__


def tree_map_with_path(f, tree, *rest, **kwargs):
    _only(kwargs)
    if rest:
        raise JaxlikeError("tree_map_with_path over several trees is not part of the stand-in")

    def walk(node, path):
        if isinstance(node, dict):
            return type(node)((k, walk(v, path + (DictKey(k),))) for k, v in node.items())
        if isinstance(node, (list, tuple)):
            raise JaxlikeError("tree_map_with_path over sequences is not part of the stand-in")
        return f(path, node)
    return walk(tree, ())


def tree_wrap(tree):
    """A (nested dict) tree of NumPy leaves as stand-in arrays; other leaves (None, str, numbers) pass through."""
    if isinstance(tree, dict):
        return type(tree)((k, tree_wrap(v)) for k, v in tree.items())
    if isinstance(tree, (_np.ndarray, _np.generic)):
        return _wrap(_np.array(tree))
    return tree


lax = _module("jax.lax", scan=scan, rsqrt=rsqrt)
nn = _module("jax.nn", relu=relu)
tree_util = _module("jax.tree_util", tree_map_with_path=tree_map_with_path, DictKey=DictKey)
jax = _module("jax", numpy=numpy, lax=lax, nn=nn, tree_util=tree_util, vmap=vmap, Array=Array)
jaxtyping = _module("jaxtyping", Array=Array, DTypeLike=object, PyTree=object)

MODULES = {"jax": jax, "jax.numpy": numpy, "jax.lax": lax, "jax.nn": nn, "jax.tree_util": tree_util, "jaxtyping": jaxtyping}
