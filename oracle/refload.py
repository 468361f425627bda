"""Runs the reference's own fixed-point files under the NumPy stand-in  --  TEST INFRASTRUCTURE ONLY.

``load()`` executes ``sparseRNNs/fxparray.py``, ``fxputils.py`` and ``fxpmodel.py`` IN PLACE from a reference checkout
(nothing is copied, nothing is written there) with ``oracle/jaxlike.py`` installed as ``jax`` / ``jaxtyping`` and three
stub modules in the place of the imports those files cannot satisfy here:

  * ``sparseRNNs.utils.logging.logger``            a silent ``logging.Logger``;
  * ``sparseRNNs.utils.quantization.QuantizationConfig``   only ``.none()`` (a default argument) and ``.to_dict()``;
  * ``sparseRNNs.model.seq_model.masked_meanpool``  raises (the regression model never pools);
  * ``sparseRNNs.model.ssm.discretize_zoh``        the float32 / complex64 ZOH formula.  The flax ``ssm.py`` is the FLOAT
    model and stays unpinned: the stub is ``oracle.fxp_oracle.discretize_zoh``, so both sides quantise the same floats
    and the comparison isolates the integer code.

``sys.modules`` is restored before ``load()`` returns.  The checkout is found through the environment variable
``SPARSERNNS_REFERENCE`` (default ``/root/reference``).  Only ``tests/test_reference_pin.py`` (its live part) and
``tests/golden/make_reference_golden.py`` use this file; no GPU test, ``smoke()`` or ``bench.py`` may.
"""
from __future__ import annotations

import importlib.util
import logging
import os
import sys
import types

from . import jaxlike

ENV = "SPARSERNNS_REFERENCE"
DEFAULT = "/root/reference"
FILES = ("fxparray", "fxputils", "fxpmodel")


def reference_path() -> str:
    return os.environ.get(ENV, DEFAULT)


def available(path: str = None) -> bool:
    path = path or reference_path()
    return all(os.path.isfile(os.path.join(path, "sparseRNNs", f + ".py")) for f in FILES)


class QuantizationConfig:
    @classmethod
    def none(cls):
        return cls()

    def to_dict(self):
        return {}


def _masked_meanpool(*args, **kwargs):
    raise jaxlike.JaxlikeError("masked_meanpool is not part of the stand-in")


def _discretize_bilinear(*args, **kwargs):
    raise jaxlike.JaxlikeError("discretize_bilinear is not part of the stand-in")


def _discretize_zoh(Lambda, B_tilde, Delta):
    from .fxp_oracle import discretize_zoh
    lam, b = discretize_zoh(jaxlike.to_numpy(Lambda), jaxlike.to_numpy(B_tilde), jaxlike.to_numpy(Delta))
    return jaxlike.numpy.asarray(lam), jaxlike.numpy.asarray(b)


def _stubs() -> dict:
    def mod(name, pkg=False, **members):
        m = types.ModuleType(name)
        if pkg:
            m.__path__ = []
        m.__dict__.update(members)
        return m

    logger = logging.getLogger("sparseRNNs.reference")
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    logger.setLevel(logging.CRITICAL + 1)
    return {
        "sparseRNNs": mod("sparseRNNs", pkg=True),
        "sparseRNNs.utils": mod("sparseRNNs.utils", pkg=True),
        "sparseRNNs.utils.logging": mod("sparseRNNs.utils.logging", logger=logger),
        "sparseRNNs.utils.quantization": mod("sparseRNNs.utils.quantization", QuantizationConfig=QuantizationConfig),
        "sparseRNNs.model": mod("sparseRNNs.model", pkg=True),
        "sparseRNNs.model.seq_model": mod("sparseRNNs.model.seq_model", masked_meanpool=_masked_meanpool),
        "sparseRNNs.model.ssm": mod("sparseRNNs.model.ssm", discretize_zoh=_discretize_zoh,
                                    discretize_bilinear=_discretize_bilinear),
    }


def load(path: str = None) -> types.SimpleNamespace:
    """Returns a namespace with ``fxparray``, ``fxputils``, ``fxpmodel`` (the executed reference modules),
    ``QuantizationConfig`` (the stub) and ``path``."""
    path = path or reference_path()
    if not available(path):
        raise FileNotFoundError(f"no reference checkout at {path!r} (set {ENV})")
    installed = dict(jaxlike.MODULES)
    installed.update(_stubs())
    names = list(installed) + [f"sparseRNNs.{f}" for f in FILES]
    saved = {n: sys.modules.get(n) for n in names}
    out = types.SimpleNamespace(path=path, QuantizationConfig=QuantizationConfig)
    try:
        sys.modules.update(installed)
        for f in FILES:
            name = f"sparseRNNs.{f}"
            spec = importlib.util.spec_from_file_location(name, os.path.join(path, "sparseRNNs", f + ".py"))
            m = importlib.util.module_from_spec(spec)
            sys.modules[name] = m
            sys.dont_write_bytecode, keep = True, sys.dont_write_bytecode   # the checkout is read-only to us
            try:
                spec.loader.exec_module(m)
            finally:
                sys.dont_write_bytecode = keep
            setattr(out, f, m)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    out.fxparray.print_call_stack = lambda: None   # a clip warning prints the call stack; the logger is silent, so is this
    return out


def build_model(ref, modeldict: dict, fxp_qconfig: dict, dims: dict, store_intermediates: bool = True):
    """The reference's ``FxpRegressionModel`` in the one configuration this project implements (fxprun's N-DNS recipe:
    prenorm BatchNorm, GLU "half1", relufication, ZOH, conj_sym, lax.scan recurrence, BatchNorm not fused)."""
    M, q = ref.fxpmodel, ref.QuantizationConfig.none()
    mixer_cls = M.FxpSSM.init_fn(H=dims["H"], P=dims["P"], discretization="zoh", conj_sym=True, q_config=q,
                                 bidirectional=False, relufication=True, associative_scan=False)
    return M.FxpRegressionModel(
        modeldict=jaxlike.tree_wrap(modeldict), fxp_qconfig=fxp_qconfig, scope="model",
        store_intermediates=store_intermediates, mixer_cls=mixer_cls, n_layers=dims["n_layers"], d_model=dims["H"],
        batchnorm=True, prenorm=True, bn_momentum=0.95, glu_variant="half1", step_rescale=1.0, relufication=True,
        fuse_batchnorm_linear=False, q_config=q, dropout=0.0, training=False, d_output=dims["d_out"], padded=False)
