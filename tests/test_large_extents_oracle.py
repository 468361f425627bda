"""The property the large-extent suites (tests/large_extents.py) rest on, held on the CPU: the C oracle's output for a batch of
k copies of R sequences is k copies of its output for the R sequences, with the same bits and exponent.  Every tensor-wide
quantity of the integer model is an extreme; a batch-wide SUM anywhere in the oracle would break this, and with it the method.
"""
import numpy as np
import pytest

from oracle import cref
from oracle import fxp_oracle as O
from sparsernns_amd import synth


@pytest.mark.parametrize("cfg", [dict(dim_scale=0.5), dict(dim_scale=1.0, calib_L=128)], ids=["ds0.5", "ds1.0"])
def test_oracle_output_repeats_with_the_batch(cfg):
    from sparsernns_amd.fxpmodel import build_regression_model

    R, k, L = 7, 3, 131
    md, qc, dims = synth.make_model(**cfg)
    cm = cref.CModel(build_regression_model(md, qc, dims["n_layers"]).export())
    x = synth.make_input(R, L, dims["d_in"], seed=131)
    fx = O.from_fp(x, qc["encoder"]["inp_bits"], qc["encoder"]["inp_exp"], True, O.FLOOR)
    one, b1, e1, _ = cm.forward(fx.data, fx.bits, fx.exp)
    rep, bk, ek, _ = cm.forward(np.tile(fx.data, (k, 1, 1)), fx.bits, fx.exp)
    assert (bk, ek) == (b1, e1)
    assert int(np.abs(one).max()) > 0
    assert np.array_equal(rep.reshape((k,) + one.shape), np.broadcast_to(one, (k,) + one.shape))
