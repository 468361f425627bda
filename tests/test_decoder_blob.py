"""The fused decoder's packed arrays cover every column its kernels load.

proj_p.hpp k_dec_p (and its float / int16 twins) load the weight rows, cs128 and bias_eff of all 288 output columns they can
serve -- six waves x three 32-column tiles -- and mask only the stores, so s5fxp_fast.hpp pack_fast pads a narrower decoder
with zero rows.  Packed to ceil(d_out / 32) * 32 rows, a d_out = 1 decoder left those loads running 28 KB past its arrays, which
lie at the end of the model blob.  The blob's size shows the padding: between two models that differ only in d_out it may grow
by the generic path's decoder (weights K x M and bias M as int32, each rounded up to 256 bytes) and by nothing else.
"""
import copy

import numpy as np
import pytest


def _al256(n):
    return (n + 255) // 256 * 256


@pytest.mark.gpu
def test_fused_decoder_arrays_do_not_shrink_with_d_out():
    import contract_models as CM
    from sparsernns_amd import _lib
    from sparsernns_amd.engine import Engine

    ex1 = CM.case("F3_dims257x1_ds0.5").export()
    w, b = np.asarray(ex1["params"]["decoder"]["weight"]), np.asarray(ex1["params"]["decoder"]["bias"])
    assert w.shape[1] == 1 and b.shape == (1,)
    e1 = Engine(ex1)
    assert _lib.lib.s5fxp_model_is_fast(e1._h) == 1
    K = w.shape[0]
    for M in (33, 257):
        ex = dict(ex1, params=dict(ex1["params"], decoder=dict(copy.copy(ex1["params"]["decoder"]), weight=np.tile(w, (1, M)),
                                                              bias=np.tile(b, M))))
        e = Engine(ex)
        assert e.d_out == M and _lib.lib.s5fxp_model_is_fast(e._h) == 1
        generic = lambda m: _al256(4 * K * m) + _al256(4 * m)
        assert e.blob.numel() - e1.blob.numel() == generic(M) - generic(1), (M, e.blob.numel(), e1.blob.numel())
