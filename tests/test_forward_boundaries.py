"""What the int32, float32 and int16 forward entries (include/s5fxp.h s5fxp_model_forward, _f32, _i16) share on the host:
the per-group loop a grouped call on a fused model falls to when its groups cannot share one set of launches, and the order of
the checks every entry makes before its first launch: bad arguments, then unsupported, then the workspace, then the stream
extent.
"""
import numpy as np
import pytest

from sparsernns_amd import synth

pytestmark = pytest.mark.gpu

SCAN_DEPTH = 32   # s5fxp_api.hip: the time blocks the recurrence kernels keep in flight (S5_SCANP_ASM_DEPTH)
SENT = {"int32": -7, "float32": -7.0, "int16": -21846}
_CACHE = {}


def _export():
    if "export" not in _CACHE:
        from sparsernns_amd.fxpmodel import build_regression_model
        md, qc, dims = synth.make_model(0.5, calib_L=128)
        _CACHE["export"] = build_regression_model(md, qc, dims["n_layers"]).export()
    return _CACHE["export"]


def _engine(monkeypatch, no_bn_ext):
    """The dim_scale 0.5 model on the fused path; no_bn_ext: created under S5FXP_NO_BN_EXT (read once, at creation), so that
    fast_bn_ext(m) is false and a grouped call cannot take the one set of fused launches."""
    from sparsernns_amd.engine import Engine
    if no_bn_ext not in _CACHE:
        if no_bn_ext:
            monkeypatch.setenv("S5FXP_NO_BN_EXT", "1")
        try:
            _CACHE[no_bn_ext] = Engine(_export())
        finally:
            if no_bn_ext:
                monkeypatch.delenv("S5FXP_NO_BN_EXT")
    return _CACHE[no_bn_ext]


def _inputs(eng, G, B, L, seed):
    """The same rows for the three boundaries: float32, and their integers at the encoder's input configuration."""
    import torch
    from oracle import fxp_oracle as O
    xf = synth.make_input(G * B, L, eng.d_in, seed=seed).astype(np.float32)
    xi = O.from_fp(xf, eng.inp_bits, eng.inp_exp, True, O.FLOOR).data.astype(np.int32)
    assert eng.inp_bits <= 16
    return {torch.float32: xf, torch.int32: xi, torch.int16: xi.astype(np.int16)}


def _buffers(dtype, xs, ny):
    """x one element into its buffer (an int16 tensor is then 2-byte aligned only) and y between 64 sentinels either side."""
    import torch
    name = str(dtype).split(".")[1]
    xbuf = torch.zeros(xs.size + 2, dtype=dtype, device="cuda")
    x = xbuf[1:1 + xs.size]
    x.copy_(torch.from_numpy(xs.reshape(-1)))
    ybuf = torch.full((1 + 64 + ny + 64,), SENT[name], dtype=dtype, device="cuda")
    return x, ybuf, ybuf[65:65 + ny]


@pytest.mark.parametrize("io", ["int32", "float32", "int16"])
def test_grouped_call_on_the_per_group_loop_of_a_fused_model(io, monkeypatch):
    """groups = 3, B = 1, L = 5 at d_in = 257: 1285 elements per group, so the group bases are odd in dwords and, for int16,
    2-byte aligned only.  Without the BatchNorm-extremes method the entry runs the groups one by one; y, every status word and
    the carry out must be those of three single calls on the slices."""
    import torch
    from sparsernns_amd import _lib

    eng = _engine(monkeypatch, True)
    assert _lib.lib.s5fxp_model_is_fast(eng._h) == 1 and eng.d_in == 257
    dtype = getattr(torch, io)
    G, B, L, W = 3, 1, 5, _lib.STATUS_WORDS
    shape = (eng.n_layers, 2, B, eng.P)
    # a carry to start from: the one three chunks of other rows leave
    warm = _inputs(eng, G, B, 9, seed=21)[torch.int32]
    state_in = torch.full((G,) + shape, -3, dtype=torch.int32, device="cuda")
    eng.enqueue(torch.from_numpy(warm).cuda(), eng.inp_bits, eng.inp_exp, torch.empty((G * B, 9, eng.d_out), dtype=torch.int32,
                device="cuda"), B, 9, state_out=state_in, groups=G)
    torch.cuda.synchronize()
    assert int(state_in.abs().max()) > 0

    xs = _inputs(eng, G, B, L, seed=22)[dtype]
    nx, ny = B * L * eng.d_in, B * L * eng.d_out
    assert nx % 2 == 1

    def run(groups, x, y, sin):
        so = torch.full((groups,) + shape if groups > 1 else shape, -3, dtype=torch.int32, device="cuda")
        eng.lane_status(0, groups).fill_(-9)
        eng.enqueue(x, eng.inp_bits, eng.inp_exp, y, B, L, state_in=sin, state_out=so, groups=groups)
        torch.cuda.synchronize()
        return eng.lane_status(0, groups).cpu().numpy()[:groups * W].copy(), so.cpu().numpy()

    x, ybuf, y = _buffers(dtype, xs, G * ny)
    if io == "int16":
        assert x.data_ptr() % 4 == 2 and y.data_ptr() % 4 == 2
    st, so = run(G, x.view(G * B, L, eng.d_in), y.view(G * B, L, eng.d_out), state_in)
    guard = torch.cat([ybuf[:65], ybuf[65 + G * ny:]])
    assert bool((guard == SENT[io]).all()), "sentinels around y were overwritten"
    got = y.cpu().numpy().copy()
    assert all(st[g * W + 2] == _lib.PATH_FUSED for g in range(G)), st[2::W]

    for g in range(G):
        x1, ybuf1, y1 = _buffers(dtype, xs[g * B:(g + 1) * B], ny)
        st1, so1 = run(1, x1.view(B, L, eng.d_in), y1.view(B, L, eng.d_out), state_in[g])
        assert st1[2] == _lib.PATH_FUSED
        one = y1.cpu().numpy()
        # bit for bit: float32 outputs are compared as their bits
        assert np.array_equal(got[g * ny:(g + 1) * ny].view(np.uint8), one.view(np.uint8)), (io, g)
        assert np.array_equal(st[g * W:(g + 1) * W], st1), (io, g, np.nonzero(st[g * W:(g + 1) * W] != st1))
        assert np.array_equal(so[g], so1), (io, g)


def _smallest_bad_extent_L(P):
    """The smallest L at which stream_extent_ok (s5fxp_api.hip) fails: ((L + 3) / 4 + 2 * SCAN_DEPTH) * P * 32 >= 2^32 - 1."""
    ok = lambda L: ((L + 3) // 4 + 2 * SCAN_DEPTH) * (P if P else 1) * 32 < 0xffffffff
    blocks = -(-0xffffffff // (32 * (P if P else 1))) - 2 * SCAN_DEPTH   # the smallest failing number of 4-step blocks
    L = 4 * (blocks - 1) + 1
    assert not ok(L) and ok(L - 1) and 0 < L < 2 ** 31
    return L


def test_check_order_of_the_three_entries(monkeypatch):
    """A call that fails more than one check returns: bad arguments first, then unsupported, then the workspace, then the stream
    extent.  All of these return before any launch: y and the status words keep their sentinels."""
    import torch
    from sparsernns_amd import _lib
    from sparsernns_amd._lib import lib
    import contract_models as CM

    eng = _engine(monkeypatch, False)
    wide = CM.case("F3_out32_ds0.5").engine()
    assert wide.out_bits > 16
    B, L = 2, 5
    stream = torch.cuda.current_stream().cuda_stream
    entries = {torch.int32: (lib.s5fxp_model_forward, lib.s5fxp_workspace_bytes),
               torch.float32: (lib.s5fxp_model_forward_f32, lib.s5fxp_workspace_bytes_f32),
               torch.int16: (lib.s5fxp_model_forward_i16, lib.s5fxp_workspace_bytes_i16)}
    seen = []
    eng.lane_status(0).fill_(-9)
    wide.lane_status(0).fill_(-9)

    def call(e, dtype, xb, xe, L=L, size=None):
        """size None: the lane's real workspace, passed as one byte short"""
        fn, query = entries[dtype]
        name = str(dtype).split(".")[1]
        x = torch.zeros((B, 5, e.d_in), dtype=dtype, device="cuda")
        y = torch.full((B, 5, e.d_out), SENT[name], dtype=dtype, device="cuda")
        st = e.lane_status(0)
        ws = e.workspace(B, 5, io=dtype)
        assert ws.numel() == query(e._h, B, 5)
        rc = fn(e._h, x.data_ptr(), xb, xe, B, L, y.data_ptr(), ws.data_ptr(), ws.numel() - 1 if size is None else size,
                st.data_ptr(), None, None, stream)
        seen.append((y, SENT[name]))
        return rc

    for dtype in entries:
        assert call(eng, dtype, eng.inp_bits, eng.inp_exp) == _lib.S5FXP_EWORKSPACE, dtype
    assert call(eng, torch.float32, eng.inp_bits, 32) == _lib.S5FXP_EBADARG
    assert call(eng, torch.int16, 17, eng.inp_exp) == _lib.S5FXP_EBADARG
    assert call(wide, torch.int16, wide.inp_bits, wide.inp_exp) == _lib.S5FXP_EUNSUPPORTED
    # a workspace that passes for a sequence whose stream extent does not: nothing is dereferenced before that check, so the
    # size is a claim and the pointer the lane's real workspace
    Lbad = _smallest_bad_extent_L(eng.P)
    size = 1 << 62
    assert lib.s5fxp_workspace_bytes_f32(eng._h, B, Lbad) <= size
    assert call(eng, torch.float32, eng.inp_bits, eng.inp_exp, L=Lbad, size=size) == _lib.S5FXP_EBADARG
    torch.cuda.synchronize()
    for y, sent in seen:
        assert bool((y == sent).all()), "y was written"
    assert bool((eng.lane_status(0) == -9).all()) and bool((wide.lane_status(0) == -9).all()), "status words were written"
