"""ggnn_rnn_bwd_fused_f32 / ggnn_rnn_bwd_fused_gather_f32 (csrc/ggnn_rnn_fused.hip): the whole BasicRNNCell backward of a timestep
in one launch, every supported (D, nx), both activations, mean and sum aggregation.

Per case: (1) dP is torch.equal to ggnn_act_bwd_f32 on the same inputs, (2) dx / d_incoming / dh are within
variant_kernel_ref.bwd_dx_bounds at factor 1 of the float64 product on the GPU's own dP -- the project's bound for the launches being
replaced --, (3) the same outputs are within the same bound of ggnn_act_bwd_f32 + ggnn_bwd_dx_f32 (what variants._hip_backward
launches), (4) two runs are bit-identical and rows beyond V of over-allocated, NaN-prefilled outputs stay untouched, (5) the gather
form is torch.equal to ggnn_gather_segment_sum_heads_f32(accumulate = 1) into g followed by the plain form.
`out` carries +0.0, -0.0 and negative entries (ReLU's edge: the derivative is 0 at and below 0), nin an all-zero row (the mean divides
by 1e-7 there).  V: 1, 15, 16, 17, one more than a workgroup covers per round, and one more than a whole round of the tile loop.
"""
import ctypes

import numpy as np
import pytest
import torch

import variant_kernel_ref as ref

pytestmark = pytest.mark.gpu

SUPPORTED = [(32, 1), (32, 2), (32, 3), (64, 1), (64, 2), (64, 3), (100, 1)]
PAD_ROWS = 24
T = 3
ALL_SWITCHES = [(True, "tanh"), (True, "relu"), (False, "tanh"), (False, "relu")]
E_INVALID, E_UNSUPPORTED = -1, -2                      # include/ggnn_hip.h


@pytest.fixture(scope="module")
def ops(pkg, cuda):
    return pkg.ops


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(D, nx, V, seed):
    rng = np.random.default_rng(seed)
    K = (nx + 1) * D
    g = rng.normal(size=(V, D)).astype(np.float32)
    out = rng.uniform(-1, 1, (V, D)).astype(np.float32)
    out[:, 3] = 0.0                                     # +0.0
    out[:, 7] = -0.0
    out[:, D - 2] = -np.abs(out[:, D - 2]) - 0.25       # a negative column
    out[V // 2, :] = np.abs(out[V // 2, :]) + 0.125     # a row that is positive everywhere ...
    out[V // 2, 3], out[V // 2, 7], out[V // 2, D - 2] = 0.0, -0.0, -0.5      # ... but for the two zeros and the negative column
    W = (rng.uniform(-1, 1, (K, D)) * 2.0 / np.sqrt(K)).astype(np.float32)
    nin = rng.integers(0, 4, (V, T)).astype(np.float32)
    nin[0] = 0.0
    return g, out, W, nin


def _launch(pkg, g, out, packed, nin, use_avg, nx, act, gather=None, V=None):
    """The C entry point on caller-owned, over-allocated, NaN-prefilled outputs -> (rc, dP, [dx_0 .. dx_{nx-1}], dh), each
    [V + PAD_ROWS, D]."""
    lib = pkg._lib.load()
    V = out.shape[0] if V is None else V
    D = out.shape[1]
    mk = lambda: torch.full((out.shape[0] + PAD_ROWS, D), float("nan"), device=out.device)
    dP, dh, dx = mk(), mk(), [mk() for _ in range(nx)]
    dxp = (ctypes.c_void_p * nx)(*[t.data_ptr() for t in dx])
    st = torch.cuda.current_stream().cuda_stream
    if gather is None:
        rc = lib.ggnn_rnn_bwd_fused_f32(g.data_ptr(), out.data_ptr(), packed.data_ptr(), dP.data_ptr(), dxp, dh.data_ptr(), nin.data_ptr(),
                                        T, 1 if use_avg else 0, nx, V, D, pkg.ops.ACT_IDS[act], st)
    else:
        gz, heads = gather
        rc = lib.ggnn_rnn_bwd_fused_gather_f32(g.data_ptr(), gz.data_ptr(), heads.data_ptr(), gz.shape[0], out.data_ptr(), packed.data_ptr(),
                                               dP.data_ptr(), dxp, dh.data_ptr(), nin.data_ptr(), T, 1 if use_avg else 0, nx, V, D,
                                               pkg.ops.ACT_IDS[act], st)
    return rc, dP, dx, dh


def _check_case(pkg, ops, cuda, D, nx, V, switches):
    seed = ref.seed_of("rnn_bwd_fused", D, nx, V)
    g_np, out_np, W_np, nin_np = _inputs(D, nx, V, seed)
    g, out, W, nin = (_dev(a, cuda) for a in (g_np, out_np, W_np, nin_np))
    packed = ops.rnn_bwd_pack(W, nx)
    assert packed.numel() * 4 == pkg._lib.load().ggnn_rnn_bwd_packed_bytes(D, nx)
    assert torch.equal(packed, ops.PACKED.rnn_bwd(W, nx, D))
    WT_np = np.ascontiguousarray(W_np.T)
    WT = pkg.backward.transposed(W)
    for use_avg, act in switches:
        what = "rnn_bwd_fused.D%d.nx%d[V=%d avg=%d %s]" % (D, nx, V, use_avg, act)
        rc, dP, dx, dh = _launch(pkg, g, out, packed, nin, use_avg, nx, act)
        assert rc == 0, what
        rc2, dP2, dx2, dh2 = _launch(pkg, g, out, packed, nin, use_avg, nx, act)
        # (1) dP: the stand-alone launch's bits (and its float64 bound, so that two equal wrong results do not pass)
        want_dP = ops.act_bwd(g, out, act)
        assert torch.equal(dP[:V], want_dP), what + ": dP differs from ggnn_act_bwd_f32"
        ref.assert_within(_np(dP[:V]), ref.act_bwd(g_np, out_np, act), ref.act_bwd_bound(g_np, out_np, act), 1, what + " dP")
        if act == "relu":
            got = _np(dP[:V])
            assert not got[:, 3].any() and not got[:, 7].any() and not got[:, D - 2].any(), what + ": ReLU' must be 0 at +0, -0 and below"
            assert np.array_equal(np.delete(got[V // 2], [3, 7, D - 2]), np.delete(g_np[V // 2], [3, 7, D - 2])), what + ": ReLU' must be 1 above 0"
        # (2) the products against float64 on the GPU's own dP
        dP_np = _np(dP[:V])
        dx0 = np.zeros((V, nx * D), np.float32)
        args = (dP_np, 1, WT_np, nx * D, True, dx0, nin_np, use_avg, None, False, False, D)
        want_dx, want_inc, want_dh = ref.bwd_dx(*args)
        Bdx, Binc, Bdh = ref.bwd_dx_bounds(*args)
        for s in range(nx - 1):
            ref.assert_within(_np(dx[s][:V]), want_dx[:, s * D:(s + 1) * D], Bdx[:, s * D:(s + 1) * D], 1, what + " dx[%d]" % s)
        ref.assert_within(_np(dx[nx - 1][:V]), want_inc, Binc, 1, what + " dinc")
        ref.assert_within(_np(dh[:V]), want_dh, Bdh, 1, what + " dh")
        # (3) ... and against the two launches being replaced
        old_dx = torch.empty((V, nx * D), dtype=torch.float32, device=cuda)
        old_inc, old_dh = torch.empty_like(out), torch.empty_like(out)
        ops.bwd_dx(want_dP, 1, WT, nx * D, True, old_dx, old_inc, nin, use_avg, old_dh, False, False, D)
        for s in range(nx - 1):
            ref.assert_within(_np(dx[s][:V]), _np(old_dx[:, s * D:(s + 1) * D]), Bdx[:, s * D:(s + 1) * D], 1, what + " dx[%d] vs bwd_dx" % s)
        ref.assert_within(_np(dx[nx - 1][:V]), _np(old_inc), Binc, 1, what + " dinc vs bwd_dx")
        ref.assert_within(_np(dh[:V]), _np(old_dh), Bdh, 1, what + " dh vs bwd_dx")
        # (4) run to run, and nothing beyond V
        assert rc2 == 0 and torch.equal(dP[:V], dP2[:V]) and torch.equal(dh[:V], dh2[:V]), what + ": two runs differ"
        assert all(torch.equal(a[:V], b[:V]) for a, b in zip(dx, dx2)), what + ": two runs differ"
        for buf in [dP, dh] + dx:
            assert bool(torch.isnan(buf[V:]).all()), what + ": rows beyond V were written"
        # the host-layer wrapper runs the same launch
        w_dP, w_dh, w_dx = ops.rnn_bwd_fused(g, out, packed, nin, use_avg, nx, act)
        assert torch.equal(w_dP, dP[:V]) and torch.equal(w_dh, dh[:V]) and all(torch.equal(a, b[:V]) for a, b in zip(w_dx, dx)), what


@pytest.mark.parametrize("V", [1, 15, 16, 17])
@pytest.mark.parametrize("D,nx", SUPPORTED)
def test_fused_backward(pkg, ops, cuda, D, nx, V):
    assert ops.rnn_bwd_fused_supported(D, nx)
    _check_case(pkg, ops, cuda, D, nx, V, ALL_SWITCHES)


@pytest.mark.parametrize("D,nx", SUPPORTED)
def test_more_than_one_workgroup_and_a_second_round(pkg, ops, cuda, D, nx):
    """One row more than a workgroup covers per round, and one row more than a whole round of the tile loop (the geometry is the
    forward's: the same RnnCfg), so a wave takes a second tile."""
    rows, wgs = ops.rnn_fused_launch_geometry(D, nx)
    assert rows > 0 and rows % 16 == 0 and wgs > 0
    _check_case(pkg, ops, cuda, D, nx, rows + 1, [(True, "tanh"), (False, "relu")])
    _check_case(pkg, ops, cuda, D, nx, rows * wgs + 1, [(True, "relu")])


def _gather_inputs(pkg, cuda, V, D, seed):
    """gz [R, D] and a CSR in which node v owns 0, 1, 2, 3, 4, 4, 0, 1, .. rows (a head record holds four)
    -> (gz, row_ptr, gather_row, heads [V, 4])."""
    rng = np.random.default_rng(seed)
    counts = (np.arange(V) % 6).astype(np.int64)
    counts[counts == 5] = 4
    if V > 4:
        assert set(counts.tolist()) >= {0, 1, 4}
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    R = max(int(row_ptr[-1]), 1)
    gather_row = rng.permutation(R).astype(np.int32)[:int(row_ptr[-1])]
    gz = rng.normal(size=(R, D)).astype(np.float32)
    gz_t, rp_t, gr_t = _dev(gz, cuda), _dev(row_ptr, cuda), _dev(gather_row if len(gather_row) else np.zeros(1, np.int32), cuda)
    heads = torch.empty((V, 4), dtype=torch.int32, device=cuda)
    pkg._lib.check(pkg._lib.load().ggnn_build_slot_heads(rp_t.data_ptr(), gr_t.data_ptr(), heads.data_ptr(), V,
                                                         torch.cuda.current_stream().cuda_stream))
    return gz_t, rp_t, gr_t, heads


@pytest.mark.parametrize("V", [1, 17, 300])
@pytest.mark.parametrize("D,nx", SUPPORTED)
def test_gather_form_equals_heads_sum_then_plain_form(pkg, ops, cuda, D, nx, V):
    lib = pkg._lib.load()
    seed = ref.seed_of("rnn_bwd_gather", D, nx, V)
    g_np, out_np, W_np, nin_np = _inputs(D, nx, V, seed)
    g, out, W, nin = (_dev(a, cuda) for a in (g_np, out_np, W_np, nin_np))
    packed = ops.rnn_bwd_pack(W, nx)
    gz, row_ptr, gather_row, heads = _gather_inputs(pkg, cuda, V, D, seed + 1)
    h_np = _np(heads)
    assert (h_np == -1).any() and (V < 5 or ((h_np >= 0).sum(1) == 4).any())
    for use_avg, act in [(True, "relu"), (False, "tanh")]:
        what = "rnn_bwd_gather.D%d.nx%d[V=%d avg=%d %s]" % (D, nx, V, use_avg, act)
        g_sum = g.clone()
        pkg._lib.check(lib.ggnn_gather_segment_sum_heads_f32(gz.data_ptr(), row_ptr.data_ptr(), gather_row.data_ptr(), heads.data_ptr(), None,
                                                             None, 0, g_sum.data_ptr(), V, D, 1, 1, torch.cuda.current_stream().cuda_stream))
        assert V < 2 or not torch.equal(g_sum, g)
        rc_p, dP_p, dx_p, dh_p = _launch(pkg, g_sum, out, packed, nin, use_avg, nx, act)
        rc_g, dP_g, dx_g, dh_g = _launch(pkg, g, out, packed, nin, use_avg, nx, act, gather=(gz, heads))
        assert rc_p == 0 and rc_g == 0
        assert torch.equal(dP_g[:V], dP_p[:V]) and torch.equal(dh_g[:V], dh_p[:V]), what
        assert all(torch.equal(a[:V], b[:V]) for a, b in zip(dx_g, dx_p)), what
        for buf in [dP_g, dh_g] + dx_g:
            assert bool(torch.isnan(buf[V:]).all()), what + ": rows beyond V were written"
        w = ops.rnn_bwd_fused(g, out, packed, nin, use_avg, nx, act, gather=(gz, heads))
        assert torch.equal(w[0], dP_g[:V]) and torch.equal(w[1], dh_g[:V])


def test_heads_outside_the_rows_add_nothing(pkg, ops, cuda):
    """A head entry of -1 or outside [0, num_rows) adds nothing and is not dereferenced: the launch on gz cut short equals the launch
    whose records name only the rows that are left."""
    D, nx, V = 64, 2, 40
    seed = ref.seed_of("rnn_bwd_gather_oob")
    g_np, out_np, W_np, nin_np = _inputs(D, nx, V, seed)
    g, out, W, nin = (_dev(a, cuda) for a in (g_np, out_np, W_np, nin_np))
    packed = ops.rnn_bwd_pack(W, nx)
    gz, _, _, heads = _gather_inputs(pkg, cuda, V, D, seed + 1)
    keep = gz.shape[0] - 7
    cut = heads.clone()
    cut[cut >= keep] = -1
    assert not torch.equal(cut, heads)
    short = gz[:keep].contiguous()
    _, dP_a, dx_a, dh_a = _launch(pkg, g, out, packed, nin, True, nx, "tanh", gather=(short, heads))
    _, dP_b, dx_b, dh_b = _launch(pkg, g, out, packed, nin, True, nx, "tanh", gather=(short, cut))
    assert torch.equal(dP_a[:V], dP_b[:V]) and torch.equal(dh_a[:V], dh_b[:V]) and all(torch.equal(a[:V], b[:V]) for a, b in zip(dx_a, dx_b))
    _, dP_c, _, _ = _launch(pkg, g, out, packed, nin, True, nx, "tanh", gather=(gz, heads))
    assert not torch.equal(dP_a[:V], dP_c[:V])              # (the cut rows did carry gradient)


def test_refusals_leave_the_outputs_untouched(pkg, ops, cuda):
    """Unsupported (D, nx), aliasing, misalignment and the 2^30 limit: each returns its error code before anything is launched."""
    lib = pkg._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    V, D, nx = 17, 32, 1
    g_np, out_np, W_np, nin_np = _inputs(D, nx, V, 5)
    g, out, W, nin = (_dev(a, cuda) for a in (g_np, out_np, W_np, nin_np))
    packed = ops.rnn_bwd_pack(W, nx)
    sentinel = lambda: torch.full((V + 1, D), -7.0, device=cuda)

    def call(g_ptr, out_ptr, dP, dinc, dh, nx=nx, V=V, D=D):
        dxp = (ctypes.c_void_p * 3)(*([dinc.data_ptr()] * 3))
        return lib.ggnn_rnn_bwd_fused_f32(g_ptr, out_ptr, packed.data_ptr(), dP.data_ptr(), dxp, dh.data_ptr(), nin.data_ptr(), T, 1, nx, V, D,
                                          0, st)

    cases = {
        "unsupported D": (dict(D=48), E_UNSUPPORTED),
        "unsupported nx at D = 100": (dict(D=100, nx=2), E_UNSUPPORTED),
        "nx = 4": (dict(nx=4), E_UNSUPPORTED),
        "V * D = 2^30": (dict(V=(1 << 30) // D), E_UNSUPPORTED),
    }
    for name, (kw, code) in cases.items():
        dP, dinc, dh = sentinel(), sentinel(), sentinel()
        assert call(g.data_ptr(), out.data_ptr(), dP, dinc, dh, **kw) == code, name
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in (dP, dinc, dh)), name
    for name, fn in {
        "dP aliases g": lambda dP, dinc, dh: lib.ggnn_rnn_bwd_fused_f32(
            dP.data_ptr(), out.data_ptr(), packed.data_ptr(), dP.data_ptr(), (ctypes.c_void_p * 1)(dinc.data_ptr()), dh.data_ptr(),
            nin.data_ptr(), T, 1, nx, V, D, 0, st),
        "dh aliases out": lambda dP, dinc, dh: lib.ggnn_rnn_bwd_fused_f32(
            g.data_ptr(), dh.data_ptr(), packed.data_ptr(), dP.data_ptr(), (ctypes.c_void_p * 1)(dinc.data_ptr()), dh.data_ptr(),
            nin.data_ptr(), T, 1, nx, V, D, 0, st),
        "dinc aliases dh": lambda dP, dinc, dh: lib.ggnn_rnn_bwd_fused_f32(
            g.data_ptr(), out.data_ptr(), packed.data_ptr(), dP.data_ptr(), (ctypes.c_void_p * 1)(dh.data_ptr()), dh.data_ptr(),
            nin.data_ptr(), T, 1, nx, V, D, 0, st),
        "misaligned g": lambda dP, dinc, dh: call(g.data_ptr() + 4, out.data_ptr(), dP, dinc, dh, V=V - 1),
        "misaligned dP": lambda dP, dinc, dh: lib.ggnn_rnn_bwd_fused_f32(
            g.data_ptr(), out.data_ptr(), packed.data_ptr(), dP.data_ptr() + 4, (ctypes.c_void_p * 1)(dinc.data_ptr()), dh.data_ptr(),
            nin.data_ptr(), T, 1, nx, V - 1, D, 0, st),
    }.items():
        dP, dinc, dh = sentinel(), sentinel(), sentinel()
        assert fn(dP, dinc, dh) == E_INVALID, name
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in (dP, dinc, dh)), name
    # the gather form: num_rows * D at the limit, and a misaligned head table
    gz, _, _, heads = _gather_inputs(pkg, cuda, V, D, 6)
    for name, rows, heads_ptr, code in (("num_rows * D = 2^30", (1 << 30) // D, heads.data_ptr(), E_UNSUPPORTED),
                                        ("misaligned heads", gz.shape[0], heads.data_ptr() + 4, E_INVALID)):
        dP, dinc, dh = sentinel(), sentinel(), sentinel()
        rc = lib.ggnn_rnn_bwd_fused_gather_f32(g.data_ptr(), gz.data_ptr(), heads_ptr, rows, out.data_ptr(), packed.data_ptr(), dP.data_ptr(),
                                               (ctypes.c_void_p * 1)(dinc.data_ptr()), dh.data_ptr(), nin.data_ptr(), T, 1, nx, V, D, 0, st)
        assert rc == code, name
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in (dP, dinc, dh)), name
    # the packer refuses what the launch refuses
    img = torch.empty(16, dtype=torch.float32, device=cuda)
    assert lib.ggnn_rnn_bwd_pack_weights_f32(W.data_ptr(), 2, 100, img.data_ptr(), st) == E_UNSUPPORTED
    assert lib.ggnn_rnn_bwd_packed_bytes(100, 2) == 0
