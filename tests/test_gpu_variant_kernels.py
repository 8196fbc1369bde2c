"""The kernels behind the non-default model switches (use_propagation_attention, graph_rnn_cell: RNN / CudnnCompatibleGRUCell) and
the generic backward kernels, each called directly and held to the float64 formulas and a-priori bounds of
tests/variant_kernel_ref.py at factor 2 -- per element, so a single bad row, lane or message id fails.

Every case is a handful of launches on at most a few thousand rows; the shapes are the smallest that reach each code path
(sub-wave widths and idle lanes, dead sub-waves, the K remainder, partial column groups, clamped row tiles, float4 tails).
tests/test_variant_kernel_ref_host.py shows on the CPU that the references are independent, that float32 stays inside factor 1
on these very inputs, and that the comparison has teeth.
"""
import ctypes

import numpy as np
import pytest
import torch

import variant_kernel_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 2
SENTINEL = -777.25


@pytest.fixture(scope="module")
def ops(pkg, cuda):
    return pkg.ops


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np(t):
    return t.detach().cpu().numpy()


def _transform(ops, c, h, W, cuda):
    """H [V, T*D] float32 on the device, from ops.msg_transform where the generic GEMM takes the hidden size (a multiple of 32
    or 100), else (D = 132: reachable at kernel level only) a float32 product from the CPU.  Either way the reference is fed
    these very float32 values."""
    V, D = c["h"].shape
    if D % 32 and D % 100:
        return _dev(ref.transform_rows(c["h"], c["W"], np.float32).reshape(V, -1), cuda)
    return ops.msg_transform(h, W)


def _graph(ops, c, cuda):
    V = c["h"].shape[0]
    return ops.build_message_index([_dev(a, cuda) for a in c["adj"]], V)


# ---- propagation attention ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", ref.ATTN_T)
@pytest.mark.parametrize("V", ref.ATTN_V)
@pytest.mark.parametrize("D", ref.ATTN_D)
def test_attention_forward(ops, cuda, D, V, T):
    c = ref.attn_inputs(D, V, T, ref.seed_of("attn", D, V, T))
    h, W, f, nin, bias = (_dev(c[k], cuda) for k in ("h", "W", "factors", "nin", "bias"))
    index = _graph(ops, c, cuda)
    H = _transform(ops, c, h, W, cuda)
    Hrows = _np(H).reshape(V * T, D)                       # the kernel's own float32 input: only the kernel under test is measured
    for bias_on, use_avg in ref.ATTN_SWITCHES:
        out = ops.gather_segment_sum_attn(H, h, index, f, nin, bias if bias_on else None, use_avg)
        again = ops.gather_segment_sum_attn(H, h, index, f, nin, bias if bias_on else None, use_avg)
        assert torch.equal(out, again), "two calls differ"
        a = (c["h"], Hrows, c["adj"], c["factors"], c["nin"], c["bias"] if bias_on else None, use_avg)
        ref.assert_within(_np(out), ref.attn_forward(*a), ref.attn_forward_bound(*a), FACTOR,
                          "attn_forward.D%d[V=%d T=%d bias=%d avg=%d]" % (D, V, T, bias_on, use_avg))
        if V > 1 and not bias_on:
            assert not _np(out)[0].any(), "node 0 receives nothing: its row must be exactly zero"


def test_attention_forward_saturated(ops, cuda):
    """Scores far beyond what exp() of an unshifted score survives in float32."""
    D, V, T = 64, 17, 3
    c = ref.attn_inputs(D, V, T, ref.seed_of("saturated"), saturate=True)
    src, dst, typ, p, s, m, S, a_ = ref._softmax(c["h"], c["adj"], c["factors"], np.float64)
    hub = s[dst == V - 1]
    assert hub.max() - hub.min() > 90 and hub.max() > 89
    h, W, f, nin = (_dev(c[k], cuda) for k in ("h", "W", "factors", "nin"))
    H = ops.msg_transform(h, W)
    out = _np(ops.gather_segment_sum_attn(H, h, _graph(ops, c, cuda), f, nin, None, False))
    assert np.isfinite(out).all()
    a = (c["h"], _np(H).reshape(V * T, D), c["adj"], c["factors"], c["nin"], None, False)
    ref.assert_within(out, ref.attn_forward(*a), ref.attn_forward_bound(*a), FACTOR, "attn_forward.saturated")


def _attention_backward(ops, H, h, d, index, f, dh):
    """The attention launches of variants._hip_backward on an index with messages, launch for launch:
    -> (coef_a, coef_s, d factor); dh is added to."""
    D = h.shape[1]
    assert index.num_messages
    comp = getattr(index, "_compact", None)
    if comp is None:
        comp = index._compact = ops.build_compact_sources(index)
    coef_a, coef_s, dfac = ops.attn_backward_target(H.view(-1, D), h, d, index, f, dh)
    dattn = ops.range_sum(dfac, index.type_off)
    bwd = ops.compact_backward(index, comp)
    ops.weighted_segment_sum(h, bwd.source_node_index, bwd.source_node_index.msg, coef_s, out=dh, accumulate=True)
    return coef_a, coef_s, dattn


@pytest.mark.parametrize("T", ref.ATTN_T)
@pytest.mark.parametrize("V", ref.ATTN_V)
@pytest.mark.parametrize("D", ref.ATTN_D)
def test_attention_backward(ops, cuda, D, V, T):
    c = ref.attn_inputs(D, V, T, ref.seed_of("attn", D, V, T))
    h, W, f, d = (_dev(c[k], cuda) for k in ("h", "W", "factors", "d"))
    index = _graph(ops, c, cuda)
    H = _transform(ops, c, h, W, cuda)
    dh = _dev(c["dh0"], cuda)                              # prefilled: both passes must add to it
    coef_a, coef_s, dattn = _attention_backward(ops, H, h, d, index, f, dh)
    a = (c["h"], _np(H).reshape(V * T, D), c["d"], c["adj"], c["factors"])
    want, B = ref.attn_backward(*a), ref.attn_backward_bounds(*a, dh_prefill=c["dh0"])
    tag = "[V=%d T=%d]" % (V, T)
    ref.assert_within(_np(coef_a), want["coef_a"], B["coef_a"], FACTOR, "attn_backward.coef_a.D%d%s" % (D, tag))     # by message id
    ref.assert_within(_np(coef_s), want["coef_s"], B["coef_s"], FACTOR, "attn_backward.coef_s.D%d%s" % (D, tag))
    ref.assert_within(_np(dattn), want["dfactor"], B["dfactor"], FACTOR, "attn_backward.dfactor.D%d%s" % (D, tag))
    ref.assert_within(_np(dh), c["dh0"].astype(np.float64) + want["dh_target"] + want["dh_source"], B["dh"], FACTOR,
                      "attn_backward.dh.D%d%s" % (D, tag))
    if c["info"]["empty_type"] is not None:
        assert _np(dattn)[c["info"]["empty_type"]] == 0.0, "d factor of the empty edge type must be exactly 0"


def test_attention_without_messages(pkg, ops, cuda):
    """M = 0.  The forward kernel gives exact zeros and the target-side backward kernel adds nothing.  Then the product's own
    backward: variants.variant_step with attention weights and a BasicRNNCell on the empty index, differentiated -- that is
    the `not index.num_messages` branch of variants._hip_backward, with build_compact_sources on the empty index and
    transform_backward on zero compact rows.  d attention weights and d edge weights must be exactly 0, and d h is the
    cell's alone: act_bwd then bwd_dx of the float64 reference."""
    import importlib
    variants = importlib.import_module(pkg.__name__ + ".variants")
    D, V, T = 100, 17, 3
    c = ref.attn_inputs(D, V, T, ref.seed_of("empty"))
    cell = ref.cell_inputs(D, V, 1, ref.seed_of("empty cell"))
    h, W, f, d = (_dev(c[k], cuda) for k in ("h", "W", "factors", "d"))
    index = ops.build_message_index([torch.zeros((0, 2), dtype=torch.int32, device=cuda) for _ in range(T)], V)
    assert index.num_messages == 0
    H = ops.msg_transform(h, W)
    nin = torch.zeros((V, T), device=cuda)
    out = ops.gather_segment_sum_attn(H, h, index, f, nin, _dev(c["bias"], cuda), True)
    assert not _np(out).any()
    dh = _dev(c["dh0"], cuda)
    ops.attn_backward_target(H.view(-1, D), h, d, index, f, dh)
    np.testing.assert_array_equal(_np(dh), c["dh0"])

    assert variants.BACKWARD_ORACLE is None                # the hand-written backward, not a test oracle
    Wc, bc = _dev(cell["W"], cuda), _dev(cell["b"], cuda)
    for t in (h, W, f):
        t.requires_grad_(True)
    out = variants.variant_step(h, index, nin, W, None, f, True, [], "rnn", [Wc, bc], "tanh")
    out.backward(d)
    a = (c["h"], c["d"], cell["W"], cell["b"])
    (want_out, want_dh), (B_out, B_dh) = ref.empty_graph_rnn_step(*a), ref.empty_graph_rnn_step_bounds(*a)
    ref.assert_within(_np(out), want_out, B_out, FACTOR, "empty_graph.rnn_out")
    ref.assert_within(_np(h.grad), want_dh, B_dh, FACTOR, "empty_graph.dh")
    assert f.grad.shape == f.shape and not _np(f.grad).any(), "d attention weights must be exactly 0"
    assert W.grad.shape == W.shape and not _np(W.grad).any(), "d edge weights must be exactly 0"


# ---- sums ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", ref.WSS_NSEG)
@pytest.mark.parametrize("D", ref.WSS_D)
def test_weighted_segment_sum(ops, cuda, D, nseg):
    c = ref.wss_inputs(D, nseg, ref.seed_of("wss", D, nseg))
    assert c["gather_row"].max() < len(c["rows"]) and c["weight_id"].max() < len(c["weights"])
    index = ops.SegmentIndex(_dev(c["row_ptr"], cuda), _dev(c["gather_row"], cuda), nseg)
    rows, wid, w = _dev(c["rows"], cuda), _dev(c["weight_id"], cuda), _dev(c["weights"], cuda)
    for acc in (False, True):
        out = _dev(c["out0"], cuda)                        # prefilled either way: without accumulate it must be overwritten
        got = ops.weighted_segment_sum(rows, index, wid, w, out=out, accumulate=acc)
        assert got is out
        a = (c["rows"], c["row_ptr"], c["gather_row"], c["weight_id"], c["weights"], c["out0"] if acc else None)
        ref.assert_within(_np(out), ref.weighted_segment_sum(*a), ref.weighted_segment_sum_bound(*a), FACTOR,
                          "weighted_segment_sum.%s[D=%d nseg=%d acc=%d]" % ("strided" if D > 256 else "direct", D, nseg, acc))
        if nseg > 1 and not acc:
            assert not _np(out)[nseg // 2].any(), "the empty segment must be exactly zero"


@pytest.mark.parametrize("which", ["lengths", "64"])
def test_range_sum(ops, cuda, which):
    v, off = ref.range_inputs(ref.seed_of("range")) if which == "lengths" else ref.range_inputs_64(ref.seed_of("range64"))
    assert off[-1] == len(v)
    values = _dev(v, cuda)
    out = ops.range_sum(values, off)
    assert torch.equal(out, ops.range_sum(values, off)), "two calls differ"
    ref.assert_within(_np(out), ref.range_sum(v, off), ref.range_sum_bound(v, off), FACTOR, "range_sum." + which)
    empty = [b for b in range(len(off) - 1) if off[b] == off[b + 1]]
    assert empty and not _np(out)[empty].any(), "an empty range must be exactly 0"


# ---- cells --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", ref.CELL_NX)
@pytest.mark.parametrize("V", ref.CELL_V)
@pytest.mark.parametrize("D", ref.CELL_D)
def test_rnn_cell(ops, cuda, D, V, nx):
    c = ref.cell_inputs(D, V, nx, ref.seed_of("cell", D, V, nx))
    xs, h, W, b = [_dev(x, cuda) for x in c["xs"]], _dev(c["h"], cuda), _dev(c["W"], cuda), _dev(c["b"], cuda)
    for act in ("tanh", "relu"):
        out = _np(ops.rnn(xs, h, W, b, act))
        a = (c["xs"], c["h"], c["W"], c["b"], act)
        ref.assert_within(out, ref.rnn(*a), ref.rnn_bound(*a), FACTOR, "rnn.%s.D%d[V=%d nx=%d]" % (act, D, V, nx))
        if act == "relu":                                  # pre-activation exactly 0 (column 5) and negative (column D-3)
            assert not out[:, 5].any() and not out[:, D - 3].any()


@pytest.mark.parametrize("nx", ref.CELL_NX)
@pytest.mark.parametrize("V", ref.CELL_V)
@pytest.mark.parametrize("D", ref.CELL_D)
def test_cudnn_gru_cell(ops, cuda, D, V, nx):
    c = ref.cell_inputs(D, V, nx, ref.seed_of("cell", D, V, nx))
    xs, h = [_dev(x, cuda) for x in c["xs"]], _dev(c["h"], cuda)
    cud = {k: _dev(v, cuda) for k, v in c["cudnn"].items()}
    plain = ops.cudnn_gru(xs, h, **cud)
    got = ops.cudnn_gru_train(xs, h, **cud)                # -> (h', r, u, c, hc)
    assert torch.equal(plain, got[0]), "cudnn_gru and cudnn_gru_train differ in h'"
    want = ref.cudnn_gru(c["xs"], c["h"], **c["cudnn"])
    B = ref.cudnn_gru_bounds(c["xs"], c["h"], **c["cudnn"])
    for name, g, w, bnd in zip(("out", "r", "u", "c", "hc"), got, want, B):
        ref.assert_within(_np(g), w, bnd, FACTOR, "cudnn_gru.%s.D%d[V=%d nx=%d]" % (name, D, V, nx))


# ---- the general dX product ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", ref.BWD_DX_NX)
@pytest.mark.parametrize("V", ref.BWD_DX_V)
@pytest.mark.parametrize("D", ref.BWD_DX_D)
@pytest.mark.parametrize("shape", ref.BWD_DX_SHAPES)
def test_bwd_dx(ops, cuda, shape, D, V, nx):
    c = ref.bwd_dx_inputs(shape, D, V, nx, ref.seed_of("bwd_dx", shape, D, V, nx))
    dYbuf = _dev(c["dYbuf"], cuda)
    dY = dYbuf[:, :c["width"]]                             # row stride 8 floats larger than the width
    assert V == 1 or dY.stride(0) == c["width"] + 8
    K = c["WT"].shape[1]
    dx = None if c["dx0"] is None else _dev(c["dx0"], cuda)
    dh = None if c["dh0"] is None else _dev(c["dh0"], cuda)
    dinc = torch.full((V, D), SENTINEL, device=cuda) if c["split_inc"] else None
    nin = None if c["nin"] is None else _dev(c["nin"], cuda)
    ops.bwd_dx(dY, c["nseg_y"], _dev(c["WT"], cuda), c["xcols"], c["split_inc"], dx, dinc, nin, c["use_avg"], dh, c["acc_dx"],
               c["acc_dh"], D)
    a = ref.bwd_dx_args(c)
    want, B = ref.bwd_dx(*a), ref.bwd_dx_bounds(*a)
    assert (want[1] is None) == (dinc is None) and (want[2] is None) == (dh is None) and K in (c["xcols"], c["xcols"] + D)
    for name, g, w, bnd in zip(("dx", "dinc", "dh"), (dx, dinc, dh), want, B):
        if w is not None:
            ref.assert_within(_np(g), w, bnd, FACTOR, "bwd_dx.%s.%s.D%d[V=%d nx=%d]" % (shape, name, D, V, nx))
    np.testing.assert_array_equal(_np(dYbuf), c["dYbuf"])


# ---- element-wise stages ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,D", ref.ELEMENTWISE_SHAPES)
def test_act_bwd_and_cudnn_stage(ops, cuda, V, D):
    c = ref.elementwise_inputs(V, D, ref.seed_of("elementwise", V, D))
    t = {k: _dev(v, cuda) for k, v in c.items()}
    for act, out in (("tanh", "c"), ("relu", "c_relu")):
        got = _np(ops.act_bwd(t["g"], t[out], act))
        ref.assert_within(got, ref.act_bwd(c["g"], c[out], act), ref.act_bwd_bound(c["g"], c[out], act), FACTOR, "act_bwd." + act)
    got = ops.cudnn_gru_bwd_stage(t["g"], t["h"], t["r"], t["u"], t["c"], t["hc"])
    a = (c["g"], c["h"], c["r"], c["u"], c["c"], c["hc"])
    for name, g, w, b in zip(("dpc", "dpg", "dh", "dhc"), got, ref.cudnn_bwd_stage(*a), ref.cudnn_bwd_stage_bounds(*a)):
        ref.assert_within(_np(g), w, b, FACTOR, "cudnn_gru_bwd_stage." + name)


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("V,D", ref.ELEMENTWISE_SHAPES)
def test_gru_backward_stages(pkg, ops, cuda, V, D, act):
    """ggnn_gru_bwd_stage1_f32 / stage2 in the call sequence of backward._backward_dense_form: stage 1 writes r*h into the last
    column block of the [x | r*h] operand, stage 2 reads drh out of the last column block of a [V, K] product."""
    lib = pkg._lib.load()
    check = pkg._lib.check
    st = torch.cuda.current_stream().cuda_stream
    nx = 2
    K = (nx + 1) * D
    c = ref.elementwise_inputs(V, D, ref.seed_of("elementwise", V, D))
    t = {k: _dev(v, cuda) for k, v in c.items()}
    cand = "c" if act == "tanh" else "c_relu"
    a_c = torch.full((V, K), SENTINEL, device=cuda)
    dpc = torch.empty((V, D), device=cuda); dh = torch.empty((V, D), device=cuda)
    dpg = torch.full((V, 2 * D), SENTINEL, device=cuda)
    check(lib.ggnn_gru_bwd_stage1_f32(t["g"].data_ptr(), t["h"].data_ptr(), t["r"].data_ptr(), t["u"].data_ptr(), t[cand].data_ptr(),
                                      ops.ACT_IDS[act], dpc.data_ptr(), dpg.data_ptr(), dh.data_ptr(), a_c.data_ptr(), K, nx * D, V, D, st))
    a = (c["g"], c["h"], c["r"], c["u"], c[cand], act)
    got = (dpc, dpg[:, D:], dh, a_c[:, nx * D:])
    for name, g, w, b in zip(("dpc", "dpu", "dh", "rh"), got, ref.gru_bwd_stage1(*a), ref.gru_bwd_stage1_bounds(*a)):
        ref.assert_within(_np(g), w, b, FACTOR, "gru_bwd_stage1.%s.%s" % (act, name))
    assert (_np(a_c[:, :nx * D]) == SENTINEL).all() and (_np(dpg[:, :D]) == SENTINEL).all(), "stage 1 wrote outside its columns"

    dxrh = torch.full((V, K), SENTINEL, device=cuda)
    dxrh[:, nx * D:] = t["drh"]
    dh2 = _dev(c["dh0"], cuda)
    check(lib.ggnn_gru_bwd_stage2_f32(dxrh.data_ptr() + 4 * nx * D, K, t["h"].data_ptr(), t["r"].data_ptr(), dh2.data_ptr(),
                                      dpg.data_ptr(), V, D, st))
    a = (c["drh"], c["h"], c["r"], c["dh0"])
    for name, g, w, b in zip(("dh", "dpr"), (dh2, dpg[:, :D]), ref.gru_bwd_stage2(*a), ref.gru_bwd_stage2_bounds(*a)):
        ref.assert_within(_np(g), w, b, FACTOR, "gru_bwd_stage2." + name)
    ref.assert_within(_np(dpg[:, D:]), ref.gru_bwd_stage1(c["g"], c["h"], c["r"], c["u"], c[cand], act)[1],
                      ref.gru_bwd_stage1_bounds(c["g"], c["h"], c["r"], c["u"], c[cand], act)[1], FACTOR,
                      "gru_bwd_stage1.%s.dpu[after stage 2]" % act)                   # stage 2 leaves the u half alone


# ---- refusals: the launcher returns before any kernel launch, the outputs stay as they were -----------------------------------
def test_attention_refuses_hidden_size_260(pkg, ops, cuda):
    D, V, T = 260, 17, 3
    c = ref.attn_inputs(D, V, T, ref.seed_of("refuse"))
    h, f, nin, d = (_dev(c[k], cuda) for k in ("h", "factors", "nin", "d"))
    H = torch.zeros((V, T * D), device=cuda)             # never read: the launcher refuses first
    index = _graph(ops, c, cuda)
    out = torch.full((V, D), SENTINEL, device=cuda)
    with pytest.raises(pkg._lib.GGNNError, match="up to 256"):
        ops.gather_segment_sum_attn(H, h, index, f, nin, None, True, out=out)
    dh = torch.full((V, D), SENTINEL, device=cuda)
    with pytest.raises(pkg._lib.GGNNError, match="up to 256"):
        ops.attn_backward_target(H.view(-1, D), h, d, index, f, dh)
    torch.cuda.synchronize()
    assert (_np(out) == SENTINEL).all() and (_np(dh) == SENTINEL).all()


def test_rnn_refuses_hidden_size_36(pkg, ops, cuda):
    D, V, nx = 36, 17, 1
    rng = np.random.default_rng(36)
    x, h = (_dev(rng.normal(size=(V, D)).astype(np.float32), cuda) for _ in range(2))
    W = _dev(rng.normal(size=(2 * D, D)).astype(np.float32), cuda)
    b = torch.zeros(D, device=cuda)
    with pytest.raises(pkg._lib.GGNNError, match="unsupported"):
        ops.rnn([x], h, W, b, "tanh")
    out = torch.full((V, D), SENTINEL, device=cuda)      # ops.rnn allocates its own output: the same entry point on a sentinel
    segs = (ctypes.c_void_p * nx)(x.data_ptr())
    rc = pkg._lib.load().ggnn_rnn_f32(segs, nx, h.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), V, D, ops.ACT_IDS["tanh"],
                                      torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    torch.cuda.synchronize()
    assert (_np(out) == SENTINEL).all()
