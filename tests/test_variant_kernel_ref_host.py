"""tests/variant_kernel_ref.py held to account on the CPU, before any kernel is compared with it:

  independence   its float64 formulas equal oracle/ggnn_oracle_torch.py (a separate restatement) and torch autograd of it;
  soundness      a float32 evaluation of every formula, on exactly the inputs tests/test_gpu_variant_kernels.py feeds the kernels,
                 stays inside the a-priori bound at factor 1 -- the condition that keeps the GPU test from failing a correct kernel;
  teeth          one dropped hub message, two swapped per-message entries, a `+=` turned `=` on one row, a zeroed last column
                 group, one element off by 1e-3: each is far outside factor 2.  The element scaled by 1 + 1e-3 is, for every
                 operation, the best-conditioned one (largest |reference| / bound, see _off_by_1e3).  d factor is the one
                 result this comparison holds only loosely: see test_teeth_attention_backward.
"""
import numpy as np
import pytest
import torch

import variant_kernel_ref as ref

F64 = torch.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64)


def _close(got, want, tol, what):
    """Element-wise: |got - want| <= tol (1 + |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    if want.size:
        excess = np.abs(got - want) / (1.0 + np.abs(want))
        assert excess.max() <= tol, "%s: error %.3e (relative to 1 + |reference|) at %s" % (
            what, excess.max(), np.unravel_index(int(excess.argmax()), want.shape))


# ---- independence -------------------------------------------------------------------------------------------------------------
def _identity_cell(D):
    """BasicRNNCell weights that pass the aggregated messages through: [x | h] [I; 0] + 0, with the identity as activation."""
    return {"W": torch.cat([torch.eye(D, dtype=F64), torch.zeros(D, D, dtype=F64)]), "b": torch.zeros(D, dtype=F64)}


@pytest.mark.parametrize("bias_on,use_avg", ref.ATTN_SWITCHES)
@pytest.mark.parametrize("V,D,T", [(1, 32, 1), (17, 64, 3), (33, 100, 4)])
def test_attention_matches_oracle_and_its_autograd(oracle_torch, V, D, T, bias_on, use_avg):
    c = ref.attn_inputs(D, V, T, ref.seed_of("indep", V, D, T))
    h, W, f, nin, bias = (_t(c[k]) for k in ("h", "W", "factors", "nin", "bias"))
    h.requires_grad_(True); W.requires_grad_(True); f.requires_grad_(True)
    adj = [torch.from_numpy(a.astype(np.int64)) for a in c["adj"]]
    out = oracle_torch.sparse_step(h, adj, nin, W, _identity_cell(D), (), bias if bias_on else None, use_avg, lambda x: x, "rnn", f)
    H64 = ref.transform_rows(c["h"], c["W"])
    mine = ref.attn_forward(c["h"], H64, c["adj"], c["factors"], c["nin"], c["bias"] if bias_on else None, use_avg)
    _close(mine, out.detach().numpy(), 1e-12, "attention forward")

    G = _t(c["d"])
    dh, dW, df = torch.autograd.grad(out, [h, W, f], G)
    d = c["d"].astype(np.float64)                            # dL / d(sum_e a_e H[g_e]): the bias passes, the mean divides
    if use_avg:
        d = d / (c["nin"].astype(np.float64).sum(-1, keepdims=True) + ref.SMALL)
    b = ref.attn_backward(c["h"], H64, d, c["adj"], c["factors"])
    src, dst, typ = ref.messages(c["adj"])
    dH = np.zeros((V * T, D))
    np.add.at(dH, src * T + typ, b["coef_a"][:, None] * d[dst])                    # d H[g_e] += a_e d[v]
    dH = dH.reshape(V, T, D)
    W64 = c["W"].astype(np.float64)
    dh_mine = b["dh_target"] + b["dh_source"] + np.einsum("vte,tde->vd", dH, W64)
    _close(dh_mine, dh.numpy(), 1e-10, "d h (target + source side + through H)")
    _close(np.einsum("vd,vte->tde", c["h"].astype(np.float64), dH), dW.numpy(), 1e-10, "d W (through d H = coef_a d)")
    _close(b["dfactor"], df.numpy(), 1e-10, "d factor")
    if c["info"]["empty_type"] is not None:
        assert b["dfactor"][c["info"]["empty_type"]] == 0.0


def _cell_case(D, V, nx, seed):
    c = ref.cell_inputs(D, V, nx, seed)
    rng = np.random.default_rng(seed + 7)
    c["g"] = rng.normal(size=(V, D)).astype(np.float32)
    c["nin"] = rng.integers(0, 4, (V, 3)).astype(np.float32)
    c["nin"][0] = 0.0                                      # a node without incoming edges: the mean divides by 1e-7 ...
    c["xs"][-1][0] *= 1e-7                                 # ... so its sum of messages is tiny too (it is: there are none)
    return c


def _cell_leaves(c, use_avg):
    """x_last = agg / (deg + 1e-7) with agg the leaf: the gradient of agg is what the kernels call dinc."""
    res = [_t(x).requires_grad_(True) for x in c["xs"][:-1]]
    agg = _t(c["xs"][-1]).requires_grad_(True)
    h = _t(c["h"]).requires_grad_(True)
    deg = _t(c["nin"]).sum(-1, keepdim=True) + ref.SMALL
    x = torch.cat(res + [agg / deg if use_avg else agg], dim=1)
    # the forward value the cells see as their last input
    xs = c["xs"][:-1] + [((c["xs"][-1].astype(np.float64)) / deg.numpy()) if use_avg else c["xs"][-1]]
    return res, agg, h, x, xs


@pytest.mark.parametrize("use_avg", [False, True])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("nx", [1, 3])
def test_rnn_cell_matches_oracle_and_its_autograd(oracle_torch, nx, activation, use_avg):
    D, V = 32, 9
    c = _cell_case(D, V, nx, ref.seed_of("rnn", nx, activation))
    res, agg, h, x, xs = _cell_leaves(c, use_avg)
    out = oracle_torch.rnn_cell(x, h, {"W": _t(c["W"]), "b": _t(c["b"])}, "rnn", oracle_torch._act(activation))
    mine = ref.rnn(xs, c["h"], c["W"], c["b"], activation)
    _close(mine, out.detach().numpy(), 1e-12, "rnn forward")
    grads = torch.autograd.grad(out, res + [agg, h], _t(c["g"]))
    dP = ref.act_bwd(c["g"], mine, activation)
    dx0 = np.zeros((V, nx * D))
    dx, dinc, dh = ref.bwd_dx(dP, 1, c["W"].astype(np.float64).T, nx * D, True, dx0 if nx > 1 else None, c["nin"], use_avg, None,
                              False, False, D)
    for i in range(nx - 1):
        _close(dx[:, i * D:(i + 1) * D], grads[i].numpy(), 1e-10, "d residual %d" % i)
    _close(dinc, grads[nx - 1].numpy(), 1e-10, "d incoming")
    _close(dh, grads[nx].numpy(), 1e-10, "d h")


@pytest.mark.parametrize("use_avg", [False, True])
@pytest.mark.parametrize("nx", [1, 3])
def test_cudnn_gru_cell_matches_oracle_and_its_autograd(oracle_torch, nx, use_avg):
    D, V = 32, 9
    c = _cell_case(D, V, nx, ref.seed_of("cudnn", nx))
    res, agg, h, x, xs = _cell_leaves(c, use_avg)
    cud = c["cudnn"]
    out = oracle_torch.rnn_cell(x, h, {k: _t(v) for k, v in cud.items()}, "cudnncompatiblegrucell", torch.tanh)
    mine, r, u, cc, hc = ref.cudnn_gru(xs, c["h"], **cud)
    _close(mine, out.detach().numpy(), 1e-12, "cudnn-GRU forward")
    grads = torch.autograd.grad(out, res + [agg, h], _t(c["g"]))
    # the composition of variants._hip_backward: stage, then the three products
    dpc, dpg, dh, dhc = ref.cudnn_bwd_stage(c["g"], c["h"], r, u, cc, hc)
    T64 = lambda w: w.astype(np.float64).T
    dx, _, _ = ref.bwd_dx(dpc, 1, T64(cud["Wcx"]), nx * D, False, np.zeros((V, nx * D)), None, False, None, False, False, D)
    _, _, dh = ref.bwd_dx(dhc, 1, T64(cud["Wch"]), 0, False, None, None, False, dh, False, True, D)
    dx, dinc, dh = ref.bwd_dx(dpg, 2, T64(cud["Wg"]), nx * D, True, dx, c["nin"], use_avg, dh, True, True, D)
    for i in range(nx - 1):
        _close(dx[:, i * D:(i + 1) * D], grads[i].numpy(), 1e-10, "d residual %d" % i)
    _close(dinc, grads[nx - 1].numpy(), 1e-10, "d incoming")
    _close(dh, grads[nx].numpy(), 1e-10, "d h")


@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_gru_backward_stages_match_autograd_of_the_oracle(oracle_torch, activation):
    """stage 1 -> drh = (dpc Wc^T)[:, h block] -> stage 2 -> the two dX products (backward._backward_dense_form)."""
    D, V, nx = 32, 9, 2
    c = _cell_case(D, V, nx, ref.seed_of("gru", activation))
    rng = np.random.default_rng(3)
    K = (nx + 1) * D
    Wg, Wc = rng.normal(size=(K, 2 * D)) / np.sqrt(K), rng.normal(size=(K, D)) / np.sqrt(K)
    bg, bc = rng.normal(size=2 * D) * 0.2, rng.normal(size=D) * 0.2
    xs = [_t(x).requires_grad_(True) for x in c["xs"]]
    h = _t(c["h"]).requires_grad_(True)
    out = oracle_torch.gru(torch.cat(xs, 1), h, _t(Wg), _t(bg), _t(Wc), _t(bc), oracle_torch._act(activation))
    grads = torch.autograd.grad(out, xs + [h], _t(c["g"]))
    x64, h64 = np.concatenate(c["xs"], 1).astype(np.float64), c["h"].astype(np.float64)
    gates = 1 / (1 + np.exp(-(np.concatenate([x64, h64], 1) @ Wg + bg)))
    r, u = gates[:, :D], gates[:, D:]
    pre = np.concatenate([x64, r * h64], 1) @ Wc + bc
    cand = np.tanh(pre) if activation == "tanh" else np.maximum(pre, 0)
    dpc, dpu, dh, rh = ref.gru_bwd_stage1(c["g"], c["h"], r, u, cand, activation)
    _close(rh, r * h64, 1e-15, "r h")
    Qc = dpc @ Wc.T
    dh, dpr = ref.gru_bwd_stage2(Qc[:, nx * D:], c["h"], r, dh)
    Qg = np.concatenate([dpr, dpu], 1) @ Wg.T
    for i in range(nx):
        _close((Qc + Qg)[:, i * D:(i + 1) * D], grads[i].numpy(), 1e-10, "d x %d" % i)
    _close(dh + Qg[:, nx * D:], grads[nx].numpy(), 1e-10, "d h")


def test_graph_builder_features():
    for V, T in [(1, 1), (1, 4), (17, 3), (33, 4), (17, 1)]:
        adj, nin, info = ref.build_graph(V, T, 5)
        src, dst, typ = ref.messages(adj)
        assert len(adj) == T and all(a.dtype == np.int32 and a.shape[1] == 2 for a in adj)
        assert int((dst == V - 1).sum()) == ref.HUB_IN and nin[V - 1].sum() == ref.HUB_IN
        live = [t for t in range(T) if t != info["empty_type"]]
        assert all(((dst == V - 1) & (typ == t)).any() for t in live)                 # the hub's messages: every populated type
        s, d, t = info["tripled"]
        assert int(((src == s) & (dst == d) & (typ == t)).sum()) >= 3
        assert ((src == V - 1) & (dst == V - 1)).any()
        if T >= 3:
            assert len(adj[1]) == 0 and (nin[:, 1] == 0).all()
        if V > 1:
            assert not (dst == 0).any() and ((src == 2) & (dst == 2)).any()
            assert int(((src == s) & (dst == d) & (typ == t)).sum()) == 3
            assert any((np.diff(a[:, 1]) < 0).any() for a in adj if len(a) > 1)         # not in target order
        else:
            assert (src == 0).all() and (dst == 0).all()
        np.testing.assert_array_equal(nin.sum(0), [len(a) for a in adj])


# ---- soundness: float32 on the CPU stays inside factor 1 ----------------------------------------------------------------------
F32 = np.float32


@pytest.mark.parametrize("T", ref.ATTN_T)
@pytest.mark.parametrize("V", ref.ATTN_V)
@pytest.mark.parametrize("D", ref.ATTN_D)
def test_f32_attention_within_bound(D, V, T):
    c = ref.attn_inputs(D, V, T, ref.seed_of("attn", D, V, T))
    H = ref.transform_rows(c["h"], c["W"], F32)                                      # one float32 H for both evaluations
    for bias_on, use_avg in ref.ATTN_SWITCHES:
        a = (c["h"], H, c["adj"], c["factors"], c["nin"], c["bias"] if bias_on else None, use_avg)
        ref.assert_within(ref.attn_forward(*a, dt=F32), ref.attn_forward(*a), ref.attn_forward_bound(*a), 1,
                          "attn_forward.D%d[V=%d T=%d bias=%d avg=%d]" % (D, V, T, bias_on, use_avg))
    a = (c["h"], H, c["d"], c["adj"], c["factors"])
    got, want, B = ref.attn_backward(*a, dt=F32), ref.attn_backward(*a), ref.attn_backward_bounds(*a, dh_prefill=c["dh0"])
    tag = "[V=%d T=%d]" % (V, T)
    ref.assert_within(got["coef_a"], want["coef_a"], B["coef_a"], 1, "attn_backward.coef_a.D%d%s" % (D, tag))
    ref.assert_within(got["coef_s"], want["coef_s"], B["coef_s"], 1, "attn_backward.coef_s.D%d%s" % (D, tag))
    ref.assert_within(got["dfactor"], want["dfactor"], B["dfactor"], 1, "attn_backward.dfactor.D%d%s" % (D, tag))
    dh32 = c["dh0"] + got["dh_target"] + got["dh_source"]
    ref.assert_within(dh32, c["dh0"].astype(np.float64) + want["dh_target"] + want["dh_source"], B["dh"], 1,
                      "attn_backward.dh.D%d%s" % (D, tag))


def test_f32_saturated_attention_within_bound():
    c = ref.attn_inputs(64, 17, 3, ref.seed_of("saturated"), saturate=True)
    H = ref.transform_rows(c["h"], c["W"], F32)
    a = (c["h"], H, c["adj"], c["factors"], c["nin"], None, False)
    out = ref.attn_forward(*a, dt=F32)
    assert np.isfinite(out).all()
    ref.assert_within(out, ref.attn_forward(*a), ref.attn_forward_bound(*a), 1, "attn_forward.saturated")


@pytest.mark.parametrize("nseg", ref.WSS_NSEG)
@pytest.mark.parametrize("D", ref.WSS_D)
def test_f32_weighted_segment_sum_within_bound(D, nseg):
    c = ref.wss_inputs(D, nseg, ref.seed_of("wss", D, nseg))
    for acc in (False, True):
        a = (c["rows"], c["row_ptr"], c["gather_row"], c["weight_id"], c["weights"], c["out0"] if acc else None)
        ref.assert_within(ref.weighted_segment_sum(*a, dt=F32), ref.weighted_segment_sum(*a), ref.weighted_segment_sum_bound(*a), 1,
                          "weighted_segment_sum.%s[D=%d nseg=%d acc=%d]" % ("strided" if D > 256 else "direct", D, nseg, acc))


def test_f32_range_sum_within_bound():
    for name, (v, off) in (("lengths", ref.range_inputs(ref.seed_of("range"))), ("64", ref.range_inputs_64(ref.seed_of("range64")))):
        ref.assert_within(ref.range_sum(v, off, dt=F32), ref.range_sum(v, off), ref.range_sum_bound(v, off), 1, "range_sum." + name)


@pytest.mark.parametrize("V", ref.CELL_V)
@pytest.mark.parametrize("D", ref.CELL_D)
def test_f32_cells_within_bound(D, V):
    for nx in ref.CELL_NX:
        c = ref.cell_inputs(D, V, nx, ref.seed_of("cell", D, V, nx))
        tag = "[V=%d nx=%d]" % (V, nx)
        for act in ("tanh", "relu"):
            a = (c["xs"], c["h"], c["W"], c["b"], act)
            ref.assert_within(ref.rnn(*a, dt=F32), ref.rnn(*a), ref.rnn_bound(*a), 1, "rnn.%s.D%d%s" % (act, D, tag))
        got = ref.cudnn_gru(c["xs"], c["h"], **c["cudnn"], dt=F32)
        want = ref.cudnn_gru(c["xs"], c["h"], **c["cudnn"])
        B = ref.cudnn_gru_bounds(c["xs"], c["h"], **c["cudnn"])
        for name, g, w, b in zip(("out", "r", "u", "c", "hc"), got, want, B):
            ref.assert_within(g, w, b, 1, "cudnn_gru.%s.D%d%s" % (name, D, tag))


@pytest.mark.parametrize("shape", ref.BWD_DX_SHAPES)
@pytest.mark.parametrize("D", ref.BWD_DX_D)
def test_f32_bwd_dx_within_bound(D, shape):
    for V in ref.BWD_DX_V:
        for nx in ref.BWD_DX_NX:
            c = ref.bwd_dx_inputs(shape, D, V, nx, ref.seed_of("bwd_dx", shape, D, V, nx))
            a = ref.bwd_dx_args(c)
            got, want, B = ref.bwd_dx(*a, dt=F32), ref.bwd_dx(*a), ref.bwd_dx_bounds(*a)
            for name, g, w, b in zip(("dx", "dinc", "dh"), got, want, B):
                assert (g is None) == (w is None) == (b is None)
                if w is not None:
                    ref.assert_within(g, w, b, 1, "bwd_dx.%s.%s.D%d[V=%d nx=%d]" % (shape, name, D, V, nx))


@pytest.mark.parametrize("V,D", ref.ELEMENTWISE_SHAPES)
def test_f32_elementwise_stages_within_bound(V, D):
    c = ref.elementwise_inputs(V, D, ref.seed_of("elementwise", V, D))
    for act, out in (("tanh", c["c"]), ("relu", c["c_relu"])):
        ref.assert_within(ref.act_bwd(c["g"], out, act, dt=F32), ref.act_bwd(c["g"], out, act), ref.act_bwd_bound(c["g"], out, act), 1,
                          "act_bwd." + act)
        a = (c["g"], c["h"], c["r"], c["u"], out, act)
        for name, g, w, b in zip(("dpc", "dpu", "dh", "rh"), ref.gru_bwd_stage1(*a, dt=F32), ref.gru_bwd_stage1(*a),
                                 ref.gru_bwd_stage1_bounds(*a)):
            ref.assert_within(g, w, b, 1, "gru_bwd_stage1.%s.%s" % (act, name))
    a = (c["g"], c["h"], c["r"], c["u"], c["c"], c["hc"])
    for name, g, w, b in zip(("dpc", "dpg", "dh", "dhc"), ref.cudnn_bwd_stage(*a, dt=F32), ref.cudnn_bwd_stage(*a),
                             ref.cudnn_bwd_stage_bounds(*a)):
        ref.assert_within(g, w, b, 1, "cudnn_gru_bwd_stage." + name)
    a = (c["drh"], c["h"], c["r"], c["dh0"])
    for name, g, w, b in zip(("dh", "dpr"), ref.gru_bwd_stage2(*a, dt=F32), ref.gru_bwd_stage2(*a), ref.gru_bwd_stage2_bounds(*a)):
        ref.assert_within(g, w, b, 1, "gru_bwd_stage2." + name)


def test_f32_empty_graph_step_within_bound():
    D, V = 100, 17
    c = ref.attn_inputs(D, V, 3, ref.seed_of("empty"))
    cell = ref.cell_inputs(D, V, 1, ref.seed_of("empty cell"))
    a = (c["h"], c["d"], cell["W"], cell["b"])
    got, want, B = ref.empty_graph_rnn_step(*a, dt=F32), ref.empty_graph_rnn_step(*a), ref.empty_graph_rnn_step_bounds(*a)
    ref.assert_within(got[0], want[0], B[0], 1, "empty_graph.rnn_out")
    ref.assert_within(got[1], want[1], B[1], 1, "empty_graph.dh")
    _raises(_off_by_1e3(want[1], B[1]), want[1], B[1], "empty graph dh off by 1e-3")
    _raises(_zero_last_columns(want[1], 4), want[1], B[1], "empty graph dh: last column group zeroed")


# ---- teeth --------------------------------------------------------------------------------------------------------------------
def _raises(got, want, bound, what):
    with pytest.raises(AssertionError, match="outside 2 x bound"):
        ref.assert_within(got, want, bound, 2, what)


def _off_by_1e3(want, bound):
    """The reference with one element scaled by 1 + 1e-3: the best-conditioned one (largest |reference| / bound).  Where a result
    is a sum that cancels, an a-priori bound follows the magnitudes summed, and a relative 1e-3 of the small result can hide."""
    got = np.array(want, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(got == 0.0, 0.0, np.abs(got) / np.broadcast_to(bound, got.shape))
    idx = np.unravel_index(int(np.argmax(cond)), got.shape)
    got[idx] *= 1 + 1e-3
    return got


def _zero_last_columns(want, n):
    got = np.array(want, dtype=np.float64)
    got[:, got.shape[1] - n:] = 0.0
    return got


def _drop_hub_message(c):
    """The case's adjacency lists without one of the hub's HUB_IN messages (nin untouched: the kernel's inputs did not change)."""
    hub = c["info"]["hub"]
    adj = [a.copy() for a in c["adj"]]
    for t, a in enumerate(adj):
        k = np.nonzero((a[:, 1] == hub) & (a[:, 0] != hub))[0]
        if len(k):
            adj[t] = np.delete(a, k[0], axis=0)
            return adj
    raise AssertionError("no hub message")


@pytest.mark.parametrize("V,D,T", [(17, 100, 3), (33, 256, 4), (1, 32, 1)])
def test_teeth_attention_forward(V, D, T):
    c = ref.attn_inputs(D, V, T, ref.seed_of("attn", D, V, T))
    H = ref.transform_rows(c["h"], c["W"], F32)
    a = (c["h"], H, c["adj"], c["factors"], c["nin"], c["bias"], True)
    want, B = ref.attn_forward(*a), ref.attn_forward_bound(*a)
    if V > 1:                                              # (V = 1: the 70 messages are one self-loop repeated, all alike)
        _raises(ref.attn_forward(c["h"], H, _drop_hub_message(c), *a[3:]), want, B, "dropped hub message")
    _raises(_off_by_1e3(want, B), want, B, "one element off by 1e-3")
    _raises(_zero_last_columns(want, 4), want, B, "last column group zeroed")
    if V > 1:
        got = want.copy()
        got[[V - 1, V - 2]] = got[[V - 2, V - 1]]                                     # a dead sub-wave's clamp gone wrong
        _raises(got, want, B, "hub row written to its neighbour")


@pytest.mark.parametrize("V,D,T", [(17, 100, 3), (33, 256, 4)])
def test_teeth_attention_backward(V, D, T):
    c = ref.attn_inputs(D, V, T, ref.seed_of("attn", D, V, T))
    H = ref.transform_rows(c["h"], c["W"], F32)
    a = (c["h"], H, c["d"], c["adj"], c["factors"])
    want, B = ref.attn_backward(*a), ref.attn_backward_bounds(*a, dh_prefill=c["dh0"])
    src, dst, typ = ref.messages(c["adj"])
    hub_msgs = np.nonzero(dst == V - 1)[0]
    for name in ("coef_a", "coef_s"):                                                 # a wrong msg_perm: two message ids swapped
        got = want[name].copy()
        i, j = hub_msgs[0], hub_msgs[-1]
        assert abs(got[i] - got[j]) > 1e-3 * max(abs(got[i]), abs(got[j]))
        got[[i, j]] = got[[j, i]]
        _raises(got, want[name], B[name], name + " swapped")
        _raises(_off_by_1e3(want[name], B[name]), want[name], B[name], name + " off by 1e-3")
    dropped = ref.attn_backward(c["h"], H, c["d"], _drop_hub_message(c), c["factors"])
    dh = c["dh0"].astype(np.float64) + want["dh_target"] + want["dh_source"]
    _raises(c["dh0"] + dropped["dh_target"] + dropped["dh_source"], dh, B["dh"], "dh: dropped hub message")
    got = dh.copy()
    got[V - 1] -= c["dh0"][V - 1]                                                     # `=` instead of `+=` on the hub's row
    _raises(got, dh, B["dh"], "dh: = instead of += on one row")
    got = dh.copy()
    got[3] -= want["dh_source"][3]                                                    # the source-side pass overwrote instead of adding
    _raises(got + 0, dh, B["dh"], "dh: source side missing on one row")
    _raises(_off_by_1e3(dh, B["dh"]), dh, B["dh"], "dh off by 1e-3")
    _raises(_zero_last_columns(dh, 4), dh, B["dh"], "dh: last column group zeroed")
    # d factor sums |p| <= 8 times per-message terms that cancel, under the worst-case score perturbation 2 (D + 2) delta eps the
    # issue prescribes.  Over the cases of the GPU test its bound is 5e-4 to 3e-2 of |d factor| typically, 0.1 to 0.4 on
    # several types and above 1 at V = 1 (where the 70 equal scores make d factor cancel to ~0), while a float32 evaluation
    # sits 40 to 600 times inside it.  So this comparison checks d factor for the type mapping, a skipped sub-wave and gross
    # errors only: neither a relative 1e-3 nor one of the hub's 70 messages shows.  Finer errors of d factor are seen through
    # coef_s (same ds) and by test_variant_hip_backward_equals_autograd_of_torch_restatement (3e-4 of max |grad|).
    got = want["dfactor"].copy()
    got[[0, T - 1]] = got[[T - 1, 0]]
    _raises(got, want["dfactor"], B["dfactor"], "d factor: two types swapped")
    got = want["dfactor"].copy()
    np.subtract.at(got, typ[hub_msgs], want["dfac"][hub_msgs])
    _raises(got, want["dfactor"], B["dfactor"], "d factor: the hub's messages missing")


def test_teeth_sums():
    c = ref.wss_inputs(260, 17, ref.seed_of("wss", 260, 17))
    a = (c["rows"], c["row_ptr"], c["gather_row"], c["weight_id"], c["weights"], c["out0"])
    want, B = ref.weighted_segment_sum(*a), ref.weighted_segment_sum_bound(*a)
    got = want.copy()
    got[16] -= c["out0"][16]
    _raises(got, want, B, "= instead of += on the 70-slot segment")
    got = want.copy()
    got[16] -= float(c["weights"][c["weight_id"][-1]]) * c["rows"][c["gather_row"][-1]]
    _raises(got, want, B, "last slot dropped")
    _raises(_zero_last_columns(want, 4), want, B, "strided column tail zeroed")
    _raises(_off_by_1e3(want, B), want, B, "off by 1e-3")
    v, off = ref.range_inputs(ref.seed_of("range"))
    want, B = ref.range_sum(v, off), ref.range_sum_bound(v, off)
    assert want[0] == 0.0 and B[0] == 0.0
    got = want.copy()
    got[4] -= float(v[off[5] - 1])                                                    # the 257th element of the 257-long range left out
    _raises(got, want, B, "range tail dropped")
    _raises(_off_by_1e3(want, B), want, B, "off by 1e-3")


def test_teeth_cells_and_bwd_dx():
    D, V, nx = 100, 129, 3
    c = ref.cell_inputs(D, V, nx, ref.seed_of("cell", D, V, nx))
    for act in ("tanh", "relu"):
        a = (c["xs"], c["h"], c["W"], c["b"], act)
        want, B = ref.rnn(*a), ref.rnn_bound(*a)
        _raises(_off_by_1e3(want, B), want, B, "rnn off by 1e-3")
        _raises(_zero_last_columns(want, 4), want, B, "rnn: last partial column group zeroed")
        got = ref.rnn(c["xs"][:-1] + [np.zeros_like(c["h"])], *a[1:])               # one K segment left out
        _raises(got, want, B, "rnn: a K segment dropped")
    want = ref.cudnn_gru(c["xs"], c["h"], **c["cudnn"])
    B = ref.cudnn_gru_bounds(c["xs"], c["h"], **c["cudnn"])
    for name, w, b in zip(("out", "r", "u", "c", "hc"), want, B):
        _raises(_off_by_1e3(w, b), w, b, "cudnn %s off by 1e-3" % name)
        _raises(_zero_last_columns(w, 4), w, b, "cudnn %s: last partial column group zeroed" % name)
    for shape in ref.BWD_DX_SHAPES:
        ci = ref.bwd_dx_inputs(shape, D, V, nx, ref.seed_of("bwd_dx", shape, D, V, nx))
        a = ref.bwd_dx_args(ci)
        want, B = ref.bwd_dx(*a), ref.bwd_dx_bounds(*a)
        for name, w, b, pre in zip(("dx", "dinc", "dh"), want, B, (ci["dx0"], None, ci["dh0"])):
            if w is None:
                continue
            _raises(_off_by_1e3(w, b), w, b, "%s %s off by 1e-3" % (shape, name))
            _raises(_zero_last_columns(w, 4), w, b, "%s %s: last column group zeroed" % (shape, name))
            if pre is not None and ((name == "dx" and ci["acc_dx"]) or (name == "dh" and ci["acc_dh"])):
                got = w.copy()
                got[V - 1, :D] -= pre[V - 1, :D]
                _raises(got, w, b, "%s %s: = instead of += on the last row" % (shape, name))
        if shape == "cudnn_c":                                                      # dinc = (dx + Q) / deg: the dx term left out
            got = want[1] - ci["dx0"][:, ci["xcols"] - D:] / (ci["nin"].sum(-1, keepdims=True) + ref.SMALL)
            _raises(got, want[1], B[1], "cudnn_c dinc without the dx term")
        if ci["use_avg"]:                                                           # the mean left out on the all-zero row
            got = want[1].copy()
            got[0] *= ref.SMALL
            _raises(got, want[1], B[1], "%s dinc: row 0 not divided" % shape)


def test_teeth_elementwise():
    V, D = 41, 100
    c = ref.elementwise_inputs(V, D, ref.seed_of("elementwise", V, D))
    want, B = ref.act_bwd(c["g"], c["c_relu"], "relu"), ref.act_bwd_bound(c["g"], c["c_relu"], "relu")
    got = want.copy()
    zero = np.nonzero((c["c_relu"].reshape(-1) == 0) & (c["g"].reshape(-1) != 0))[0][0]
    got.reshape(-1)[zero] = c["g"].reshape(-1)[zero]                                # relu'(0) taken as 1
    _raises(got, want, B, "relu'(+-0) = 1")
    a = (c["g"], c["h"], c["r"], c["u"], c["c"], c["hc"])
    for name, w, b in zip(("dpc", "dpg", "dh", "dhc"), ref.cudnn_bwd_stage(*a), ref.cudnn_bwd_stage_bounds(*a)):
        _raises(_off_by_1e3(w, b), w, b, "cudnn stage %s off by 1e-3" % name)
        got = w.copy()
        got.reshape(-1)[-4:] = 0.0                                                  # the last float4 of the tail
        _raises(got, w, b, "cudnn stage %s: last float4 missing" % name)
    def last_float4_missing(w):
        got = w.copy()
        got.reshape(-1)[-4:] = 0.0
        return got
    w, b = ref.act_bwd(c["g"], c["c"], "tanh"), ref.act_bwd_bound(c["g"], c["c"], "tanh")
    _raises(_off_by_1e3(w, b), w, b, "act_bwd tanh off by 1e-3")
    _raises(last_float4_missing(w), w, b, "act_bwd tanh: last float4 missing")
    _raises(c["g"] * (1 - c["c"].astype(np.float64)), w, b, "act_bwd tanh: 1 - out instead of 1 - out^2")
    for act, cand in (("tanh", c["c"]), ("relu", c["c_relu"])):
        a = (c["g"], c["h"], c["r"], c["u"], cand, act)
        for name, w, b in zip(("dpc", "dpu", "dh", "rh"), ref.gru_bwd_stage1(*a), ref.gru_bwd_stage1_bounds(*a)):
            _raises(_off_by_1e3(w, b), w, b, "stage 1 %s %s off by 1e-3" % (act, name))
            _raises(last_float4_missing(w), w, b, "stage 1 %s %s: last float4 missing" % (act, name))
            got = w.copy()
            got[[V - 1, V - 2]] = got[[V - 2, V - 1]]
            _raises(got, w, b, "stage 1 %s %s: last two rows swapped" % (act, name))
    dpc, Bdpc = ref.gru_bwd_stage1(*a)[0], ref.gru_bwd_stage1_bounds(*a)[0]       # (relu) act'(+-0) taken as 1
    got = dpc.copy()
    full = (c["g"].astype(np.float64) * (1 - c["u"].astype(np.float64))).reshape(-1)
    got.reshape(-1)[zero] = full[zero]
    _raises(got, dpc, Bdpc, "stage 1 relu'(+-0) = 1")
    a = (c["drh"], c["h"], c["r"], c["dh0"])
    (dh, dpr), (Bdh, Bdpr) = ref.gru_bwd_stage2(*a), ref.gru_bwd_stage2_bounds(*a)
    got = dh.copy()
    got[V - 1] -= c["dh0"][V - 1]
    _raises(got, dh, Bdh, "stage 2 dh: = instead of +=")
    _raises(_off_by_1e3(dpr, Bdpr), dpr, Bdpr, "stage 2 dpr off by 1e-3")
    _raises(_off_by_1e3(dh, Bdh), dh, Bdh, "stage 2 dh off by 1e-3")
    _raises(last_float4_missing(dpr), dpr, Bdpr, "stage 2 dpr: last float4 missing")
    _raises(last_float4_missing(dh), dh, Bdh, "stage 2 dh: last float4 missing")
