"""The two kernels of csrc/ggnn_attn_compact.hip -- propagation attention over the rows of the compacted transform -- called
directly and held to the float64 formulas and a-priori bounds of tests/variant_kernel_ref.py at factor 2, per element: the
same inputs, shapes and switches as the dense-row kernels' tests (tests/test_gpu_variant_kernels.py).

The graph of ref.build_graph has a 70-message hub (the slots beyond the eight whose scores stay in registers), a tripled
(src, type) pair (several slots share one compact row), an empty edge type, self-loops, a node that receives nothing, and
V = 1 / 17 / 33 leave dead sub-waves at every sub-wave width.  The kernel under test never sees the dense tensor: Hc is a copy of
the active rows.  tests/test_variant_kernel_ref_host.py shows that float32 stays inside factor 1 of these bounds on these inputs.
"""
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
    """H [V, T*D] float32 on the device, as tests/test_gpu_variant_kernels._transform builds it."""
    V, D = c["h"].shape
    if D % 32 and D % 100:
        return _dev(ref.transform_rows(c["h"], c["W"], np.float32).reshape(V, -1), cuda)
    return ops.msg_transform(h, W)


def _graph(ops, c, cuda):
    V = c["h"].shape[0]
    return ops.build_message_index([_dev(a, cuda) for a in c["adj"]], V)


def _compact(ops, index, H, D):
    """(comp, Hc): the batch's active (node, type) pairs and a COPY of their rows of H, type-major / node-ascending."""
    V, T = index.num_nodes, index.num_edge_types
    comp = ops.build_compact_sources(index)
    R = comp.num_rows
    counts = [comp.type_row_off[t + 1] - comp.type_row_off[t] for t in range(T)]
    type_of_row = torch.repeat_interleave(torch.arange(T, device=H.device), torch.tensor(counts, device=H.device))
    Hc = H.view(V * T, D)[comp.pair_node[:R].long() * T + type_of_row].contiguous()
    assert Hc.shape == (R, D) and Hc.data_ptr() != H.data_ptr()
    return comp, Hc


def _case(ops, cuda, D, V, T, seed, saturate=False):
    c = ref.attn_inputs(D, V, T, seed, saturate=saturate)
    t = {k: _dev(c[k], cuda) for k in ("h", "W", "factors", "nin", "bias", "d")}
    index = _graph(ops, c, cuda)
    H = _transform(ops, c, t["h"], t["W"], cuda)
    comp, Hc = _compact(ops, index, H, D)
    Hrows = _np(H).reshape(V * T, D)
    del H
    return c, t, index, comp, Hc, Hrows


@pytest.mark.parametrize("T", ref.ATTN_T)
@pytest.mark.parametrize("V", ref.ATTN_V)
@pytest.mark.parametrize("D", ref.ATTN_D)
def test_attention_compact_forward(ops, cuda, D, V, T):
    c, t, index, comp, Hc, Hrows = _case(ops, cuda, D, V, T, ref.seed_of("attn", D, V, T))
    info = c["info"]
    if V > 1:       # the tripled (src, type) pair: three slots, one compact row
        slot_rows = _np(comp.gather_row)[_np(index.gather_row) == info["tripled"][0] * T + info["tripled"][2]]
        assert len(slot_rows) >= 3 and len(set(slot_rows.tolist())) == 1
    for bias_on, use_avg in ref.ATTN_SWITCHES:
        bias = t["bias"] if bias_on else None
        out = ops.gather_segment_sum_attn_compact(Hc, t["h"], index, comp, t["factors"], t["nin"], bias, use_avg)
        again = ops.gather_segment_sum_attn_compact(Hc, t["h"], index, comp, t["factors"], t["nin"], bias, use_avg)
        assert torch.equal(out, again), "two calls differ"
        a = (c["h"], Hrows, c["adj"], c["factors"], c["nin"], c["bias"] if bias_on else None, use_avg)
        ref.assert_within(_np(out), ref.attn_forward(*a), ref.attn_forward_bound(*a), FACTOR,
                          "attn_compact_forward.D%d[V=%d T=%d bias=%d avg=%d]" % (D, V, T, bias_on, use_avg))
        if V > 1 and not bias_on:
            assert not _np(out)[0].any(), "node 0 receives nothing: its row must be exactly zero"


def test_attention_compact_forward_saturated(ops, cuda):
    """Scores far beyond what exp() of an unshifted score survives in float32 (the case of test_attention_forward_saturated)."""
    D, V, T = 64, 17, 3
    c, t, index, comp, Hc, Hrows = _case(ops, cuda, D, V, T, ref.seed_of("saturated"), saturate=True)
    src, dst, typ, p, s, m, S, a_ = ref._softmax(c["h"], c["adj"], c["factors"], np.float64)
    hub = s[dst == V - 1]
    assert hub.max() - hub.min() > 90 and hub.max() > 89
    out = _np(ops.gather_segment_sum_attn_compact(Hc, t["h"], index, comp, t["factors"], t["nin"], None, False))
    assert np.isfinite(out).all()
    a = (c["h"], Hrows, c["adj"], c["factors"], c["nin"], None, False)
    ref.assert_within(out, ref.attn_forward(*a), ref.attn_forward_bound(*a), FACTOR, "attn_compact_forward.saturated")


@pytest.mark.parametrize("T", ref.ATTN_T)
@pytest.mark.parametrize("V", ref.ATTN_V)
@pytest.mark.parametrize("D", ref.ATTN_D)
def test_attention_compact_backward(ops, cuda, D, V, T):
    """The attention launches of variants._hip_backward on the compacted route, launch for launch, dh prefilled."""
    c, t, index, comp, Hc, Hrows = _case(ops, cuda, D, V, T, ref.seed_of("attn", D, V, T))
    assert index.num_messages
    index._compact = comp
    dh = _dev(c["dh0"], cuda)                              # prefilled: both passes must add to it
    coef_a, coef_s, dfac = ops.attn_backward_target_compact(Hc, t["h"], t["d"], index, comp, t["factors"], dh)
    dattn = ops.range_sum(dfac, index.type_off)
    bwd = ops.compact_backward(index, comp)
    ops.weighted_segment_sum(t["h"], bwd.source_node_index, bwd.source_node_index.msg, coef_s, out=dh, accumulate=True)
    a = (c["h"], Hrows, c["d"], c["adj"], c["factors"])
    want, B = ref.attn_backward(*a), ref.attn_backward_bounds(*a, dh_prefill=c["dh0"])
    tag = "[V=%d T=%d]" % (V, T)
    ref.assert_within(_np(coef_a), want["coef_a"], B["coef_a"], FACTOR, "attn_compact_backward.coef_a.D%d%s" % (D, tag))
    ref.assert_within(_np(coef_s), want["coef_s"], B["coef_s"], FACTOR, "attn_compact_backward.coef_s.D%d%s" % (D, tag))
    ref.assert_within(_np(dattn), want["dfactor"], B["dfactor"], FACTOR, "attn_compact_backward.dfactor.D%d%s" % (D, tag))
    ref.assert_within(_np(dh), c["dh0"].astype(np.float64) + want["dh_target"] + want["dh_source"], B["dh"], FACTOR,
                      "attn_compact_backward.dh.D%d%s" % (D, tag))
    if c["info"]["empty_type"] is not None:
        assert _np(dattn)[c["info"]["empty_type"]] == 0.0, "d factor of the empty edge type must be exactly 0"


def test_attention_compact_without_messages(ops, cuda):
    """M = 0: the forward gives exact zeros (bias rows of a node without incoming edges are zero too), the backward leaves dh alone."""
    D, V, T = 100, 17, 3
    c = ref.attn_inputs(D, V, T, ref.seed_of("empty"))
    h, f, d = (_dev(c[k], cuda) for k in ("h", "factors", "d"))
    index = ops.build_message_index([torch.zeros((0, 2), dtype=torch.int32, device=cuda) for _ in range(T)], V)
    assert index.num_messages == 0
    comp = ops.CompactSources(torch.zeros(1, dtype=torch.int32, device=cuda), [0] * (T + 1),
                              torch.zeros(0, dtype=torch.int32, device=cuda))
    Hc = torch.full((1, D), SENTINEL, device=cuda)         # no slot refers to it
    nin = torch.zeros((V, T), device=cuda)
    out = ops.gather_segment_sum_attn_compact(Hc, h, index, comp, f, nin, _dev(c["bias"], cuda), True)
    assert not _np(out).any()
    dh = _dev(c["dh0"], cuda)
    ops.attn_backward_target_compact(Hc, h, d, index, comp, f, dh)
    np.testing.assert_array_equal(_np(dh), c["dh0"])


def test_attention_compact_refuses_hidden_size_260(pkg, ops, cuda):
    """The launchers return before any kernel launch: the outputs stay as they were."""
    D, V, T = 260, 17, 3
    c = ref.attn_inputs(D, V, T, ref.seed_of("refuse"))
    h, f, nin, d = (_dev(c[k], cuda) for k in ("h", "factors", "nin", "d"))
    index = _graph(ops, c, cuda)
    comp = ops.build_compact_sources(index)
    Hc = torch.zeros((comp.num_rows, D), device=cuda)      # never read: the launcher refuses first
    out = torch.full((V, D), SENTINEL, device=cuda)
    with pytest.raises(pkg._lib.GGNNError, match="up to 256"):
        ops.gather_segment_sum_attn_compact(Hc, h, index, comp, f, nin, None, True, out=out)
    dh = torch.full((V, D), SENTINEL, device=cuda)
    with pytest.raises(pkg._lib.GGNNError, match="up to 256"):
        ops.attn_backward_target_compact(Hc, h, d, index, comp, f, dh)
    torch.cuda.synchronize()
    assert (_np(out) == SENTINEL).all() and (_np(dh) == SENTINEL).all()
