"""ggnn_attn_bwd_source_compact_f32 (ops.attn_backward_source_compact): the source side of the propagation-attention backward
(TF autodiff of chem_tensorflow_sparse.py:170-196) over the compacted rows, one launch for the two ggnn_weighted_segment_sum_f32
launches of variants._hip_backward -- dHc[row(u,t)] = sum coef_a * dinc[dst] over the (node, type) pair's messages and
dh[u] += sum coef_s * h[dst] over the node's.  Both outputs bit for bit against those two launches on hand-built and random message
lists at every sub-wave width, and at V = 2000 against float64 sums under the a-priori bound of tests/variant_kernel_ref.py."""
import numpy as np
import pytest
import torch

import variant_kernel_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 2                       # tests/test_gpu_variant_kernels.py
SENTINEL = -777.25
WIDTHS = (32, 64, 100, 128, 256)     # sub-waves of 16 (8 lanes idle / none), 32 (7 idle / none), 64 lanes


def _hand_built():
    """V = 17, T = 4: nodes 3, 9 and 16 send nothing; node 5 sends 11 messages (3 + 8 on two types: past the 4 slots the kernel holds
    in registers, the pair boundary inside the held ones and a pair running across the held / tail boundary); node 7 sends on all
    four types (exactly the held slots, every one a pair of its own); the message
    (2 -> 4, type 1) is listed twice; the lists are in no order of the source, so message ids permute the by-source slots."""
    adj = [[(12, 0), (7, 1), (5, 6), (0, 2), (5, 0), (5, 5), (1, 1)],
           [(2, 4), (7, 8), (2, 4), (14, 13), (6, 7)],
           [(15, 15), (5, 1), (5, 2), (7, 10), (5, 3), (5, 4), (5, 8), (5, 9), (5, 10), (5, 11), (4, 12), (8, 0)],
           [(13, 14), (7, 7), (11, 10), (10, 11)]]
    return 17, [np.asarray(a, np.int32).reshape(-1, 2) for a in adj]


def _random(V, T, seed):
    rng = np.random.default_rng(seed)
    adj = []
    for t in range(T):
        n = int(V * (0.4 + 0.5 * t))
        src = rng.integers(0, V, n)
        src = src[src % 11 != 3]                                   # nodes 3, 14, 25 .. send nothing
        src = np.concatenate([src, np.full(13 + t, 40 + t)])       # nodes 40 .. 43: a pair with more messages than are held
        dst = rng.integers(0, V, len(src))
        a = np.stack([src, dst], 1)
        adj.append(np.concatenate([a, a[:len(a) // 20]]).astype(np.int32))      # duplicates
    return V, adj


CASES = {"self_loop": lambda: (1, [np.asarray([[0, 0]], np.int32)]), "hand_built": _hand_built,
         "random_2000": lambda: _random(2000, 4, 7)}


@pytest.fixture(scope="module")
def graphs(pkg, cuda):
    """Per case: the index structures (built once, shared by every width) and NumPy copies for the float64 sums."""
    ops = pkg.ops
    out = {}
    for name, make in CASES.items():
        V, adj = make()
        index = ops.build_message_index([torch.from_numpy(a).to(cuda) for a in adj], V)
        comp = index._compact = ops.build_compact_sources(index)
        bwd = ops.compact_backward(index, comp)
        out[name] = (V, index, comp, bwd, ops.source_slot_rows(index, comp))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


def test_hand_built_graph_has_what_it_says(graphs):
    V, index, comp, bwd, slot_row = graphs["hand_built"]
    sni = bwd.source_node_index
    rp, msg, dst, rows = _np(sni.row_ptr), _np(sni.msg), _np(sni.gather_row), _np(slot_row)
    sent = np.diff(rp)
    assert V == 17 and index.num_edge_types == 4 and index.num_messages == 28 == sent.sum()
    assert sent[5] == 11 and not sent[[3, 9, 16]].any() and sent.max() == 11
    assert len(set(rows[rp[7]:rp[8]])) == 4                                       # node 7: four compact rows
    assert len(set(rows[rp[5]:rp[6]])) == 2 and rows[rp[5] + 2] != rows[rp[5] + 3] == rows[rp[5] + 4]    # across the held / tail boundary
    two = [(int(d), int(r)) for d, r in zip(dst[rp[2]:rp[3]], rows[rp[2]:rp[3]])]
    assert two == [(4, two[0][1])] * 2                                             # the duplicated message: one pair, twice
    assert sorted(msg.tolist()) == list(range(28)) and (msg != np.arange(28)).any()
    # slot_row is the compact row of the slot's (source, type) pair: rows_index lists the same slots row by row
    ri = bwd.rows_index
    by_row = sorted(zip(np.repeat(np.arange(comp.num_rows), np.diff(_np(ri.row_ptr))).tolist(), _np(ri.msg).tolist()))
    assert by_row == sorted(zip(rows.tolist(), msg.tolist()))


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("case", list(CASES))
def test_source_kernel_equals_the_two_launches(pkg, cuda, graphs, case, D):
    ops = pkg.ops
    V, index, comp, bwd, slot_row = graphs[case]
    M, R = index.num_messages, comp.num_rows
    rng = np.random.default_rng(1000 * D + V)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(cuda)
    dinc, h, dh0 = t(rng.standard_normal((V, D))), t(rng.standard_normal((V, D))), t(rng.standard_normal((V, D)))
    coef_a, coef_s = t(rng.uniform(0.0, 1.0, M)), t(rng.standard_normal(M))
    sni, ri = bwd.source_node_index, bwd.rows_index

    want_dHc = ops.weighted_segment_sum(dinc, ri, ri.msg, coef_a)
    want_dh = dh0.clone()
    ops.weighted_segment_sum(h, sni, sni.msg, coef_s, out=want_dh, accumulate=True)

    got_dh = dh0.clone()
    got_dHc = torch.full((R, D), SENTINEL, dtype=torch.float32, device=cuda)
    assert ops.attn_backward_source_compact(dinc, h, sni, slot_row, R, coef_a, coef_s, got_dh, out=got_dHc) is got_dHc
    assert torch.equal(got_dHc, want_dHc[:R]) and torch.equal(_bits(got_dHc), _bits(want_dHc[:R])), (case, D)
    assert torch.equal(got_dh, want_dh) and torch.equal(_bits(got_dh), _bits(want_dh)), (case, D)
    assert bool((got_dh != dh0).any()) and not bool((got_dHc == SENTINEL).any())
    # without dh (the first timestep of the first layer: h0 is data): the same dHc, nothing else written
    only = ops.attn_backward_source_compact(dinc, h, sni, slot_row, R, coef_a, coef_s, None)
    assert torch.equal(_bits(only[:R]), _bits(want_dHc[:R]))

    if case == "random_2000":
        n = lambda x: _np(x)
        a = (n(dinc), n(ri.row_ptr), n(ri.gather_row), n(ri.msg), n(coef_a), None)
        worst_a = ref.assert_within(n(got_dHc), ref.weighted_segment_sum(*a), ref.weighted_segment_sum_bound(*a), FACTOR,
                                    "attn_bwd_source_compact.dHc[D=%d]" % D)
        s = (n(h), n(sni.row_ptr), n(sni.gather_row), n(sni.msg), n(coef_s), n(dh0))
        worst_s = ref.assert_within(n(got_dh), ref.weighted_segment_sum(*s), ref.weighted_segment_sum_bound(*s), FACTOR,
                                    "attn_bwd_source_compact.dh[D=%d]" % D)
        print("D=%d: largest error / bound dHc %.3f, dh %.3f" % (D, worst_a, worst_s))
        sent = np.diff(n(sni.row_ptr))
        assert sent.max() > 8 and (sent == 0).any() and (sent == 4).any() and (sent == 5).any()      # around the held slots
