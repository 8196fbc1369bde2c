"""The fused GRU forward after the rest of its non-model work went (csrc/ggnn_gru_fused.hip): one sigmoid epilogue for the packed tail
tile (hidden size 100: u columns 96..99 ride in the r gate's last tile), the epilogues' cross-lane moves as row swaps instead of LDS
permutes, the one-division mean at every fan-in, and the ticket counters zeroed by the compacted transform launches instead of a fill
in front of every forward (csrc/ggnn_propagate.hip).  None of it may change a bit:

  *  ggnn_gru_packed_gather_f32 == ggnn_gather_segment_sum_f32 + ggnn_gru_packed_f32 on the int32 views, whole tensor and columns
     96..99 on their own, on thin tail tickets only (V <= 197) and on full + tail tickets at the real grid size;
  *  the training launch stores the r, u, c of the un-gathered launch;
  *  every gather-fused result is inside the float64 bound of tests/gru_fwd_ref.py (a-priori, magnitudes only) at the factor the GPU
     tests of tests/variant_kernel_ref.py use (2 = gru_fwd_ref.CAP[100]);
  *  ggnn_sparse_propagate_f32 gives the same bits on a fresh workspace, on the workspace a call has just used and on one filled with
     0xFF bytes.

The graphs hold in-degrees 0 (the mean divides 0 by 1e-7), 1, 2, 3 (an inexact division), 4 (the gather's pipelined slots) and 6 (two
slots fetched synchronously)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gru_fwd_ref as gr

pytestmark = pytest.mark.gpu

T = 4
DEGREES = (3, 0, 1, 2, 4, 6)                     # in-degree of node v: DEGREES[v % 6]
SMALL_V = (1, 15, 16, 17, 33, 4 * 16 * 3 + 5)    # thin tail tickets only
LARGE_V = 32768 + 16 * 7 + 3                     # full tickets of the 4-wave forms on 256 CUs and tail tickets
UNTOUCHED = 7.0                                  # prefill of the propagate test's outputs: outside [-1, 1], where every state lies
FACTOR = 2.0                                     # variant_kernel_ref: "The GPU tests use factor 2"
assert FACTOR == gr.CAP[100] == gr.CAP[64]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _graph(V):
    """Adjacency lists [E_t, 2] (source, target) and the in-degree table [V, T]; sources and types random, every list shuffled."""
    rng = np.random.default_rng(5 * V + 1)
    deg = np.array([DEGREES[v % 6] for v in range(V)])
    dst = np.repeat(np.arange(V), deg).astype(np.int32)
    src = rng.integers(0, V, len(dst)).astype(np.int32)
    typ = rng.integers(0, T, len(dst))
    order = rng.permutation(len(dst))
    src, dst, typ = src[order], dst[order], typ[order]
    adj = tuple(np.stack([src[typ == t], dst[typ == t]], axis=1).astype(np.int32).reshape(-1, 2) for t in range(T))
    nin = np.zeros((V, T), np.float32)
    for t in range(T):
        np.add.at(nin[:, t], adj[t][:, 1], 1.0)
    assert (nin.sum(-1) == deg).all() and (V < 6 or set(deg) == set(DEGREES))
    return adj, nin


@functools.lru_cache(maxsize=None)
def _case(D, nx, V, act, use_avg):
    """The host side of a case (gru_fwd_ref.Case on this file's graph): states, residual inputs and message rows in (-1, 1)."""
    rng = np.random.default_rng(1000 * V + D)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    h, res, H = u(V, D), (u(V, D), u(V, D)), u(V, T * D)
    adj, nin = _graph(V)
    Wg, bg, Wc, bc = gr.weights(D, nx)
    return gr.Case(D, nx, V, T, True, int(use_avg), act, res[:nx - 1], H, h, Wg, bg, Wc, bc, adj, nin, None)


@functools.lru_cache(maxsize=None)
def _bounds(D, nx, V, act, use_avg):
    """(float64 reference, a-priori bounds) of a case: computed once, shared by both operand formats, never written."""
    return gr.bounds(_case(D, nx, V, act, use_avg))


@functools.lru_cache(maxsize=None)
def _device(D, V):
    """Device tensors shared by every case at (D, V); never written."""
    c = _case(D, 3, V, "tanh", 1)
    return dict(h=dev(c.h), res=[dev(r) for r in c.res], H=dev(c.H), adj=[dev(a) for a in c.adj], nin=dev(c.nin))


@functools.lru_cache(maxsize=None)
def _weights(D, nx):
    return tuple(dev(w) for w in gr.weights(D, nx))


def _check(pkg, D, nx, fmt, act, use_avg, V, fp64):
    Wg, bg, Wc, bc = _weights(D, nx)
    packed = pkg.ops.PackedWeights().gru(Wg, Wc, nx, D, fmt)
    i = _device(D, V)
    h, res, H = i["h"], i["res"][:nx - 1], i["H"]
    nin = i["nin"] if use_avg else None
    index = pkg.ops.build_message_index(i["adj"], V)
    incoming = pkg.ops.gather_segment_sum(H, index, nin, None, bool(use_avg))
    want = pkg.ops.gru_packed(res + [incoming], h, packed, bg, bc, activation=act, fmt=fmt)
    cnt = torch.zeros(1, dtype=torch.int32, device=h.device)
    for counter in (None, cnt):                                      # static tickets | a zeroed device counter
        got = pkg.ops.gru_packed_gather(res, h, packed, bg, bc, H.view(V * T, D), index, None, nin, activation=act,
                                        tile_counter=counter, fmt=fmt)
        what = (D, nx, fmt, act, use_avg, V, counter is not None)
        if D % 16:
            tail = slice(D - D % 16, D)                              # the packed tail tile's columns, on their own
            assert torch.equal(bits(got[:, tail]), bits(want[:, tail])), ("tail columns",) + what
        assert torch.equal(bits(got), bits(want)), what
        if fp64:
            ref, bound = _bounds(D, nx, V, act, use_avg)
            gr.assert_within(got.cpu().numpy(), ref["h_out"], bound["h_out"], FACTOR, "h_out %s" % (what,))
    assert int(cnt[0]) > 0
    if V >= 2:
        assert DEGREES[1] == 0 and torch.all(incoming[1] == 0)       # the node without incoming messages


@pytest.mark.parametrize("use_avg", [1, 0], ids=["mean", "sum"])
@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("fmt", [2, 3], ids=["f16x2", "bf16x3"])
@pytest.mark.parametrize("nx", [1, 2, 3])
def test_gather_fused_equals_composed_route_h100(pkg, cuda, nx, fmt, act, use_avg):
    for V in SMALL_V:
        _check(pkg, 100, nx, fmt, act, use_avg, V, fp64=True)
    # the real grid size; against float64 there for the benchmark's cell (tanh, mean), bit for bit for all
    _check(pkg, 100, nx, fmt, act, use_avg, LARGE_V, fp64=(act == "tanh" and use_avg == 1))


@pytest.mark.parametrize("fmt", [2, 3], ids=["f16x2", "bf16x3"])
def test_gather_fused_equals_composed_route_h64(pkg, cuda, fmt):
    """No tail tile at hidden size 64: unaffected."""
    for V in SMALL_V:
        _check(pkg, 64, 1, fmt, "tanh", 1, V, fp64=True)


@pytest.mark.parametrize("use_avg", [1, 0], ids=["mean", "sum"])
@pytest.mark.parametrize("fmt", [2, 3], ids=["f16x2", "bf16x3"])
@pytest.mark.parametrize("nx", [1, 2, 3])
def test_training_launch_saves_the_ungathered_gates(pkg, cuda, nx, fmt, use_avg):
    D = 100
    Wg, bg, Wc, bc = _weights(D, nx)
    packed = pkg.ops.PackedWeights().gru(Wg, Wc, nx, D, fmt)
    for V in SMALL_V:
        i = _device(D, V)
        h, res, H = i["h"], i["res"][:nx - 1], i["H"]
        nin = i["nin"] if use_avg else None
        index = pkg.ops.build_message_index(i["adj"], V)
        incoming = pkg.ops.gather_segment_sum(H, index, nin, None, bool(use_avg))
        want_s, got_s = {}, {}
        want = pkg.ops.gru_packed(res + [incoming], h, packed, bg, bc, fmt=fmt, save=want_s)
        got = pkg.ops.gru_packed_gather(res, h, packed, bg, bc, H.view(V * T, D), index, None, nin, save=got_s, fmt=fmt)
        assert torch.equal(bits(got), bits(want)), V
        for k in ("r", "u", "c"):
            assert torch.equal(bits(got_s[k][:, 96:]), bits(want_s[k][:, 96:])), (V, k, "tail columns")
            assert torch.equal(bits(got_s[k]), bits(want_s[k])), (V, k)
        assert torch.equal(bits(got_s["incoming"]), bits(incoming)), V
        ref, bound = _bounds(D, nx, V, "tanh", use_avg)
        for k in ("r", "u", "c", "incoming"):
            gr.assert_within(got_s[k].cpu().numpy(), ref[k], bound[k], FACTOR, "%s nx=%d fmt=%d V=%d" % (k, nx, fmt, V))


@pytest.mark.parametrize("fmt", [2, 3], ids=["f16x2", "bf16x3"])
def test_forward_does_not_lean_on_a_fill_of_the_ticket_counters(pkg, cuda, fmt):
    """ggnn_sparse_propagate_f32 with a caller-held workspace, layers of [2, 1] steps (the second with a residual input), at the size
    whose GRU launches take their tail tickets from the counters: a fresh (zeroed) workspace, the same workspace again -- its counters
    are where the first call left them -- and a workspace of 0xFF bytes give the same bits.  The outputs start as a value no state can
    take (|h'| <= 1 for |h| <= 1), so a ticket nobody took shows.
    The test hands no NaN-patterned memory back: the 0xFF workspace is zeroed before it is released and the outputs' sentinel is
    finite -- freed device memory reaches later allocations uninitialised, in this process and in the next one on the device, and a
    test that compares two `torch.empty` results of a launch without rows then meets NaN != NaN."""
    from conftest import random_graph_batch
    ops = pkg.ops
    lib = pkg._lib.load()
    D, V = 100, LARGE_V
    steps, residuals = [2, 1], [[], [0]]
    rng = np.random.default_rng(fmt)
    h, adj, nin = random_graph_batch(rng, V, (5 * V) // 2, T, D, sorted_src=True)
    index = ops.build_message_index([dev(a) for a in adj], V)
    comp = ops.build_compact_sources(index)
    pw = ops.PackedWeights()
    keep, edge_packed, bg, bc, gru_packed = [], [], [], [], []
    for l in range(len(steps)):
        nx = len(residuals[l]) + 1
        Wg, bgl, Wc, bcl = _weights(D, nx)
        edge_w = dev(rng.uniform(-0.3, 0.3, (T, D, D)).astype(np.float32))
        keep.append(edge_w)
        edge_packed.append(pw.edge(edge_w, fmt))
        gru_packed.append(pw.gru(Wg, Wc, nx, D, fmt))
        bg.append(bgl)
        bc.append(bcl)
    h0, nin_d = dev(h), dev(nin)
    L = len(steps)
    i32 = lambda xs: (ctypes.c_int32 * max(len(xs), 1))(*xs)
    off = (ctypes.c_int64 * (T + 1))(*comp.type_row_off)
    ws_bytes = lib.ggnn_sparse_propagate_workspace_bytes(V, D, T, comp.num_rows)

    def run(ws):
        outs = [torch.full_like(h0, UNTOUCHED) for _ in range(L)]
        rc = lib.ggnn_sparse_propagate_f32(
            ops._ptr(h0), V, D, T, ops._ptr(index.row_ptr), ops._ptr(comp.gather_row), ops._ptr(comp.pair_node), off,
            ops._ptr(nin_d), 1, L, i32(steps), i32([0, 0, 1]), i32([0]), None, ops._ptr_array(edge_packed), None, None,
            ops._ptr_array(bg), None, ops._ptr_array(bc), ops._ptr_array(gru_packed), i32([fmt] * L), i32([fmt] * L), 0, ops.FUSE_GATHER,
            ops._ptr_array(outs), ops._ptr(ws), ws_bytes, ops._stream())
        assert rc == 0, lib.ggnn_last_error()
        torch.cuda.synchronize()
        return outs

    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=h0.device)
    first = run(ws)
    again = run(ws)
    ws_ff = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=h0.device)
    ones = run(ws_ff)
    ws_ff.zero_()
    torch.cuda.synchronize()
    assert float(h0.abs().max()) <= 1.0
    for l in range(L):
        assert float(first[l].abs().max()) < 2.0, l                  # (finite, and no row left at UNTOUCHED)
        assert torch.equal(bits(again[l]), bits(first[l])), ("same workspace", l)
        assert torch.equal(bits(ones[l]), bits(first[l])), ("0xFF workspace", l)
