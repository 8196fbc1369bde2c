"""ggnn_rnn_panel_gather_f32 (csrc/ggnn_rnn_panel.hip): the BasicRNNCell with the segment sum gathered inside at hidden sizes 128 / 192 /
256 on column panels -- the twin of tests/test_gpu_rnn_fused_kernel.py.  The three widths cover PARTS = 1, 3 and 2 of the ring.

Per case: (1) the gathered segment the launch writes back is torch.equal to the stand-alone segment sum over the same compact rows
(ops.gather_segment_sum_compact without bias), (2) h' is within FACTOR x variant_kernel_ref.rnn_bound of the float64 cell evaluated
on the GPU's own `incoming`, (3) h' is bit-identical with and without save_incoming and from run to run, (4) rows beyond V of an
over-allocated, NaN-prefilled output stay untouched.  The graph is variant_kernel_ref.build_graph (node 0 without messages, the
70-message hub, an empty edge type); W / b carry the all-zero column and the b = -100 column: ReLU's two edges.
"""
import ctypes

import numpy as np
import pytest
import torch

import variant_kernel_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 2                                     # tests/test_gpu_variant_kernels.py
SUPPORTED = [(D, nx) for D in (128, 192, 256) for nx in (1, 2, 3)]
PAD_ROWS = 24


@pytest.fixture(scope="module")
def ops(pkg, cuda):
    return pkg.ops


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np(t):
    return t.detach().cpu().numpy()


def _launch(pkg, residuals, h, packed, b, Hc, index, comp, nin, T, use_avg, act, save):
    """The C entry point on caller-owned, over-allocated, NaN-prefilled outputs -> (h' buffer [V + PAD_ROWS, D], incoming buffer)."""
    lib = pkg._lib.load()
    V, D = h.shape
    nx = len(residuals) + 1
    out = torch.full((V + PAD_ROWS, D), float("nan"), device=h.device)
    inc = torch.full((V + PAD_ROWS, D), float("nan"), device=h.device) if save else None
    segs = (ctypes.c_void_p * max(nx - 1, 1))(*[x.data_ptr() for x in residuals])
    pkg._lib.check(lib.ggnn_rnn_panel_gather_f32(
        segs, nx, h.data_ptr(), packed.data_ptr(), b.data_ptr(), out.data_ptr(), Hc.data_ptr(), Hc.shape[0], index.row_ptr.data_ptr(),
        comp.gather_row.data_ptr(), comp.gather_row.numel(), nin.data_ptr(), T, 1 if use_avg else 0,
        None if inc is None else inc.data_ptr(), V, D, pkg.ops.ACT_IDS[act], torch.cuda.current_stream().cuda_stream))
    return out, inc


def _check_case(pkg, ops, cuda, D, nx, V, T, switches):
    seed = ref.seed_of("rnn_panel", D, nx, V, T)
    c = ref.cell_inputs(D, V, nx, seed)
    adj, nin_np, info = ref.build_graph(V, T, seed + 1)
    index = ops.build_message_index([_dev(a, cuda) for a in adj], V)
    comp = ops.build_compact_sources(index)
    R = comp.num_rows
    assert 0 < R <= index.num_messages
    rng = np.random.default_rng(seed + 2)
    Hc_np = rng.normal(size=(R, D)).astype(np.float32)       # the kernel needs no transform: any [R, D] rows
    Hc, nin = _dev(Hc_np, cuda), _dev(nin_np, cuda)
    residuals = [_dev(x, cuda) for x in c["xs"][:nx - 1]]
    h, W, b = _dev(c["h"], cuda), _dev(c["W"], cuda), _dev(c["b"], cuda)
    packed = ops.rnn_panel_pack(W, nx)
    assert packed.numel() * 4 == pkg._lib.load().ggnn_rnn_panel_packed_bytes(D, nx)
    for use_avg, act in switches:
        what = "rnn_panel.D%d.nx%d[V=%d T=%d avg=%d %s]" % (D, nx, V, T, use_avg, act)
        want_inc = ops.gather_segment_sum_compact(Hc, index, comp, nin, None, use_avg)
        out_s, inc_s = _launch(pkg, residuals, h, packed, b, Hc, index, comp, nin, T, use_avg, act, save=True)
        out_n, _ = _launch(pkg, residuals, h, packed, b, Hc, index, comp, nin, T, use_avg, act, save=False)
        out_2, inc_2 = _launch(pkg, residuals, h, packed, b, Hc, index, comp, nin, T, use_avg, act, save=True)
        # (1) the gathered segment
        assert torch.equal(inc_s[:V], want_inc), what + ": save_incoming differs from the stand-alone segment sum"
        if V > 1:
            assert not _np(inc_s[0]).any(), what + ": node 0 receives nothing, its row must be exactly zero"
        # (2) the cell against float64, on the GPU's own incoming
        xs = c["xs"][:nx - 1] + [_np(inc_s[:V])]
        want = ref.rnn(xs, c["h"], c["W"], c["b"], act)
        ref.assert_within(_np(out_s[:V]), want, ref.rnn_bound(xs, c["h"], c["W"], c["b"], act), FACTOR, what)
        if act == "relu":
            got = _np(out_s[:V])
            # The b = -100 column is 0 where its pre-activation is negative.  That is every row, except at V = 1 under SUM aggregation:
            # there the one node is the hub and all its ~75 messages are self-loops on one compact row, so `incoming` is ~75 x one
            # N(0, 1) row and at these widths the product alone can pass 100 (D = 128: 136.5 in float64 too).
            clipped = want[:, D - 3] == 0
            assert clipped.all() or (V == 1 and not use_avg), what + ": the b = -100 column's pre-activation is positive in float64"
            assert not got[:, 5].any() and not got[clipped, D - 3].any(), \
                what + ": the zero column and the b = -100 column must be exactly 0"
        # (3) bit-identical with and without the save, and from run to run
        assert torch.equal(out_s[:V], out_n[:V]), what + ": h' depends on save_incoming"
        assert torch.equal(out_s[:V], out_2[:V]) and torch.equal(inc_s[:V], inc_2[:V]), what + ": two runs differ"
        # (4) nothing beyond V is written
        for buf in (out_s, out_n, inc_s):
            assert bool(torch.isnan(buf[V:]).all()), what + ": rows beyond V were written"
        # the host-layer wrapper runs the same launch
        save = {}
        nin_arg = nin if use_avg else None
        out_w = ops.rnn_panel_gather(residuals, h, packed, b, Hc, index, comp.gather_row, nin_arg, act, save=save)
        assert torch.equal(out_w, out_s[:V]) and torch.equal(save["incoming"], inc_s[:V]), what + ": ops.rnn_panel_gather"


ALL_SWITCHES = [(True, "tanh"), (True, "relu"), (False, "tanh"), (False, "relu")]


@pytest.mark.parametrize("V", [1, 16, 17, 33, 129])          # 129: one row past a workgroup's pass of 8 x 16
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("D,nx", SUPPORTED)
def test_panel_cell(pkg, ops, cuda, D, nx, T, V):
    assert ops.rnn_panel_supported(D, nx)
    _check_case(pkg, ops, cuda, D, nx, V, T, ALL_SWITCHES)


def test_second_pass(pkg, ops, cuda):
    """More rows than one pass of the launch covers: rows_per_workgroup x max_workgroups + 40 (from the geometry query)."""
    D, nx = 128, 1
    rows, wgs = ops.rnn_panel_launch_geometry(D, nx)
    assert rows > 0 and rows % 16 == 0 and wgs > 0
    _check_case(pkg, ops, cuda, D, nx, rows * wgs + 40, 3, [(True, "relu")])


def test_out_of_range_gather_rows_contribute_nothing(pkg, ops, cuda):
    """A gather_row outside [0, num_rows) adds nothing and is not dereferenced; row_ptr values are clamped to [0, M]: the launch on
    an index whose LAST slots point past the rows equals the segment sum over the index without those slots."""
    D, nx, V, T = 192, 2, 17, 3
    seed = ref.seed_of("rnn_panel_oob")
    c = ref.cell_inputs(D, V, nx, seed)
    adj, nin_np, _ = ref.build_graph(V, T, seed + 1)
    index = ops.build_message_index([_dev(a, cuda) for a in adj], V)
    comp = ops.build_compact_sources(index)
    R = comp.num_rows
    Hc = _dev(np.random.default_rng(seed).normal(size=(R, D)).astype(np.float32), cuda)
    nin = _dev(nin_np, cuda)
    residuals = [_dev(x, cuda) for x in c["xs"][:nx - 1]]
    h, W, b = _dev(c["h"], cuda), _dev(c["W"], cuda), _dev(c["b"], cuda)
    packed = ops.rnn_panel_pack(W, nx)
    want, _ = _launch(pkg, residuals, h, packed, b, Hc, index, comp, nin, T, False, "tanh", save=False)
    # the same rows with a tail of Hc cut off: the slots that pointed there now point outside [0, num_rows)
    keep = R - 3
    gather = _np(comp.gather_row)
    row_ptr = _np(index.row_ptr)
    seg = np.repeat(np.arange(V), np.diff(row_ptr))
    inc = np.zeros((V, D), np.float32)
    Hc_np = _np(Hc)
    for s in range(len(gather)):                            # slot order, float32: the kernel's own sum
        if gather[s] < keep:
            inc[seg[s]] += Hc_np[gather[s]]
    got, got_inc = _launch(pkg, residuals, h, packed, b, Hc[:keep].contiguous(), index, comp, nin, T, False, "tanh", save=True)
    np.testing.assert_array_equal(_np(got_inc[:V]), inc)
    assert not torch.equal(got[:V], want[:V])               # (the cut rows did carry messages)
    xs = c["xs"][:nx - 1] + [inc]
    ref.assert_within(_np(got[:V]), ref.rnn(xs, c["h"], c["W"], c["b"], "tanh"), ref.rnn_bound(xs, c["h"], c["W"], c["b"], "tanh"),
                      FACTOR, "rnn_panel.out_of_range")
