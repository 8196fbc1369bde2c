"""ggnn_cudnn_gru_packed_f32 (csrc/ggnn_cudnn_gru_fused.hip): the CudnnCompatibleGRUCell in one launch, every supported (D, nx).

The C entry point is driven on caller-owned, over-allocated (+24 rows), NaN-prefilled outputs.  Per case: (1) h', r, u, c, hc are
within FACTOR x variant_kernel_ref.cudnn_gru_bounds of the float64 variant_kernel_ref.cudnn_gru -- the bound and factor
tests/test_gpu_variant_kernels.py holds the composed ggnn_cudnn_gru_f32 to; the exact bf16x3 products' error against float64 is below
the f32-MFMA kernels' (DESIGN.md K0), so the fused kernel stays inside it --, (2) h' is bit-identical with and without the saves and
from run to run, (3) rows beyond V of every output are still NaN, (4) ops.cudnn_gru_packed gives the same bits as the raw call,
(5) against the composed ops.cudnn_gru_train on the same inputs the difference is within the SUM of the two kernels' bounds (a
swapped gate or a misplaced bias is far outside it)."""
import ctypes

import numpy as np
import pytest
import torch

import variant_kernel_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 2                                     # tests/test_gpu_variant_kernels.py
SUPPORTED = [(D, nx) for D in (32, 64, 100) for nx in (1, 2, 3)]
PAD_ROWS = 24
NAMES = ("out", "r", "u", "c", "hc")


@pytest.fixture(scope="module")
def ops(pkg, cuda):
    return pkg.ops


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np(t):
    return t.detach().cpu().numpy()


def _launch(pkg, xs, h, packed, bg, bcx, bch, save):
    """The C entry point -> (h' buffer [V + PAD_ROWS, D], [r, u, c, hc] buffers or [])."""
    lib = pkg._lib.load()
    V, D = h.shape
    nx = len(xs)
    out = torch.full((V + PAD_ROWS, D), float("nan"), device=h.device)
    saves = [torch.full((V + PAD_ROWS, D), float("nan"), device=h.device) for _ in range(4)] if save else []
    ptrs = [s.data_ptr() for s in saves] if save else [None] * 4
    segs = (ctypes.c_void_p * nx)(*[x.data_ptr() for x in xs])
    pkg._lib.check(lib.ggnn_cudnn_gru_packed_f32(segs, nx, h.data_ptr(), packed.data_ptr(), bg.data_ptr(), bcx.data_ptr(), bch.data_ptr(),
                                                 out.data_ptr(), *ptrs, V, D, torch.cuda.current_stream().cuda_stream))
    return out, saves


def _check_case(pkg, ops, cuda, D, nx, V, c=None):
    what = "cudnn_gru_fused.D%d.nx%d[V=%d]" % (D, nx, V)
    if c is None:
        c = ref.cell_inputs(D, V, nx, ref.seed_of("cudnn_fused", D, nx, V))
    w = c["cudnn"]
    xs, h = [_dev(x, cuda) for x in c["xs"]], _dev(c["h"], cuda)
    t = {k: _dev(v, cuda) for k, v in w.items()}
    packed = ops.cudnn_gru_pack(t["Wg"], t["Wcx"], t["Wch"], nx)
    assert packed.numel() * 4 == pkg._lib.load().ggnn_cudnn_gru_packed_bytes(D, nx)
    out_s, saves = _launch(pkg, xs, h, packed, t["bg"], t["bcx"], t["bch"], save=True)
    out_n, _ = _launch(pkg, xs, h, packed, t["bg"], t["bcx"], t["bch"], save=False)
    out_2, saves_2 = _launch(pkg, xs, h, packed, t["bg"], t["bcx"], t["bch"], save=True)
    got = [out_s] + saves
    # (1) against float64
    want = ref.cudnn_gru(c["xs"], c["h"], **w)
    B = ref.cudnn_gru_bounds(c["xs"], c["h"], **w)
    for name, g, wnt, bnd in zip(NAMES, got, want, B):
        ref.assert_within(_np(g[:V]), wnt, bnd, FACTOR, "%s.%s" % (what, name))
    # (2) bit-identical with and without the saves, and from run to run
    assert torch.equal(out_s[:V], out_n[:V]), what + ": h' depends on the saves"
    assert torch.equal(out_s[:V], out_2[:V]), what + ": two runs differ in h'"
    for name, a, b in zip(NAMES[1:], saves, saves_2):
        assert torch.equal(a[:V], b[:V]), what + ": two runs differ in " + name
    # (3) nothing beyond V is written
    for name, buf in zip(NAMES + ("out (no saves)",), got + [out_n]):
        assert bool(torch.isnan(buf[V:]).all()), "%s: rows beyond V of %s were written" % (what, name)
    # (4) the host-layer wrapper runs the same launch
    save = {}
    out_w = ops.cudnn_gru_packed(xs, h, packed, t["bg"], t["bcx"], t["bch"], save=save)
    assert torch.equal(out_w, out_s[:V]), what + ": ops.cudnn_gru_packed h'"
    for name, buf in zip(NAMES[1:], saves):
        assert torch.equal(save[name], buf[:V]), what + ": ops.cudnn_gru_packed " + name
    assert torch.equal(ops.cudnn_gru_packed(xs, h, packed, t["bg"], t["bcx"], t["bch"]), out_s[:V])
    # (5) against the composed three-launch cell: within the sum of the two kernels' bounds
    composed = ops.cudnn_gru_train(xs, h, **t)              # -> (h', r, u, c, hc)
    for name, g, o, bnd in zip(NAMES, got, composed, B):
        ref.assert_within(_np(g[:V]), _np(o).astype(np.float64), 2 * np.asarray(bnd), FACTOR, "%s.%s vs composed" % (what, name))
    return c, got


@pytest.mark.parametrize("V", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("D,nx", SUPPORTED)
def test_fused_cell(pkg, ops, cuda, D, nx, V):
    assert ops.cudnn_gru_fused_supported(D, nx)
    _check_case(pkg, ops, cuda, D, nx, V)


def test_persistent_loop_second_round(pkg, ops, cuda):
    """More rows than one round of the persistent loop covers: rows_per_pass x max_workgroups + 40 (from the geometry query) reaches
    the second round and a partial last pass."""
    D, nx = 32, 1
    rows, wgs = ops.cudnn_gru_fused_launch_geometry(D, nx)
    assert rows > 0 and rows % 16 == 0 and wgs > 0
    _check_case(pkg, ops, cuda, D, nx, rows * wgs + 40)


def test_zero_padded_columns_stay_zero(pkg, ops, cuda):
    """Hidden 84 runs at width 100: columns 84 .. 99 of every operand are zero, and those columns of h' must be exactly 0
    (u = 0.5, c = tanh(0) = 0, h = 0)."""
    D, nx, V, H = 100, 3, 33, 84
    c = ref.cell_inputs(D, V, nx, ref.seed_of("cudnn_fused_pad", D, nx, V))
    for x in c["xs"] + [c["h"]]:
        x[:, H:] = 0
    w = c["cudnn"]
    for name, blocks in (("Wg", 2), ("Wcx", 1), ("Wch", 1)):
        W = w[name].reshape(-1, D, blocks, D)
        W[:, H:, :, :] = 0
        W[:, :, :, H:] = 0
    for name, blocks in (("bg", 2), ("bcx", 1), ("bch", 1)):
        w[name].reshape(blocks, D)[:, H:] = 0
    _, got = _check_case(pkg, ops, cuda, D, nx, V, c)
    out = _np(got[0][:V])
    assert not out[:, H:].any(), "the zero-padded columns of h' must be exactly 0"
    assert out[:, :H].any()
