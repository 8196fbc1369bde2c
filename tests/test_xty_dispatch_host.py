"""Which kernel runs a weight-gradient product (ggnn_xty_f32 / ggnn_xty_acc_f32, csrc/ggnn_bwd_gemm.hip), checked without a GPU
through ggnn_xty_describe -- the launcher's own selection function -- and ggnn_xty_cells, the dispatch table it selects from:

  coverage   every instantiation in the table is selected by some swept shape in some leg (tests/test_gpu_xty_cells.py runs them)
  package    every shape the models produce has a kernel on both matrix paths
  refusals   the shapes refused inside the accepted domain are exactly the ones include/ggnn_hip.h names
  pins       the cell of the training shapes at hidden 32 / 64 / 96 / 100: a change of selection is a diff of this file
  bound      the bound the GPU test holds the kernels to (xty_cases.REL / ABS) passes a plain float32 row-by-row product of the
             same cases, and fails each of seven wrong results a kernel of this design could produce (teeth)."""
import ctypes

import numpy as np
import pytest

import xty_cases as xc

LEGS = xc.LEGS


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.fixture(scope="module")
def sweeps(lib):
    """{leg: ({cell: smallest shape}, [(refused shape, rc)])}: one sweep per leg, shared by the tests below."""
    return {name: xc.sweep(lib, leg) for name, leg in LEGS.items()}


def test_symbols_and_argument_errors(lib, pkg):
    for name in ("ggnn_xty_describe", "ggnn_xty_cells"):
        assert name in pkg._lib.SYMBOLS and getattr(lib, name) is not None
    out = (ctypes.c_int32 * 8)()
    assert lib.ggnn_xty_describe(200, 200, 1, 0, -1, -1, -1, None) == xc.E_INVALID
    for K, N in ((0, 100), (-4, 100), (6, 100), (100, 0), (100, 6), (100, 260), (100, -4)):
        assert lib.ggnn_xty_describe(K, N, 0, 0, 1, 1, 0, out) == xc.E_INVALID, (K, N)
        assert lib.ggnn_last_error()
    assert lib.ggnn_xty_describe(200, 200, 1, 0, 1, 1, 0, out) == 0
    # {family, gathered, rows, mtm, ntm, K blocks, X tiles per K block, dY tiles}: 201 rows = 13 tiles in one block, 200 columns = 13
    assert list(out) == [2, 0, 32, 4, 4, 1, 13, 13]
    assert lib.ggnn_xty_describe(1024, 64, 0, 0, 1, 1, 0, out) == 0 and list(out[5:]) == [4, 16, 4]
    assert lib.ggnn_xty_describe(1024, 64, 1, 0, 1, 1, 0, out) == 0 and list(out[5:]) == [5, 13, 4]     # 1025 rows: 65 tiles
    # the table can be counted without a buffer, and a short buffer is not overrun
    n = lib.ggnn_xty_cells(None, 0)
    buf = (ctypes.c_int32 * 10)(*([-7] * 10))
    assert lib.ggnn_xty_cells(buf, 1) == n and list(buf[5:]) == [-7] * 5 and buf[0] in (0, 1, 2)


def test_every_instantiation_is_selected_by_a_swept_shape(lib, sweeps):
    """The table is learnt from the library, not copied here; its size is pinned (33 + 4 + 4), so that a kernel added to the table
    shows up as a failure until the sweep (and with it the GPU test) reaches it."""
    table = xc.table(lib)
    assert len(table) == len(set(table)) == lib.ggnn_xty_cells(None, 0) == 41
    assert sorted((f, sum(1 for c in table if c[0] == f)) for f in xc.FAMILIES) == [(0, 33), (1, 4), (2, 4)]
    reached = {}
    for name, (cells, _) in sweeps.items():
        assert set(cells) <= set(table), (name, set(cells) - set(table))          # nothing is launched that the table lacks
        for c in cells:
            reached.setdefault(c, []).append(name)
    assert set(reached) == set(table), sorted(set(table) - set(reached))
    # six 32-row f32 instantiations exist for the GGNN_XTY_ROWS=32 experiment alone, and the per-wave split kernel's 64-row forms
    # only run when the planes kernel is switched off
    only = lambda leg: sorted(c for c, legs in reached.items() if legs == [leg])
    assert only("rows32") == [(0, 0, 32, 1, 1), (0, 0, 32, 1, 2), (0, 0, 32, 1, 3), (0, 0, 32, 2, 1), (0, 0, 32, 2, 2), (0, 0, 32, 3, 1)]
    assert only("noplanes") == [(1, 0, 64, 3, 2), (1, 0, 64, 4, 2)]
    # the default leg reaches the per-wave split kernel too: 27 or more tiles of operand columns do not fit the planes' LDS
    assert {c for c in sweeps["default"][0] if c[0] == 1} == {(1, 0, 32, 3, 4), (1, 0, 32, 4, 4)}


def package_shapes():
    """(K, N, ones, gathered) of every product the models ask for (backward.py, the native training steps)."""
    shapes = set()
    for D in (32, 64, 96, 100):
        for nseg in (1, 2, 3, 4):
            for N in (D, 2 * D):
                for ones in (0, 1):
                    shapes.add((nseg * D, N, ones, 0))            # GRU / RNN-cell weights (+ bias through the ones row)
        for N in (4, 8):
            shapes.add((D, N, 0, 0))                              # edge-bias products: N = number of edge types
        shapes.add((D, D, 0, 0))                                  # the GCN's layer weights
    for D in (32, 64, 96, 100, 128):
        shapes.add((D, D, 0, 1))                                  # edge weights: rows of h gathered per message
    return sorted(shapes)


def test_every_package_shape_has_a_kernel_on_both_matrix_paths(lib):
    for leg in ("default", "f32"):
        for shape in package_shapes():
            rc, cell, _ = xc.describe(lib, *shape, LEGS[leg])
            assert rc == 0 and cell is not None, (leg, shape, lib.ggnn_last_error())
            assert cell[1] == shape[3]


def header_refuses(shape, leg):
    """include/ggnn_hip.h: refused inside the accepted domain are the row-gathered products with Kout > 128 or N > 128, and every
    row-gathered product under GGNN_XTY_ROWS=32."""
    K, N, ones, gathered = shape
    return bool(gathered) and (K + ones > 128 or N > 128 or leg.rows_override == 32)


def test_refused_set_is_what_the_header_states(sweeps):
    for name, (_, refused) in sweeps.items():
        assert all(rc == xc.E_UNSUPPORTED for _, rc in refused), name           # inside the domain nothing is an ARGUMENT error
        got = {s for s, _ in refused}
        want = {s for s in xc.swept_shapes() if header_refuses(s, LEGS[name])}
        assert got == want, (name, sorted(got ^ want)[:10])


def test_wide_blocks_run_on_32_row_slabs(lib):
    """A 16-tile operand (pitch 272) does not fit a wave's DMA instructions with 64-row slabs; before the selection looked at that,
    Kout per block 241..256 with N <= 48 (and N 241..256 with Kout <= 48) were refused as 'slab too wide'."""
    for leg in LEGS.values():
        for K, N, ones in ((240, 4, 1), (256, 48, 0), (244, 16, 0), (496, 32, 0), (4, 244, 1), (48, 256, 0), (32, 256, 1)):
            rc, cell, _ = xc.describe(lib, K, N, ones, 0, leg)
            assert rc == 0 and cell[0] == 0 and cell[2] == 32, (K, N, ones, cell)
    assert xc.describe(lib, 236, 4, 1, 0, LEGS["default"])[1] == (0, 0, 64, 4, 1)            # 15 tiles: still 64 rows


# (K, N, ones, gathered): (cell on the default path, cell under GGNN_MATRIX=f32) -- [incoming | h] and [x0 | incoming | h] against
# dpc (N = D) and dpg (N = 2 D) with the bias row, and the row-gathered edge-weight product, at hidden 32, 64, 96, 100
PINS = {
    (64, 32, 1, 0): ((0, 0, 64, 2, 1), (0, 0, 64, 2, 1)),
    (64, 64, 1, 0): ((0, 0, 64, 2, 1), (0, 0, 64, 2, 1)),
    (96, 32, 1, 0): ((0, 0, 64, 2, 1), (0, 0, 64, 2, 1)),
    (96, 64, 1, 0): ((0, 0, 64, 2, 1), (0, 0, 64, 2, 1)),
    (32, 32, 0, 1): ((0, 1, 64, 1, 1), (0, 1, 64, 1, 1)),
    (128, 64, 1, 0): ((0, 0, 64, 3, 1), (0, 0, 64, 3, 1)),
    (128, 128, 1, 0): ((2, 0, 32, 3, 2), (0, 0, 64, 3, 2)),
    (192, 64, 1, 0): ((0, 0, 64, 4, 1), (0, 0, 64, 4, 1)),
    (192, 128, 1, 0): ((2, 0, 32, 4, 2), (0, 0, 32, 4, 2)),
    (64, 64, 0, 1): ((0, 1, 64, 1, 1), (0, 1, 64, 1, 1)),
    (192, 96, 1, 0): ((2, 0, 32, 4, 2), (0, 0, 64, 4, 2)),
    (192, 192, 1, 0): ((0, 0, 32, 4, 3), (0, 0, 32, 4, 3)),
    (288, 96, 1, 0): ((2, 0, 32, 3, 2), (0, 0, 64, 3, 2)),
    (288, 192, 1, 0): ((0, 0, 32, 3, 3), (0, 0, 32, 3, 3)),
    (96, 96, 0, 1): ((0, 1, 64, 2, 2), (0, 1, 64, 2, 2)),
    (200, 100, 1, 0): ((2, 0, 32, 4, 2), (0, 0, 64, 4, 2)),
    (200, 200, 1, 0): ((2, 0, 32, 4, 4), (0, 0, 32, 4, 4)),
    (300, 100, 1, 0): ((2, 0, 32, 3, 2), (0, 0, 64, 3, 2)),
    (300, 200, 1, 0): ((2, 0, 32, 3, 4), (0, 0, 32, 3, 4)),
    (100, 100, 0, 1): ((0, 1, 64, 2, 2), (0, 1, 64, 2, 2)),
}


def test_training_shapes_are_pinned_to_their_cells(lib):
    for shape, (split, f32) in PINS.items():
        assert xc.describe(lib, *shape, LEGS["default"])[1] == split, shape
        assert xc.describe(lib, *shape, LEGS["f32"])[1] == f32, shape


def test_oversized_calls_are_refused_without_a_launch(lib):
    """nbatch = 65 and N = 260 are argument errors of the product itself: found before any pointer is used (these are not device
    pointers, and this machine may have no GPU)."""
    fake = 4096
    segs = (ctypes.c_void_p * 1)(fake)
    ldx = (ctypes.c_int32 * 1)(100)
    big = 1 << 30

    def call(N=100, nbatch=1, K=100, Dseg=100):
        off = (ctypes.c_int32 * (nbatch + 1))(*([0] + [5] * nbatch))
        return lib.ggnn_xty_acc_f32(segs, 1, Dseg, ldx, None, fake, N + (-N) % 4, fake, None, 0, K, N, 0, off, nbatch, fake, big, None)

    assert call(nbatch=65) == xc.E_INVALID and b"batch" in lib.ggnn_last_error()
    assert call(nbatch=0) == xc.E_INVALID
    assert call(N=260) == xc.E_INVALID and b"260" in lib.ggnn_last_error()
    assert call(N=6) == xc.E_INVALID
    assert call(K=104) == xc.E_INVALID                                                    # K != nseg * Dseg
    out = (ctypes.c_int32 * 8)()
    assert lib.ggnn_xty_describe(100, 260, 0, 0, 1, 1, 0, out) == xc.E_INVALID


# ---- the bound: passes a plain f32 product, fails wrong ones -------------------------------------------------------------------------
def cell_cases(sweeps):
    """(cell, shape, M) of tests/test_gpu_xty_cells.py's per-cell cases, each once (a cell reached in several legs has one smallest
    shape per leg; most coincide)."""
    seen = set()
    for name in LEGS:
        for cell, shape in sorted(sweeps[name][0].items()):
            for M in xc.row_counts(cell[2]):
                if (shape, M) not in seen:
                    seen.add((shape, M))
                    yield cell, shape, M


def test_float32_product_by_rows_is_inside_the_bound(sweeps):
    """The bound is not tuned to the kernels: numpy's float32 product of the same operands, summed one row at a time, passes it
    -- weight rows and ones row alike."""
    worst = 0.0
    shapes = set()
    for cell, shape, M in cell_cases(sweeps):
        c = xc.make_case(M, M, *shape)
        want, bound = xc.reference(c)
        worst = max(worst, xc.assert_within(xc.float32_by_rows(c), want, bound, (cell, shape, M)))
        shapes.add(shape)
    print("worst error / bound of the float32 product by rows: %.3f over %d shapes" % (worst, len(shapes)))
    assert {s for cells, _ in sweeps.values() for s in cells.values()} == shapes
    # (measured 0.79, at an element whose sum happens to be large, |sum| = 17 of sum|.| = 62 over 257 rows: half an ulp of 16 per add)
    assert 0.05 < worst <= 1.0
    # batches: the per-batch sums, one batch empty, one of a single row
    c = xc.make_case(5, 300, 64, 68, 1, 1, row_off=[0, 131, 131, 132, 260, 300])
    want, bound = xc.reference(c)
    assert want.shape == (5, 65, 68) and not want[1].any() and np.all(bound[1] == xc.ABS)
    xc.assert_within(xc.float32_by_rows(c), want, bound, "batches")


def _fails(got, want, bound, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        xc.assert_within(got, want, bound, what)


@pytest.mark.parametrize("K,N,gathered,rows", [(64, 68, 0, 64), (192, 196, 0, 32), (300, 200, 0, 32), (64, 68, 1, 64), (4, 4, 0, 64)])
def test_teeth(K, N, gathered, rows):
    """Wrong results of the kinds this design can produce, at the LARGEST row count of the per-cell cases (the loosest bound): each
    must fall outside the bound."""
    M = xc.row_counts(rows)[-1]
    c = xc.make_case(K + N, M, K, N, 1, gathered)
    X, Y = xc.x_matrix(c).astype(np.float64), xc.y_matrix(c).astype(np.float64)
    want, bound = xc.reference(c)
    xc.assert_within(want, want, bound, "the reference itself")
    _fails(np.full_like(want, np.nan), want, bound, "NaN")

    got = want.copy(); got[0] -= np.outer(X[M - 1], Y[M - 1])
    _fails(got, want, bound, "one row dropped")
    got = want.copy(); got[0] -= X[M - M % 4:].T @ Y[M - M % 4:] if M % 4 else X[M - 4:].T @ Y[M - 4:]
    _fails(got, want, bound, "last 4-row step dropped")
    got = want.copy(); got[0] -= X[M - 4:].T @ Y[M - 4:]
    _fails(got, want, bound, "last 4 rows dropped")
    got = want.copy(); got[0, K] = 0.0
    _fails(got, want, bound, "ones row missing")
    nseg, Dseg = xc.segments(K)
    got = want.copy(); got[0, Dseg - 4:Dseg] = 0.0
    _fails(got, want, bound, "last float4 of the first segment dropped")
    got = want.copy(); got[0, K - 4:K] = 0.0
    _fails(got, want, bound, "last float4 of the last segment dropped")
    if K >= 32 and N >= 32:
        got = want.copy(); got[0, 0:16, 0:16], got[0, 16:32, 16:32] = want[0, 16:32, 16:32], want[0, 0:16, 0:16]
        _fails(got, want, bound, "two 16 x 16 tiles swapped")
        got = want.copy(); got[0, 16:32, 0:16] = want[0, 16:32, 0:16].T
        _fails(got, want, bound, "one tile transposed")
    # one row of the neighbouring batch added, in either direction; the GPU test scales neighbouring batches by 2^10 against each
    # other, here the plain operands already suffice
    off = [0, M // 2, M]
    cb = c._replace(row_off=off)
    wb, bb = xc.reference(cb)
    got = wb.copy(); got[0] += np.outer(X[off[1]], Y[off[1]])
    _fails(got, wb, bb, "first row of the next batch added")
    got = wb.copy(); got[1] += np.outer(X[off[1] - 1], Y[off[1] - 1])
    _fails(got, wb, bb, "last row of the previous batch added")
