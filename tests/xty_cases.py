"""Shared by tests/test_xty_dispatch_host.py (CPU) and tests/test_gpu_xty_cells.py (GPU): the sweep of ggnn_xty_describe over the
accepted domain of ggnn_xty_f32, the smallest shape that selects each kernel instantiation, the operands of a case, its float64
reference and its a-priori bound.  Nothing here knows the dispatch table: cells are learnt from the library (ggnn_xty_cells,
ggnn_xty_describe).

A cell is (family, gathered, rows, mtm, ntm): family 0 = xty_kernel (f32 MFMA), 1 = xty_split_kernel, 2 = xty_planes_kernel.
A shape is (K, N, ones, gathered).  A leg is one setting of the switches the library reads once per process."""
import ctypes
from collections import namedtuple

import numpy as np

FAMILIES = {0: "f32", 1: "split", 2: "planes"}
Leg = namedtuple("Leg", "env matrix_split planes rows_override")
LEGS = {
    "default": Leg({}, 1, 1, 0),
    "f32": Leg({"GGNN_MATRIX": "f32"}, 0, 1, 0),
    "noplanes": Leg({"GGNN_XTY_PLANES": "0"}, 1, 0, 0),
    "rows32": Leg({"GGNN_XTY_ROWS": "32"}, 1, 1, 32),
}
LEG_VARS = ("GGNN_MATRIX", "GGNN_XTY_SPLIT", "GGNN_XTY_PLANES", "GGNN_XTY_ROWS")
PROCESS = Leg({}, -1, -1, -1)                        # "whatever this process was started with"

K_MAX, N_MAX = 1024, 256
E_INVALID, E_UNSUPPORTED = -1, -2

# the bound of tests/test_gpu_parity.py and DESIGN.md's tolerance section for an f32 product chain, per output element:
# |got - want| <= REL * sum_r |x_r||y_r| + ABS; the ones row is an X column of ones, held to the same form (REL * sum_r |y_r| + ABS)
REL, ABS = 4e-7, 1e-6


def table(lib):
    """The library's dispatch table as a list of cells."""
    n = lib.ggnn_xty_cells(None, 0)
    buf = (ctypes.c_int32 * (5 * n))()
    assert lib.ggnn_xty_cells(buf, n) == n
    return [tuple(buf[5 * i:5 * i + 5]) for i in range(n)]


def describe(lib, K, N, ones, gathered, leg=PROCESS):
    """(rc, cell, (kblocks, kb_tiles, n_tiles)); cell and geometry are None when the shape is refused."""
    out = (ctypes.c_int32 * 8)()
    rc = lib.ggnn_xty_describe(K, N, int(ones), int(gathered), leg.matrix_split, leg.planes, leg.rows_override, out)
    if rc != 0:
        return rc, None, None
    return 0, tuple(out[:5]), tuple(out[5:8])


def swept_shapes():
    """K = nseg * Dseg with nseg <= 4 and Dseg % 4 == 0 (every multiple of 4: nseg = 1) up to 1024, N % 4 == 0 up to 256, both
    ones_row values, gathered and not."""
    for K in range(4, K_MAX + 1, 4):
        for N in range(4, N_MAX + 1, 4):
            for ones in (0, 1):
                for gathered in (0, 1):
                    yield K, N, ones, gathered


def sweep(lib, leg):
    """{cell: smallest shape by K * N that selects it in this leg} (ties: with the ones row, then the smaller K) and the list of
    refused shapes with their return codes."""
    best, refused = {}, []
    for K, N, ones, gathered in swept_shapes():
        rc, cell, _ = describe(lib, K, N, ones, gathered, leg)
        if rc != 0:
            refused.append(((K, N, ones, gathered), rc))
            continue
        key = (K * N, -ones, K)
        if cell not in best or key < best[cell][0]:
            best[cell] = (key, (K, N, ones, gathered))
    return {c: v[1] for c, v in best.items()}, refused


def family_name(cell):
    return FAMILIES[cell[0]] + ("-gathered" if cell[1] else "")


def family_shapes(cells):
    """{family name: the smallest swept shape WITH the ones row of that family} from a {cell: shape} map of shapes with ones == 1
    (see sweep_with_ones): the operands of the large-M, batch and accumulate cases."""
    best = {}
    for cell, shape in cells.items():
        name = family_name(cell)
        key = (shape[0] * shape[1], shape[0])
        if name not in best or key < best[name][0]:
            best[name] = (key, cell, shape)
    return {n: (v[1], v[2]) for n, v in best.items()}


def sweep_with_ones(lib, leg):
    """As sweep, over the shapes with the ones row only (add_bias_to needs it)."""
    best = {}
    for K, N, ones, gathered in swept_shapes():
        if not ones:
            continue
        rc, cell, _ = describe(lib, K, N, 1, gathered, leg)
        if rc == 0:
            key = (K * N, K)
            if cell not in best or key < best[cell][0]:
                best[cell] = (key, (K, N, 1, gathered))
    return {c: v[1] for c, v in best.items()}


def row_counts(rows):
    """Less than one MFMA step, the slab edges, a third slab (which reuses the first buffer), a second workgroup row that owns one
    row (workgroup rows are dealt one per 4 slabs) and one that owns a ragged tail."""
    return [1, 3, rows - 1, rows, rows + 1, 2 * rows + 1, 4 * rows + 1, 8 * rows + 5]


def segments(K):
    """(nseg, Dseg) of a swept K: as many segments (<= 4) as K allows, so that segment boundaries fall inside the product."""
    for nseg in (4, 3, 2, 1):
        if K % (4 * nseg) == 0:
            return nseg, K // nseg
    raise ValueError(K)


Case = namedtuple("Case", "xwide ywide nseg Dseg N ones x_rows row_off")


def make_case(seed, M, K, N, ones, gathered, row_off=None, x_rows=None, extra_x_rows=7):
    """uniform(-1, 1) operands: X's segments are column slices of ONE wider matrix, offset by 4 columns (so ldx > Dseg and the
    segments are not 64-byte aligned), dY a column slice of a wider matrix.  Row-gathered: X has more rows than M and the index
    holds repeats and X's last row."""
    rng = np.random.default_rng(seed)
    nseg, Dseg = segments(K)
    mx = M + extra_x_rows if gathered else M
    xwide = rng.uniform(-1, 1, (mx, K + 8)).astype(np.float32)
    ywide = rng.uniform(-1, 1, (M, N + 8)).astype(np.float32)
    if gathered and x_rows is None:
        x_rows = rng.integers(0, mx, M).astype(np.int32)
        if M:
            x_rows[rng.integers(0, M)] = mx - 1
        if M > 2:
            x_rows[M // 2] = x_rows[0]
    return Case(xwide, ywide, nseg, Dseg, N, int(ones), x_rows if gathered else None, row_off)


def scale_batches(c, log2=10):
    """dY of every second non-empty batch times 2^log2 (exact): neighbouring batches then differ by that factor, and one row leaked
    from the larger neighbour is 2^log2 times what the smaller batch's bound allows per row."""
    k = 0
    for s in batches(c):
        if s.stop > s.start:
            if k % 2:
                c.ywide[s] *= np.float32(2.0 ** log2)
            k += 1
    return c


def x_matrix(c):
    """The X operand the kernel sees, [M, K (+1)] float32: gathered rows, segments side by side, the ones column."""
    K = c.nseg * c.Dseg
    x = c.xwide[:, 4:4 + K]
    if c.x_rows is not None:
        x = x[c.x_rows]
    if c.ones:
        x = np.concatenate([x, np.ones((x.shape[0], 1), np.float32)], 1)
    return x


def y_matrix(c):
    return c.ywide[:, 4:4 + c.N]


def batches(c):
    M = c.ywide.shape[0]
    off = [0, M] if c.row_off is None else list(c.row_off)
    return [slice(off[b], off[b + 1]) for b in range(len(off) - 1)]


def reference(c):
    """(want, bound) in float64, [B, Kout, N] (B = 1 without row_off)."""
    X, Y = x_matrix(c).astype(np.float64), y_matrix(c).astype(np.float64)
    want = np.stack([X[s].T @ Y[s] for s in batches(c)])
    bound = np.stack([REL * (np.abs(X[s]).T @ np.abs(Y[s])) + ABS for s in batches(c)])
    return want, bound


def float32_by_rows(c):
    """The same product in float32, one row at a time in row order: the plainest f32 evaluation there is."""
    X, Y = x_matrix(c), y_matrix(c)
    out = []
    for s in batches(c):
        acc = np.zeros((X.shape[1], Y.shape[1]), np.float32)
        for r in range(s.start, s.stop):
            acc += np.outer(X[r], Y[r])
        out.append(acc)
    return np.stack(out)


def worst_ratio(got, want, bound):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / bound))


def assert_within(got, want, bound, what):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bad = ~(err <= bound)                                   # (a NaN is outside every bound)
    if bad.any():
        idx = np.unravel_index(int(np.argmax(np.where(np.isnan(err), np.inf, err / bound))), err.shape)
        raise AssertionError("%s: %d of %d elements outside the bound; worst at %s: got %r want %r bound %.3g (ratio %.3g)"
                             % (what, int(bad.sum()), bad.size, idx, got[idx], want[idx], bound[idx], err[idx] / bound[idx]))
    return worst_ratio(got, want, bound)
