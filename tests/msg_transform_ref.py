"""Host reference of the compacted message transform (test infrastructure, not product code; plain numpy, never calls the kernels):

  *  the formula, Hc[r] = h[pair_node[r]] @ W[type(r)] (chem_tensorflow_sparse.py:160-164 on the active (node, type) pairs), in
     float64 (`reference`), and `evaluate`, the same rows through any matmul: float32 numpy, and the two operand formats of
     csrc/ggnn_split.hpp emulated in numpy -- gru_fwd_ref.matmul_f16x2 (kSplitF16x2) and `matmul_bf16x3` (kSplitBf16x3);
  *  `bound`: the a-priori per-element bound  PRE * (|h[pair_node[r]]| @ |W_t|) + FLOOR.  PRE is gru_fwd_ref.PRE, the project's
     figure for a K-term f32 product chain; FLOOR = 2^-126, the smallest normal float32 (a result that lands in the denormal range
     may be flushed or rounded on the denormal grid).  Nothing in it is fitted to a kernel;
  *  the inputs of tests/test_msg_transform_ref_host.py (CPU) and tests/test_gpu_msg_transform_cells.py (GPU) -- the host test
     evaluates on exactly what the GPU test feeds the kernels: pairs node-ascending and unique per type over a V just large
     enough, states in (-1, 1), Glorot-scaled weights; `backward_case`: the backward's Z = dHc W_t^T (identity pair list, W^T as
     the weights, gradient-sized operands 1e-6 .. 1e3);
  *  `multipass_rows`: the smallest two-type row counts at which the schedule a `describe` callable reports
     (ggnn_msg_transform_compact_describe) has a wave with at least three tiles and one with exactly two;
  *  `corruptions`: the eight wrong results the comparison must reject, as full output buffers (guard rows included).

CAP[D] is the factor over the bound at which the GPU test accepts a kernel (measured on the dense route, see the header of
tests/test_gpu_msg_transform_cells.py)."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from gru_fwd_ref import PRE, matmul_bf16x2_truncated, matmul_f16x2, worst_ratio  # noqa: F401  (PRE imported, not restated)
from variant_kernel_ref import assert_within

FLOOR = 2.0 ** -126
SIZES = (32, 64, 100, 128, 192, 256)
FMT_NAMES = {0: "f32", 2: "f16x2", 3: "bf16x3"}
F16X2, BF16X3 = 2, 3
# Factor over the a-priori bound the GPU test allows a kernel, per hidden size: the next power of two above 2 x the worst error / bound
# ratio of the dense route (ggnn_msg_transform_f32 gathered at [pair_node, t]) over every case of the GPU test.  Measured: see the table
# in tests/test_gpu_msg_transform_cells.py -- 0.729 / 0.917 / 0.800 / 0.727 / 0.821 / 0.815, so 2 x is 1.45 .. 1.83.
CAP = {32: 2.0, 64: 2.0, 100: 2.0, 128: 2.0, 192: 2.0, 256: 2.0}
GUARD = 33                                  # sentinel rows behind type_row_off[T]: two tiles and a row
SENTINEL = np.float32(-1.25e30)
WAVES = 8                                   # waves of a workgroup: the tile stride of a type that has ONE workgroup
# the instantiations: whole-block D x {f32, bf16x3, f16x2}, ring D x {bf16x3, f16x2}, stationary D x {bf16x3, f32}
INSTANTIATIONS = tuple(["whole-block-D%d-%s" % (D, f) for D in (32, 64, 100) for f in ("f32", "bf16x3", "f16x2")] +
                       ["ring-D%d-%s" % (D, f) for D in (128, 192, 256) for f in ("bf16x3", "f16x2")] +
                       ["stationary-D%d-%s" % (D, f) for D in (128, 192, 256) for f in ("bf16x3", "f32")])
# legs of the GPU test: (environment of the process, the one family the leg's own process keeps -- None: all it selects)
LEGS = {"split": ({}, None), "f32": ({"GGNN_MATRIX": "f32"}, None), "split-stationary": ({"GGNN_PANEL_TRANSFORM": "0"}, "stationary")}
LEG_VARS = ("GGNN_MATRIX", "GGNN_PANEL_TRANSFORM")

# rows per type of the small cases (every case at every hidden size)
_T64 = [0] * 64
for _t, _n in ((3, 1), (4, 1), (17, 16), (31, 1), (62, 1)):
    _T64[_t] = _n
SMALL_CASES = {
    "rows": (1, 15, 16, 17, 127, 128, 129),              # one row, a tile less / exactly / plus one row, eight tiles -1 / 0 / +1 row
    "empty": (0, 17, 0, 0, 129, 0),                      # empty types first, in the middle (two in a row) and last
    "t1": (129,),
    "t1-one-row": (1,),
    "t64": tuple(_T64),                                  # the linear type scan over equal offsets; the last type empty
}

Case = namedtuple("Case", "name D T V row_off pair_node h W")


def instantiation(family, D, fmt):
    return "%s-D%d-%s" % (family, D, FMT_NAMES[fmt])


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _seed(name, D, rows):
    return (sum(map(ord, name)) * 1000003 + 31 * D + 7 * sum(rows) + len(rows)) % (2 ** 31 - 1)


def make_case(name, D, rows):
    """Pairs node-ascending and unique per type over V = the largest type's rows + an eighth + 3 (so even that type skips nodes),
    states in (-1, 1), weights Glorot-scaled and different for every type."""
    rows = tuple(int(r) for r in rows)
    rng = np.random.default_rng(_seed(name, D, rows))
    T = len(rows)
    V = max(rows) + max(rows) // 8 + 3
    row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    pn = np.concatenate([np.sort(rng.choice(V, n, replace=False)) for n in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    s = np.sqrt(6.0 / (2 * D))
    h = rng.uniform(-1, 1, (V, D)).astype(np.float32)
    W = rng.uniform(-s, s, (T, D, D)).astype(np.float32)
    return Case(name, D, T, V, row_off, pn, h, W)


@functools.lru_cache(maxsize=64)
def small_case(name, D):
    return make_case(name, D, SMALL_CASES[name])


BACKWARD_ROWS = (129, 0, 300, 17)


@functools.lru_cache(maxsize=8)
def backward_case(D):
    """(case, Wfwd): the backward's use.  case.h = dHc [R, D], case.pair_node = arange(R) (V = R), case.W[t] = Wfwd[t]^T contiguous --
    what the raw-weight route is given; the packed route packs Wfwd's transposes itself.
    dHc: every ROW has a scale of its own, 10^U(-6, 3) (row 0: 1e-6, row 1: 1e3), its elements U(-1, 1) times that -- the gradient
    rows of different nodes and graphs differ by orders of magnitude, the elements of one row do not.  (Magnitudes drawn
    log-uniformly per ELEMENT make a product a sum of a few dominant terms that does not cancel while every partial sum is rounded at
    full scale: a plain float32 chain over K = 32 terms then reaches 7 roundings of one sign, 4.2e-7 of sum |a||w|, past the
    constant PRE -- which is the project's figure for operands of one scale, not the worst case K 2^-24.  The host test requires the
    float32 evaluation inside factor 1 on every case, so such a case is no valid one.)"""
    rows = BACKWARD_ROWS
    rng = np.random.default_rng(_seed("backward", D, rows))
    T, R = len(rows), sum(rows)
    s = np.sqrt(6.0 / (2 * D))
    Wf = rng.uniform(-s, s, (T, D, D)).astype(np.float32)
    scale = 10.0 ** rng.uniform(-6, 3, (R, 1))
    scale[0], scale[1] = 1e-6, 1e3
    dHc = (rng.uniform(-1, 1, (R, D)) * scale).astype(np.float32)
    row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    return Case("backward", D, T, R, row_off, np.arange(R, dtype=np.int32), dHc, np.ascontiguousarray(Wf.transpose(0, 2, 1))), Wf


# ---- the formula --------------------------------------------------------------------------------------------------------------
def evaluate(c, matmul, W=None):
    """[R, D] float64: the rows of every type through matmul(h rows, W[t])."""
    W = c.W if W is None else W
    R = int(c.row_off[-1])
    out = np.zeros((R, c.D))
    for t in range(c.T):
        a, b = int(c.row_off[t]), int(c.row_off[t + 1])
        if b > a:
            out[a:b] = matmul(c.h[c.pair_node[a:b]], W[t])
    return out


def reference(c):
    return evaluate(c, lambda a, w: a.astype(np.float64) @ w.astype(np.float64))


def bound(c):
    return PRE * evaluate(c, lambda a, w: np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64))) + FLOOR


def matmul_f32(a, w):
    return a.astype(np.float32) @ w.astype(np.float32)


def _bf16_pieces(x):
    """csrc/ggnn_split.hpp, kSplitBf16x3: three pieces cut by TRUNCATION, 8 significand bits each, hi + mid + lo == x exactly."""
    trunc = lambda v: (np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    x = np.ascontiguousarray(x, np.float32)
    hi = trunc(x)
    r = x - hi
    mid = trunc(r)
    return hi, mid, r - mid


def matmul_bf16x3(a, w):
    """SIX of the nine piece products, a_hi w_hi + (a_hi w_mid + a_mid w_hi) + (a_mid w_mid + a_hi w_lo + a_lo w_hi), accumulated in
    float32; the three smallest (below 2^-21 |a w| together) are dropped."""
    ah, am, al = _bf16_pieces(a)
    wh, wm, wl = _bf16_pieces(w)
    return (ah @ wh + ((ah @ wm + am @ wh) + (am @ wm + (ah @ wl + al @ wh)))).astype(np.float32)


FORMATS = {"f32": matmul_f32, "bf16x3": matmul_bf16x3, "f16x2": matmul_f16x2}


# ---- the comparison -----------------------------------------------------------------------------------------------------------
def with_guard(rows):
    """The output buffer as the GPU test allocates it: [R + GUARD, D], the guard rows (and, before a launch, all rows) SENTINEL."""
    out = np.full((rows.shape[0] + GUARD, rows.shape[1]), SENTINEL, np.float32)
    out[:rows.shape[0]] = rows
    return out


def check(buf, ref, bnd, factor, what):
    """buf [R + GUARD, D] float32: every row of every type inside factor x bound, every guard row bit-unchanged.  -> worst ratio."""
    R = ref.shape[0]
    assert buf.shape == (R + GUARD, ref.shape[1]) and buf.dtype == np.float32, (buf.shape, buf.dtype)
    touched = np.argwhere(buf[R:].view(np.uint32) != SENTINEL.view(np.uint32))
    assert not len(touched), "%s: guard row %d (row %d of the buffer), column %d was written: %r" % (
        what, touched[0][0], R + touched[0][0], touched[0][1], buf[R + touched[0][0], touched[0][1]])
    return assert_within(buf[:R], ref, bnd, factor, what)


# ---- the multi-pass regime ------------------------------------------------------------------------------------------------------
def walks(types):
    """(some wave walks >= 3 tiles, some wave walks exactly 2, some type has waves one tile apart) of a describe's per-type
    (workgroups, most tiles a wave walks, fewest): the waves of a type walk `most` or `fewest` = most - 1 tiles."""
    return (any(mx >= 3 for _, mx, _ in types), any(mn <= 2 <= mx for _, mx, mn in types), any(mx - mn == 1 for _, mx, mn in types))


def multipass_rows(describe, small, limit):
    """(big, small) rows of two types: `small` is fixed (ragged; little enough that its share of the workgroups is one), `big` =
    16 k + 7 is the smallest for which describe((0, big, big + small))['types'] has a wave with >= 3 tiles and one with exactly 2.
    Sizes come from the query alone -- no CU count is known here."""
    for k in range(8, limit // 16):
        big = 16 * k + 7
        if all(walks(describe((0, big, big + small))["types"])):
            return big, small
    raise AssertionError("no multi-pass schedule with at most %d rows" % limit)


def strides(d, D):
    """Per type, the tile stride of its waves in a describe result: its workgroups x waves (stationary: per column panel)."""
    return [wg // (D // 64 if d["family"] == "stationary" else 1) * d["waves"] for wg, _, _ in d["types"]]


# ---- wrong results --------------------------------------------------------------------------------------------------------------
def corruptions(c, ref, strides=None):
    """{what: [R + GUARD, D] float32 buffer} -- the eight wrong results, each only where the case has room for it.
    strides[t]: the tile stride of type t's waves (default: one workgroup of WAVES waves)."""
    D, T, R = c.D, c.T, int(c.row_off[-1])
    good = ref.astype(np.float32)
    rows = np.diff(c.row_off)
    strides = [WAVES] * T if strides is None else strides
    out = {}
    # 1. a tile holding the rows of the tile one stride earlier (the prefetched fragment was not advanced): the LAST tile of every type
    #    with more tiles than waves
    for t in range(T):
        n_wt = (int(rows[t]) + 15) // 16
        if strides[t] and n_wt > strides[t]:
            a = int(c.row_off[t])
            k = n_wt - 1
            dst = np.arange(a + 16 * k, int(c.row_off[t + 1]))
            src = dst - 16 * strides[t]
            w = good.copy()
            w[dst] = (c.h[c.pair_node[src]].astype(np.float64) @ c.W[t].astype(np.float64)).astype(np.float32)
            out["stale prefetch (type %d)" % t] = with_guard(w)
    # 2. a type multiplied by its neighbour's weights
    live = [t for t in range(T) if rows[t]]
    if T > 1 and live:
        Wn = c.W.copy()
        Wn[live[0]] = c.W[(live[0] + 1) % T]
        out["neighbour's weights"] = with_guard(evaluate(c, lambda a, w: a.astype(np.float64) @ w.astype(np.float64), Wn).astype(np.float32))
    # 3. W transposed
    out["W transposed"] = with_guard(evaluate(c, lambda a, w: a.astype(np.float64) @ w.astype(np.float64).T).astype(np.float32))
    # 4. the K remainder dropped (k = 96 .. 99 at D = 100)
    if D % 16:
        K = D // 16 * 16
        out["K remainder dropped"] = with_guard(evaluate(c, lambda a, w: a[:, :K].astype(np.float64) @ w[:K].astype(np.float64)).astype(np.float32))
    # 5. the low operand piece dropped (two truncated bf16 pieces of three)
    out["low piece dropped"] = with_guard(evaluate(c, matmul_bf16x2_truncated).astype(np.float32))
    # 6. a missing acc_scale (the f16x2 accumulators hold 2^8 x the sums)
    out["acc_scale missing"] = with_guard(good * np.float32(256.0))
    # 7. a tail tile's clamped lanes (row_of -> row_end - 1) store: the row after the type's end receives the type's last row --
    #    the next type's first row, and for the last type with rows the first guard row
    ragged = [t for t in live if rows[t] % 16]
    for t in ragged[-1:]:
        w = with_guard(good)
        w[int(c.row_off[t + 1])] = good[int(c.row_off[t + 1]) - 1]
        out["clamped row stored past the last type"] = w
    for t in ragged[:1]:
        if int(c.row_off[t + 1]) < R:
            w = with_guard(good)
            w[int(c.row_off[t + 1])] = good[int(c.row_off[t + 1]) - 1]
            out["clamped row stored into the next type"] = w
    # 8. the last column tile dropped at D = 100 (columns 96 .. 99 keep what the buffer held)
    if D % 16:
        w = with_guard(good)
        w[:R, D // 16 * 16:] = SENTINEL
        out["last column tile dropped"] = w
    return out
