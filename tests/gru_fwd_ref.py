"""Host reference of the fused GRU forward (test infrastructure, not product code; plain numpy, never calls the kernels):

  *  the formula -- the gathered segment sum / mean (chem_tensorflow_sparse.py:198-209) and the TF-1.3 GRUCell (:211-216) -- in
     float64 (`forward`), with `dt=np.float32` the same formula in float32 on the CPU, and `forward_f16x2`, the cell with every
     product operand rounded to two f16 pieces as csrc/ggnn_split.hpp does (kSplitF16x2);
  *  `bounds`: a-priori per-element error bounds of h', r, u, c and `incoming`, built from magnitudes -- the same formulas on
     absolute values.  Nothing in them is fitted to a kernel:
       pre-activations   4e-7 * (sum_k |a_k| |w_k| + |b|)      the project's figure for a K-term f32 product chain (DESIGN.md,
                                                               Tolerances; test_gpu_parity.py::test_gru)
       sigmoid / tanh    + 3e-7 each                           ggnn_gemm.hpp:44-47, the hardware exp2 / rcp epilogues
       passed on with the derivatives: 1/4 for sigmoid, 1 for tanh and ReLU; r's error into the candidate through |h| |Wc_h|; u's
       and c's into h' through |h| + |c| and 1 - u; the gathered segment's own error (slots + 2) * 2^-24 * sum |rows| / denominator
       through |Wg| and |Wc|.  Products and sums of the epilogues (r * h, the blend) add their float32 roundings, 2^-24 each.
  *  the inputs of tests/test_gru_fwd_ref_host.py (CPU) and tests/test_gpu_gru_fwd_cells.py (GPU) -- the host test evaluates on
     exactly what the GPU test feeds the kernels -- and the sweep of ggnn_gru_describe that finds an argument tuple per cell.
     Nothing here knows the dispatch tables: cells are learnt from the library (ggnn_gru_cells, ggnn_gru_describe).

CAP[D] is the factor over the bound at which the GPU test accepts a fused cell (measured on the two-launch route, see the header of
tests/test_gpu_gru_fwd_cells.py); the host test shows that wrong results of eight kinds fail at that factor."""
from __future__ import annotations

import ctypes
import functools
import itertools
from collections import namedtuple

import numpy as np

from variant_kernel_ref import EPS, assert_within  # noqa: F401  (assert_within: the one comparison, re-exported)

SMALL32 = np.float32(1e-7)       # utils.py:8 SMALL_NUMBER as the kernels add it
PRE = 4e-7                       # K-term f32 product chain, relative to sum |a| |w| + |b|
TRANS = 3e-7                     # sigmoid / tanh on v_exp_f32 / v_rcp_f32
# Factor over the a-priori bound the GPU test allows a fused cell, per hidden size: the next power of two above 2 x the worst
# error / bound ratio of the two-launch route (ggnn_gru_gates_f32 + ggnn_gru_candidate_f32) over every case of the GPU test.
# Measured: 0.580 / 0.580 / 0.592 / 0.532 / 0.507 / 0.519 (the table in tests/test_gpu_gru_fwd_cells.py), so 2 x is 1.01 .. 1.18.
CAP = {32: 2.0, 64: 2.0, 100: 2.0, 128: 2.0, 192: 2.0, 256: 2.0}
OUTPUTS = ("h_out", "r", "u", "c", "incoming")
SMALL_V = (1, 15, 16, 17, 63, 65)
E_INVALID, E_UNSUPPORTED = -1, -2
FAMILIES = ("ring", "hot", "wide", "panel", "f32")
FMT_NAMES = {0: "f32", 2: "f16x2", 3: "bf16x3"}
ACTS = {"tanh": 0, "relu": 1}


# ---- inputs -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph(V, T):
    """Adjacency lists [E_t, 2] and the in-degree table [V, T], as tests/test_gpu_gru_issue_diet.py::_graph: ~2.5 random edges per
    node, node 0 receives nothing, node V - 1 receives five messages (one more than the gather's slot heads)."""
    rng = np.random.default_rng(1000 * T + V)
    M = (5 * V) // 2
    types = rng.integers(0, T, M)
    src = rng.integers(0, V, M).astype(np.int32)
    dst = rng.integers(0, V, M).astype(np.int32)
    hub = V - 1
    keep = (dst != 0) & (dst != hub)
    types, src, dst = types[keep], src[keep], dst[keep]
    types = np.concatenate([types, np.arange(5) % T])
    src = np.concatenate([src, rng.integers(0, V, 5).astype(np.int32)])
    dst = np.concatenate([dst, np.full(5, hub, np.int32)])
    adj = tuple(np.stack([src[types == t], dst[types == t]], axis=1).astype(np.int32).reshape(-1, 2) for t in range(T))
    nin = np.zeros((V, T), np.float32)
    for t in range(T):
        np.add.at(nin[:, t], adj[t][:, 1], 1.0)
    assert nin[hub].sum() == 5 and (V == 1 or nin[0].sum() == 0)
    return adj, nin


Case = namedtuple("Case", "D nx V T gather use_avg act res H h Wg bg Wc bc adj nin x_last")


@functools.lru_cache(maxsize=64)
def weights(D, nx):
    """Glorot-scaled weights, gate bias around 1 (what the model initialises to), candidate bias in (-0.5, 0.5)."""
    rng = np.random.default_rng(31 * D + nx)
    K = (nx + 1) * D
    sg, sc = np.sqrt(6.0 / (K + 2 * D)), np.sqrt(6.0 / (K + D))
    return (rng.uniform(-sg, sg, (K, 2 * D)).astype(np.float32), rng.uniform(0.5, 1.5, 2 * D).astype(np.float32),
            rng.uniform(-sc, sc, (K, D)).astype(np.float32), rng.uniform(-0.5, 0.5, D).astype(np.float32))


@functools.lru_cache(maxsize=8)
def _states(D, V, T):
    rng = np.random.default_rng(77 * V + 13 * D + T)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    return u(V, D), (u(V, D), u(V, D)), u(V, max(T, 1) * D), u(V, D)


def make_case(D, nx, V, gather, T=4, use_avg=1, act="tanh"):
    """States, residual inputs and message rows in (-1, 1).  gather: the last input segment is the segment sum / mean of the rows
    H[src, t] over the messages of `graph(V, T)`; plain: it is x_last."""
    h, res, H, x_last = _states(D, V, T if gather else 0)
    Wg, bg, Wc, bc = weights(D, nx)
    adj, nin = graph(V, T) if gather else (None, None)
    return Case(D, nx, V, T if gather else 0, bool(gather), int(use_avg) if gather else 0, act, res[:nx - 1], H if gather else None, h,
                Wg, bg, Wc, bc, adj, nin, None if gather else x_last)


# ---- the formula --------------------------------------------------------------------------------------------------------------
def segment(c, dt=np.float64, rows=None, denominator=None):
    """(incoming, sum |rows| / denominator, slots): the gathered segment, its magnitude and the messages per node."""
    V, D, T = c.V, c.D, c.T
    H = (c.H if rows is None else rows).astype(dt).reshape(V, T, D)
    seg, mag, slots = np.zeros((V, D), dt), np.zeros((V, D)), np.zeros(V)
    for t in range(T):
        np.add.at(seg, c.adj[t][:, 1], H[c.adj[t][:, 0], t])
        np.add.at(mag, c.adj[t][:, 1], np.abs(H[c.adj[t][:, 0], t].astype(np.float64)))
        np.add.at(slots, c.adj[t][:, 1], 1.0)
    if c.use_avg:
        den = c.nin.astype(dt).sum(-1, keepdims=True) + dt(SMALL32) if denominator is None else denominator.astype(dt)
        seg = seg / den
        mag = mag / den.astype(np.float64)
    return seg, mag, slots


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _act(name, x):
    return np.tanh(x) if name == "tanh" else np.maximum(x, 0)


def cell(xs, h, Wg, bg, Wc, bc, act, dt=np.float64, matmul=None):
    """TF-1.3 GRUCell: [r|u] = sigmoid([x|h] Wg + bg); c = act([x | r*h] Wc + bc); h' = u*h + (1-u)*c."""
    mm = matmul or (lambda a, w: a @ w)
    D = h.shape[1]
    x = [s.astype(dt) for s in xs]
    h = h.astype(dt)
    g = _sigmoid(mm(np.concatenate(x + [h], 1), Wg.astype(dt)) + bg.astype(dt))
    r, u = g[:, :D], g[:, D:]
    c = _act(act, mm(np.concatenate(x + [r * h], 1), Wc.astype(dt)) + bc.astype(dt))
    return dict(h_out=u * h + (1 - u) * c, r=r, u=u, c=c)


def forward(c, dt=np.float64, matmul=None, incoming=None):
    """{h_out, r, u, c, incoming} of a case."""
    inc = incoming if incoming is not None else (segment(c, dt)[0] if c.gather else c.x_last.astype(dt))
    out = cell(list(c.res) + [inc], c.h, c.Wg, c.bg, c.Wc, c.bc, c.act, dt, matmul)
    out["incoming"] = inc
    return out


def bounds(c):
    """A-priori error bounds of forward(c)'s five results, float64, from magnitudes."""
    D, nx = c.D, c.nx
    ref = forward(c)
    if c.gather:
        _, mag, slots = segment(c)
        b_inc = (slots[:, None] + 2) * EPS * mag
    else:
        b_inc = np.zeros((c.V, D))
    x = np.concatenate([np.abs(s.astype(np.float64)) for s in c.res] + [np.abs(ref["incoming"])], 1)
    h = np.abs(c.h.astype(np.float64))
    aWg, aWc = np.abs(c.Wg.astype(np.float64)), np.abs(c.Wc.astype(np.float64))
    inc0 = (nx - 1) * D                                                    # first weight row of the gathered segment
    via = (lambda W: b_inc @ W[inc0:inc0 + D]) if c.gather else (lambda W: 0.0)
    b_g = PRE * (np.concatenate([x, h], 1) @ aWg + np.abs(c.bg)) + via(aWg)
    b_g = 0.25 * b_g + TRANS
    b_r, b_u = b_g[:, :D], b_g[:, D:]
    rh = ref["r"] * h
    b_rh = b_r * h + EPS * rh
    b_c = PRE * (np.concatenate([x, rh], 1) @ aWc + np.abs(c.bc)) + via(aWc) + b_rh @ aWc[nx * D:]
    if c.act == "tanh":
        b_c = b_c + TRANS
    u, cc = ref["u"], np.abs(ref["c"])
    b_h = b_u * (h + cc) + (1 - u) * b_c + 3 * EPS * (u * h + (1 - u) * cc)
    return ref, dict(h_out=b_h, r=b_r, u=b_u, c=b_c, incoming=b_inc)


def worst_ratio(got, ref, bound):
    """The largest error / bound of a result, asserting nothing (0 / 0 counts as 0; a non-finite result as infinite)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0.0, 0.0, err / bound).max())


# ---- the operand formats ------------------------------------------------------------------------------------------------------
def _f16_pieces(x):
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def matmul_f16x2(a, w):
    """csrc/ggnn_split.hpp, kSplitF16x2: activations as two f16 pieces, weights x 2^8 as two f16 pieces (round to nearest, the
    residual subtraction exact), THREE products hi*hi + hi*lo + lo*hi accumulated in float32, the sum scaled back by 2^-8."""
    ah, al = _f16_pieces(a.astype(np.float32))
    wh, wl = _f16_pieces(w.astype(np.float32) * np.float32(256.0))
    return ((ah @ wh + (ah @ wl + al @ wh)) * np.float32(1.0 / 256.0)).astype(np.float32)


def _bf16_trunc(x):
    return (x.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def matmul_bf16x2_truncated(a, w):
    """A WRONG format (the host test's corruption): operands cut to two truncated bf16 pieces, 16 bits."""
    def two(x):
        hi = _bf16_trunc(x)
        return hi + _bf16_trunc(x.astype(np.float32) - hi)
    return (two(a) @ two(w)).astype(np.float32)


# ---- the library's selection, swept ------------------------------------------------------------------------------------------
Args = namedtuple("Args", "D nx fmt gather save act use_avg T tickets form")
NFIELD, NOUT = 13, 17
SIZES = (32, 64, 100, 128, 192, 256)
FORMS = (0, 1, 2, 6, 61, 64)
# legs of the GPU test: environment of the process (the split path is what a process without GGNN_MATRIX runs)
LEGS = {"split": {}, "f32": {"GGNN_MATRIX": "f32"}, "f32-nosave": {"GGNN_MATRIX": "f32", "GGNN_GRU_NOSAVE_KERNEL": "1"}}
LEG_VARS = ("GGNN_MATRIX", "GGNN_GRU_NOSAVE_KERNEL", "GGNN_GRU_FORM", "GGNN_GRU_COOP_SMALL")


def table(lib):
    n = lib.ggnn_gru_cells(None, 0)
    buf = (ctypes.c_int32 * (NFIELD * n))()
    assert lib.ggnn_gru_cells(buf, n) == n
    return [tuple(buf[NFIELD * i:NFIELD * (i + 1)]) for i in range(n)]


def describe(lib, a, form=None, matrix_split=-1):
    """(rc, cell, (waves, rows per pass, workgroups per CU, grows to one tile per workgroup)) of ggnn_gru_describe."""
    out = (ctypes.c_int32 * NOUT)()
    rc = lib.ggnn_gru_describe(a.D, a.nx, a.fmt, int(a.gather), int(a.save), ACTS[a.act], int(a.use_avg), a.T, int(a.tickets),
                               a.form if form is None else form, matrix_split, out)
    return rc, tuple(out[:NFIELD]), tuple(out[NFIELD:])


def cell_id(cell):
    fam, D, NX, NW, FORM, FMT, SAVE, SAVEX, GATHER, TK, G4AVG, NTW, HALF = cell
    s = "%s-D%d-nx%d-%s-form%d-%dw" % (FAMILIES[fam], D, NX, FMT_NAMES[FMT], FORM, NW)
    s += "-gather" if GATHER else "-plain"
    s += "-train" if SAVE else "-infer"
    if fam == 1:
        s += "-counter" if TK == 1 else "-static"
    if fam == 2:
        s += "-ntw%d%s" % (NTW, "-half" if HALF else "")
    return s


def sweep(lib):
    """{cell: [Args, ...]} of THIS process (its matrix path and GGNN_GRU_NOSAVE_KERNEL): every argument tuple of the domain the
    library accepts, under the cell it selects.  The first tuple of a cell is its primary case (tanh, mean, static tickets where the
    cell's selection allows them); the others vary activation, aggregation, T and the ticket source."""
    found = {}
    for D, nx, fmt, gather, save, form in itertools.product(SIZES, (1, 2, 3), (2, 3), (1, 0), (0, 1), FORMS):
        variants = itertools.product(("tanh", "relu"), (1, 0), (4, 3), (0, 1)) if gather else \
            itertools.product(("tanh", "relu"), (0,), (0,), (0, 1))
        if not gather and form != FORMS[0]:
            continue                                                       # (a plain launch does not read the form)
        for act, use_avg, T, tickets in variants:
            a = Args(D, nx, fmt, gather, save, act, use_avg, T, tickets, form)
            rc, cell, _ = describe(lib, a)
            if rc == 0:
                found.setdefault(cell, []).append(a)
            else:
                assert rc == E_UNSUPPORTED and gather and D >= 128, (a, rc, lib.ggnn_last_error())
    return found


def large_v(geom, cus):
    """One full round of the cell's workgroups plus 40 rows: thin tail tickets (4-wave forms), the cooperative tail (form 0), a
    second pass with fewer tiles than NTW (wide), a partial last round (panel)."""
    waves, rows, per_cu, _ = geom
    return per_cu * cus * rows + 40
