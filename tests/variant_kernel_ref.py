"""Kernel-level references for the NON-DEFAULT switches of chem_tensorflow_sparse.py (test infrastructure, not product code):
propagation attention (:147-149, 170-196), BasicRNNCell / CudnnCompatibleGRUCell (:105-110), the mean / bias aggregation
(:198-209) and the generic backward kernels behind them.

For every operation there are two functions, both plain numpy and neither calling the package:

  *  the formula, restated from chem_tensorflow_sparse.py and the kernel comments of csrc/ggnn_scatter.hip, ggnn_gemm.hpp and
     ggnn_bwd.hip.  `dt=np.float64` (the default) is the reference; `dt=np.float32` evaluates the same formula in float32 on the
     CPU, which tests/test_variant_kernel_ref_host.py holds inside the bound at factor 1.
  *  `*_bound`: an a-priori per-element error bound, shaped like the result, computed in float64 from ABSOLUTE values of the
     inputs.  Such a bound holds for any correct float32 evaluation in any summation order; nothing in it is fitted to a kernel.

`assert_within(got, ref, bound, factor, what)` is the one comparison.  The GPU tests use factor 2: factor 1 is the a-priori bound,
the 2 covers the hardware v_exp_f32 / v_rcp_f32 forms of sigmoid / tanh in ggnn_gemm.hpp (about 1 ulp each).

The input generators (`*_inputs`, `build_graph`) live here too, so that the host test evaluates float32 on exactly the inputs the
GPU test feeds the kernels.
"""
from __future__ import annotations

import math

import numpy as np

EPS = 2.0 ** -24                 # unit roundoff of float32
SMALL = 1e-7                     # utils.py:8 SMALL_NUMBER
HUB_IN = 70                      # messages into the hub node: more than one 64-lane slot read
RATIOS = {}                      # what (up to its "[") -> largest error / bound of the comparisons that passed; tools/variant_kernel_accuracy.py writes it into profiles/


# ---- the comparison -----------------------------------------------------------------------------------------------------------
def assert_within(got, ref, bound, factor, what):
    """|got - ref| <= factor * bound for every element (and got finite); reports the worst element otherwise.
    Returns the largest error / bound ratio (0 / 0 counts as 0: an exact result with a zero bound passes)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, "%s: shape %s, reference %s" % (what, got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    err = np.where(np.isfinite(got), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    worst = float(ratio.max())
    bad = err > factor * bound
    if bad.any():
        flat = int(np.argmax(np.where(bad, ratio, -1.0)))
        idx = np.unravel_index(flat, ref.shape)
        row = idx[0] if idx else 0
        col = idx[1] if len(idx) > 1 else 0
        raise AssertionError(
            "%s: %d of %d elements outside %g x bound; worst at row %d, column %d: got %.9g, reference %.9g, error %.3e, "
            "bound %.3e (ratio %.3g)" % (what, int(bad.sum()), ref.size, factor, row, col, got[idx], ref[idx], err[idx],
                                          bound[idx], ratio[idx]))
    key = what.split("[")[0]
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    return worst


# ---- the graph every scatter test runs on -------------------------------------------------------------------------------------
def build_graph(V, T, seed):
    """-> (adjacency lists [E_t, 2] int32 (src, dst) per edge type, nin [V, T] float32, info).

    Fixed features, at every (V, T):
      * node 0 receives nothing;
      * node V-1 is a hub with exactly HUB_IN = 70 incoming messages spread over all populated types, one a self-loop;
      * the triple (src V-2, dst 1, last type) occurs three times;
      * node 2 has a self-loop;
      * edge type 1 is empty when T >= 3;
      * about 3 random edges per node besides (targets 1 .. V-2), and every list is shuffled, so message ids are not in
        target order.
    V = 1: all HUB_IN edges are self-loops on node 0 (the hub) and the "node 0 receives nothing" feature is dropped."""
    assert V == 1 or V >= 4
    rng = np.random.default_rng(seed)
    empty = 1 if T >= 3 else None
    live = [t for t in range(T) if t != empty]
    hub = V - 1
    edges = []
    if V == 1:
        edges += [(0, 0, live[k % len(live)]) for k in range(HUB_IN)]
        tripled = (0, 0, live[-1])
    else:
        edges.append((hub, hub, live[0]))
        edges += [(int(rng.integers(0, V - 1)), hub, live[k % len(live)]) for k in range(1, HUB_IN)]
        tripled = (V - 2, 1, live[-1])
        edges += [tripled] * 3
        edges.append((2, 2, live[0]))
        for _ in range(3 * V):
            edges.append((int(rng.integers(0, V)), int(rng.integers(1, V - 1)), live[int(rng.integers(0, len(live)))]))
    adj = []
    for t in range(T):
        a = np.array([(s, d) for s, d, tt in edges if tt == t], dtype=np.int32).reshape(-1, 2)
        adj.append(a[rng.permutation(len(a))])
    nin = np.zeros((V, T), np.float32)
    for t in range(T):
        np.add.at(nin[:, t], adj[t][:, 1], 1.0)
    return adj, nin, {"hub": hub, "empty_type": empty, "tripled": tripled}


def messages(adj):
    """(src, dst, type) per message id, type-major like chem_tensorflow_sparse.py:124-129,168."""
    src = np.concatenate([a[:, 0] for a in adj]).astype(np.int64)
    dst = np.concatenate([a[:, 1] for a in adj]).astype(np.int64)
    typ = np.concatenate([np.full(len(a), t, np.int64) for t, a in enumerate(adj)])
    return src, dst, typ


# ---- propagation attention ----------------------------------------------------------------------------------------------------
def _softmax(h, adj, factors, dt):
    """Scores and attention weights per message (:170-196): p = <h[src], h[dst]>, s = p f[type],
    a = exp(s - max_v) / (sum_v exp(s - max_v) + 1e-7), max / sum over the messages into the same target."""
    src, dst, typ = messages(adj)
    V = h.shape[0]
    hh = h.astype(dt)
    p = (hh[src] * hh[dst]).sum(-1, dtype=dt)
    s = p * factors.astype(dt)[typ]
    m = np.full(V, -np.inf, dt)
    np.maximum.at(m, dst, s)
    e = np.exp(s - m[dst])
    S = np.zeros(V, dt)
    np.add.at(S, dst, e)
    a = e / (S[dst] + dt(SMALL))
    return src, dst, typ, p, s, m, S, a


def _score_terms(h, adj, factors):
    """Per message, in float64: P = sum_i |h[src,i] h[dst,i]|, and per target: in-degree n_v, delta_v = max_e P_e |f[t_e]|."""
    src, dst, typ = messages(adj)
    V = h.shape[0]
    h64 = np.abs(h.astype(np.float64))
    P = (h64[src] * h64[dst]).sum(-1)
    n = np.zeros(V)
    np.add.at(n, dst, 1.0)
    delta = np.zeros(V)
    np.maximum.at(delta, dst, P * np.abs(factors.astype(np.float64))[typ])
    return P, n, delta


def attn_forward(h, Hrows, adj, factors, nin=None, bias=None, use_avg=False, dt=np.float64):
    """incoming[v] = (sum_e a_e Hrows[src_e * T + t_e] [+ nin[v] @ bias]) [/ (sum_t nin[v,t] + 1e-7)]   (:170-209).
    Hrows [V*T, D]: the transformed states, row src*T + t = h[src] W_t."""
    src, dst, typ, p, s, m, S, a = _softmax(h, adj, factors, dt)
    T = len(adj)
    V, D = h.shape
    out = np.zeros((V, D), dt)
    np.add.at(out, dst, a[:, None] * Hrows.astype(dt)[src * T + typ])
    if bias is not None:
        out = out + nin.astype(dt) @ bias.astype(dt)
    if use_avg:
        out = out / (nin.astype(dt).sum(-1, keepdims=True, dtype=dt) + dt(SMALL))
    return out


def attn_forward_bound(h, Hrows, adj, factors, nin=None, bias=None, use_avg=False):
    """B[v,d] = eps (n_v + 4 + 2 (D + 2) delta_v) sum_e a_e |H[g_e, d]|:  the score is a D-term dot times a factor, so it and the
    max it is shifted by each carry (D + 2) eps delta_v; that perturbs exp(s - max) by 2 (D + 2) delta_v eps relatively;
    the n_v-term sums, the exp, the product and the division account for n_v + 4.  The bias term adds
    eps (T + 1) sum_t nin |bias|; mean aggregation scales everything by 1 / (deg + 1e-7)."""
    src, dst, typ, p, s, m, S, a = _softmax(h, adj, factors, np.float64)
    P, n, delta = _score_terms(h, adj, factors)
    T = len(adj)
    V, D = h.shape
    mag = np.zeros((V, D))
    np.add.at(mag, dst, a[:, None] * np.abs(Hrows.astype(np.float64))[src * T + typ])
    B = EPS * (n + 4 + 2 * (D + 2) * delta)[:, None] * mag
    if bias is not None:
        B = B + EPS * (T + 1) * (nin.astype(np.float64) @ np.abs(bias.astype(np.float64)))
    if use_avg:
        B = B / (nin.astype(np.float64).sum(-1, keepdims=True) + SMALL)
    return B


def attn_backward(h, Hrows, d, adj, factors, dt=np.float64):
    """What autodiff derives from :170-196 for d = dL/d(sum_e a_e H[g_e]) [V, D]:
        da_e = <H[g_e], d[v]>,   ds_e = a_e (da_e - sum_k a_k da_k)  [- (1e-7 / (S + 1e-7)) sum_k a_k da_k on the arg-max score]
        coef_a[m] = a_e,  coef_s[m] = ds_e f[t_e],  dfac[m] = ds_e p_e,  d factor[t] = sum of dfac over the messages of type t
        dh[v] += sum_e coef_s_e h[src_e]  (target side),   dh[u] += sum over the messages leaving u of coef_s_m h[dst_m]
    The bracketed term is the gradient through the max shift: with the 1e-7 in the denominator a_e is not exactly invariant to the
    shift, and both TensorFlow and torch differentiate the max (ties share it evenly).  The kernel treats the shift as a constant;
    attn_backward_bounds carries the difference."""
    src, dst, typ, p, s, m, S, a = _softmax(h, adj, factors, dt)
    T = len(adj)
    V, D = h.shape
    hh = h.astype(dt)
    f = factors.astype(dt)
    da = (Hrows.astype(dt)[src * T + typ] * d.astype(dt)[dst]).sum(-1, dtype=dt)
    t1 = np.zeros(V, dt)
    np.add.at(t1, dst, a * da)
    ds = a * (da - t1[dst])
    tie = (s == m[dst])
    ntie = np.zeros(V, dt)
    np.add.at(ntie, dst, tie.astype(dt))
    ds = ds - np.where(tie, (dt(SMALL) / (S[dst] + dt(SMALL))) * t1[dst] / np.maximum(ntie[dst], dt(1)), dt(0))
    coef_s = ds * f[typ]
    dfac = ds * p
    dfactor = np.zeros(T, dt)
    np.add.at(dfactor, typ, dfac)
    dh_t = np.zeros((V, D), dt)
    np.add.at(dh_t, dst, coef_s[:, None] * hh[src])
    dh_s = np.zeros((V, D), dt)
    np.add.at(dh_s, src, coef_s[:, None] * hh[dst])
    return {"coef_a": a, "coef_s": coef_s, "dfac": dfac, "dfactor": dfactor, "dh_target": dh_t, "dh_source": dh_s}


def attn_backward_bounds(h, Hrows, d, adj, factors, dh_prefill=None):
    """Bounds for coef_a [M], coef_s [M], d factor [T] and the combined dh [V, D] (prefill + target side + source side).

    rho_v = eps (n_v + 4 + 2 (D + 2) delta_v) is the relative error of a_e (attn_forward_bound).  da_e is a D-term dot:
    (D + 1) eps DA_e with DA_e = sum_i |H[g_e,i] d[v,i]|.  t1 = sum_k a_k da_k inherits rho_v A1 + (D + 1) eps A2 + (n_v + 1) eps A1
    with A1 = sum_k a_k |da_k|, A2 = sum_k a_k DA_k.  ds_e = a_e (da_e - t1) cancels, so every relative term multiplies
    a_e (|da_e| + A1) instead of |ds_e|:
        E_ds = a_e [ (rho_v + 2 eps) (|da_e| + A1) + (D + 1) eps (DA_e + A2) + (rho_v + (n_v + 1) eps) A1 ]
               + [arg-max messages] (1e-7 / (S + 1e-7)) A1 / ties     (the max-shift gradient the kernel leaves out, see attn_backward)
    coef_s = ds f and dfac = ds p add one product rounding each, dfac also the (D + 1) eps P_e of p.  The sums (n terms) add
    (n + 2) eps times the sum of magnitudes, the type reduction the range_sum bound."""
    src, dst, typ, p, s, m, S, a = _softmax(h, adj, factors, np.float64)
    P, n, delta = _score_terms(h, adj, factors)
    T = len(adj)
    V, D = h.shape
    h64 = np.abs(h.astype(np.float64))
    f = np.abs(factors.astype(np.float64))[typ]
    Hg = Hrows.astype(np.float64)[src * T + typ]
    dv = d.astype(np.float64)[dst]
    da = np.abs((Hg * dv).sum(-1))
    DA = (np.abs(Hg) * np.abs(dv)).sum(-1)
    A1 = np.zeros(V)
    np.add.at(A1, dst, a * da)
    A2 = np.zeros(V)
    np.add.at(A2, dst, a * DA)
    rho = EPS * (n + 4 + 2 * (D + 2) * delta)
    r, nn, a1, a2 = rho[dst], n[dst], A1[dst], A2[dst]
    mag = a * (da + a1)                                     # stands for |ds_e|
    tie = (s == m[dst])
    ntie = np.zeros(V)
    np.add.at(ntie, dst, tie.astype(np.float64))
    E_ds = a * ((r + 2 * EPS) * (da + a1) + (D + 1) * EPS * (DA + a2) + (r + (nn + 1) * EPS) * a1)
    E_ds = E_ds + np.where(tie, (SMALL / (S[dst] + SMALL)) * a1 / np.maximum(ntie[dst], 1.0), 0.0)
    E_cs = f * (E_ds + EPS * mag)
    E_df = np.abs(p) * E_ds + mag * ((D + 1) * EPS * P + EPS * np.abs(p))
    B_fac = np.zeros(T)
    np.add.at(B_fac, typ, E_df)
    df_mag = np.zeros(T)
    np.add.at(df_mag, typ, mag * np.abs(p))
    cnt = np.array([len(x) for x in adj], dtype=np.float64)
    B_fac = B_fac + (np.ceil(cnt / 256) + 10) * EPS * df_mag
    nout = np.zeros(V)
    np.add.at(nout, src, 1.0)
    B_dh = np.zeros((V, D))
    np.add.at(B_dh, dst, E_cs[:, None] * h64[src])
    np.add.at(B_dh, src, E_cs[:, None] * h64[dst])
    mag_t = np.zeros((V, D))
    np.add.at(mag_t, dst, (f * mag)[:, None] * h64[src])
    mag_s = np.zeros((V, D))
    np.add.at(mag_s, src, (f * mag)[:, None] * h64[dst])
    pre = np.zeros((V, D)) if dh_prefill is None else np.abs(dh_prefill.astype(np.float64))
    B_dh = B_dh + (n + 2)[:, None] * EPS * mag_t + (nout + 2)[:, None] * EPS * mag_s + 2 * EPS * (pre + mag_t + mag_s)
    return {"coef_a": rho[dst] * a, "coef_s": E_cs, "dfactor": B_fac, "dh": B_dh}


def attn_inputs(D, V, T, seed, saturate=False):
    """Inputs of the attention tests: states with |h|^2 ~ 8 (self-loop scores up to ~8, the others a few units), type factors
    of mixed sign with one exact 0 on a populated type (T >= 3), an upstream gradient and a prefilled dh.
    saturate: the states are scaled so that the hub's scores span more than 90 (exp of an unshifted score overflows float32)."""
    adj, nin, info = build_graph(V, T, seed)
    rng = np.random.default_rng(seed + 1000)
    scale = math.sqrt(24.0 / D) * (4.5 if saturate else 1.0)
    h = (rng.uniform(-1, 1, (V, D)) * scale).astype(np.float32)
    W = (rng.uniform(-1, 1, (T, D, D)) / math.sqrt(D)).astype(np.float32)
    factors = np.array({1: [-0.6], 3: [0.0, 0.5, -0.8], 4: [0.7, 0.4, 0.0, -0.9]}[T], np.float32)
    if saturate:
        factors = np.abs(factors) + np.float32(0.7)
    bias = (rng.normal(size=(T, D)) * 0.1).astype(np.float32)
    d = rng.normal(size=(V, D)).astype(np.float32)
    dh0 = rng.normal(size=(V, D)).astype(np.float32)
    return {"adj": adj, "nin": nin, "info": info, "h": h, "W": W, "factors": factors, "bias": bias, "d": d, "dh0": dh0}


def transform_rows(h, W, dt=np.float64):
    """Hrows [V*T, D], row v*T + t = h[v] @ W[t]   (:160-164)."""
    V, D = h.shape
    return np.einsum("vd,tde->vte", h.astype(dt), W.astype(dt)).reshape(V * W.shape[0], D)


# ---- sums ---------------------------------------------------------------------------------------------------------------------
def weighted_segment_sum(rows, row_ptr, gather_row, weight_id, weights, out0=None, dt=np.float64):
    """out[s] (+)= sum over the slots of segment s of weights[weight_id[slot]] * rows[gather_row[slot]]."""
    nseg = len(row_ptr) - 1
    seg = np.repeat(np.arange(nseg), np.diff(row_ptr))
    out = np.zeros((nseg, rows.shape[1]), dt) if out0 is None else out0.astype(dt).copy()
    np.add.at(out, seg, weights.astype(dt)[weight_id][:, None] * rows.astype(dt)[gather_row])
    return out


def weighted_segment_sum_bound(rows, row_ptr, gather_row, weight_id, weights, out0=None):
    """(n_slots + 2) eps (sum |w| |row| + |prefill|): n_slots - 1 additions, one product rounding per term, the accumulate.
    The prefill stands under the same factor as the sum (one more term of it), which the plain segment-sum bound has not."""
    nseg = len(row_ptr) - 1
    n = np.diff(row_ptr).astype(np.float64)
    seg = np.repeat(np.arange(nseg), np.diff(row_ptr))
    mag = np.zeros((nseg, rows.shape[1])) if out0 is None else np.abs(out0.astype(np.float64))
    np.add.at(mag, seg, np.abs(weights.astype(np.float64))[weight_id][:, None] * np.abs(rows.astype(np.float64))[gather_row])
    return (n + 2)[:, None] * EPS * mag


def wss_inputs(D, nseg, seed):
    """Segments with duplicates: one empty segment (nseg > 1), one with HUB_IN slots, 0..5 slots otherwise."""
    rng = np.random.default_rng(seed)
    R, NW = 23, 31
    counts = rng.integers(0, 6, nseg)
    counts[nseg - 1] = HUB_IN
    if nseg > 1:
        counts[nseg // 2] = 0
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ns = int(row_ptr[-1])
    return {"rows": rng.normal(size=(R, D)).astype(np.float32), "row_ptr": row_ptr,
            "gather_row": rng.integers(0, R, ns).astype(np.int32), "weight_id": rng.integers(0, NW, ns).astype(np.int32),
            "weights": rng.normal(size=NW).astype(np.float32), "out0": rng.normal(size=(nseg, D)).astype(np.float32)}


def range_sum(values, offsets, dt=np.float64):
    v = values.astype(dt)
    return np.array([v[offsets[b]:offsets[b + 1]].sum(dtype=dt) for b in range(len(offsets) - 1)], dtype=dt)


def range_sum_bound(values, offsets):
    """(ceil(len / 256) + 10) eps sum |values|: ceil(len / 256) strided additions per thread and an 8-level tree."""
    v = np.abs(values.astype(np.float64))
    return np.array([(math.ceil((offsets[b + 1] - offsets[b]) / 256) + 10) * EPS * v[offsets[b]:offsets[b + 1]].sum()
                     for b in range(len(offsets) - 1)])


RANGE_LENGTHS = (0, 1, 255, 256, 257, 100003)


def range_inputs(seed, lengths=RANGE_LENGTHS):
    rng = np.random.default_rng(seed)
    offsets = [0] + [int(x) for x in np.cumsum(lengths)]
    return rng.normal(size=offsets[-1]).astype(np.float32), offsets


def range_inputs_64(seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 600, 64)
    lengths[7] = 0
    return range_inputs(seed + 1, tuple(int(x) for x in lengths))


# ---- GEMM-based operations ----------------------------------------------------------------------------------------------------
def gemm_atol(A, W):
    """The project's bound for its f32-MFMA products (tests/test_gpu_gru_issue_diet.py, test_gpu_parity.py::test_gru), per
    element instead of its max:  max(3e-6, 4e-7 (|A| @ |W|)).  RTOL of the result comes on top."""
    return np.maximum(3e-6, 4e-7 * (np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64))))


RTOL = 1e-5


def _act(name, x):
    return np.tanh(x) if name == "tanh" else np.maximum(x, x.dtype.type(0))


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def rnn(xs, h, W, b, activation, dt=np.float64):
    """BasicRNNCell (:109-110): act([x | h] W + b)."""
    A = np.concatenate(list(xs) + [h], axis=1).astype(dt)
    return _act(activation, A @ W.astype(dt) + b.astype(dt))


def rnn_bound(xs, h, W, b, activation):
    """tanh and relu are 1-Lipschitz: the product's bound passes through times 1, plus RTOL of the output.  Beyond the
    project's product bound: eps |b| for the rounding of the bias addition (it matters on the b = -100 column only)."""
    A = np.concatenate(list(xs) + [h], axis=1)
    return gemm_atol(A, W) + EPS * np.abs(b.astype(np.float64)) + RTOL * np.abs(rnn(xs, h, W, b, activation))


def cudnn_gru(xs, h, Wg, bg, Wcx, bcx, Wch, bch, dt=np.float64):
    """CudnnCompatibleGRUCell (:105-108): [r|u] = sigmoid([x|h] Wg + bg); hc = h Wch + bch; c = tanh(x Wcx + bcx + r hc);
    h' = u h + (1 - u) c.  -> (h', r, u, c, hc)"""
    D = h.shape[1]
    x = np.concatenate(list(xs), axis=1).astype(dt)
    hh = h.astype(dt)
    g = _sigmoid(np.concatenate([x, hh], axis=1) @ Wg.astype(dt) + bg.astype(dt))
    r, u = g[:, :D], g[:, D:]
    hc = hh @ Wch.astype(dt) + bch.astype(dt)
    c = np.tanh(x @ Wcx.astype(dt) + bcx.astype(dt) + r * hc)
    return u * hh + (1 - u) * c, r, u, c, hc


def cudnn_gru_bounds(xs, h, Wg, bg, Wcx, bcx, Wch, bch):
    """The product bound through the epilogues: times 1 through sigmoid / tanh, times the other factor through a product."""
    D = h.shape[1]
    out, r, u, c, hc = cudnn_gru(xs, h, Wg, bg, Wcx, bcx, Wch, bch)
    x = np.concatenate(list(xs), axis=1)
    Bg = gemm_atol(np.concatenate([x, h], axis=1), Wg) + EPS * np.abs(bg.astype(np.float64))
    Br, Bu = Bg[:, :D] + RTOL * r, Bg[:, D:] + RTOL * u
    Bhc = gemm_atol(h, Wch) + EPS * np.abs(bch.astype(np.float64)) + RTOL * np.abs(hc)
    Bpre = gemm_atol(x, Wcx) + EPS * np.abs(bcx.astype(np.float64)) + r * Bhc + np.abs(hc) * Br + 2 * EPS * np.abs(r * hc)
    Bc = Bpre + RTOL * np.abs(c)
    a = np.abs(h.astype(np.float64))
    Bout = Bu * (a + np.abs(c)) + np.abs(1 - u) * Bc + RTOL * np.abs(out)
    return Bout, Br, Bu, Bc, Bhc


def cell_inputs(D, V, nx, seed):
    """Inputs of the cell tests.  The RNN's W / b have one all-zero column with a zero bias (pre-activation exactly 0 in any
    summation order) and one column with bias -100 (negative for every row): the two edges of ReLU."""
    rng = np.random.default_rng(seed)
    K = (nx + 1) * D

    def u(*shape, s=1.0):
        return (rng.uniform(-1, 1, shape) * s).astype(np.float32)
    xs = [u(V, D) for _ in range(nx)]
    h = u(V, D)
    W = u(K, D, s=2.0 / math.sqrt(K))
    b = u(D, s=0.3)
    W[:, 5] = 0.0
    b[5] = 0.0
    b[D - 3] = -100.0
    cud = {"Wg": u(K, 2 * D, s=2.0 / math.sqrt(K)), "bg": u(2 * D, s=0.3), "Wcx": u(nx * D, D, s=2.0 / math.sqrt(nx * D)),
           "bcx": u(D, s=0.3), "Wch": u(D, D, s=2.0 / math.sqrt(D)), "bch": u(D, s=0.3)}
    return {"xs": xs, "h": h, "W": W, "b": b, "cudnn": cud}


def bwd_dx(dY, nseg_y, WT, xcols, split_inc, dx0, nin, use_avg, dh0, acc_dx, acc_dh, D, dt=np.float64):
    """ggnn_bwd_dx_f32 (csrc/ggnn_gemm.hip): Q = dY[:, :nseg_y D] WT.  Columns [0, xcols) are the x segments: with split_inc the
    last D of them go to dinc = (acc_dx ? dx0 + Q : Q) [/ (sum_t nin + 1e-7)], the others to dx (= or +=); columns [xcols, K)
    to dh (= or +=).  -> (dx or None, dinc or None, dh or None); dx keeps dx0 where the kernel writes nothing."""
    Q = dY[:, :nseg_y * D].astype(dt) @ WT.astype(dt)
    K = WT.shape[1]
    inc0 = xcols - D if (split_inc and xcols > 0) else xcols
    dx = None if dx0 is None else dx0.astype(dt).copy()
    dinc = dh = None
    if inc0 > 0:
        dx[:, :inc0] = (dx[:, :inc0] if acc_dx else 0) + Q[:, :inc0]
    if inc0 < xcols:
        dinc = Q[:, inc0:xcols] + (dx0.astype(dt)[:, inc0:xcols] if acc_dx else 0)
        if use_avg:
            dinc = dinc / (nin.astype(dt).sum(-1, keepdims=True, dtype=dt) + dt(SMALL))
    if K > xcols:
        dh = Q[:, xcols:] + (dh0.astype(dt) if acc_dh else 0)
    return dx, dinc, dh


def bwd_dx_bounds(dY, nseg_y, WT, xcols, split_inc, dx0, nin, use_avg, dh0, acc_dx, acc_dh, D):
    """Per element: the product's bound, + eps (|prefill| + |Q|) where the epilogue adds, times 1 / (deg + 1e-7) for dinc under
    mean aggregation, + RTOL of the result."""
    A = dY[:, :nseg_y * D]
    at = gemm_atol(A, WT)
    Qa = np.abs(A.astype(np.float64) @ WT.astype(np.float64))
    K = WT.shape[1]
    inc0 = xcols - D if (split_inc and xcols > 0) else xcols
    dx, dinc, dh = bwd_dx(dY, nseg_y, WT, xcols, split_inc, dx0, nin, use_avg, dh0, acc_dx, acc_dh, D)
    Bdx = Binc = Bdh = None
    if dx is not None:
        Bdx = np.zeros_like(dx)                            # (columns the kernel leaves alone must come back bit-identical)
        pre = np.abs(dx0.astype(np.float64)) if acc_dx else np.zeros_like(dx)
        Bdx[:, :inc0] = at[:, :inc0] + EPS * (pre[:, :inc0] + Qa[:, :inc0]) + RTOL * np.abs(dx[:, :inc0])
    if dinc is not None:
        pre = np.abs(dx0.astype(np.float64))[:, inc0:xcols] if acc_dx else 0.0
        Binc = at[:, inc0:xcols] + EPS * (pre + Qa[:, inc0:xcols])
        if use_avg:
            Binc = Binc / (nin.astype(np.float64).sum(-1, keepdims=True) + SMALL)
        Binc = Binc + RTOL * np.abs(dinc)
    if dh is not None:
        pre = np.abs(dh0.astype(np.float64)) if acc_dh else 0.0
        Bdh = at[:, xcols:] + EPS * (pre + Qa[:, xcols:]) + RTOL * np.abs(dh)
    return Bdx, Binc, Bdh


BWD_DX_SHAPES = ("rnn_avg", "rnn_sum", "cudnn_a", "cudnn_b", "cudnn_c")


def bwd_dx_inputs(shape, D, V, nx, seed):
    """The four call shapes of variants._hip_backward (the RNN one with and without mean aggregation).  dY has a row stride
    8 floats larger than its width; nin has an all-zero row (row 0), so the mean divides by 1e-7 there."""
    rng = np.random.default_rng(seed)
    T = 3
    nseg_y = 2 if shape == "cudnn_c" else 1
    xcols = 0 if shape == "cudnn_b" else nx * D
    K = xcols if shape == "cudnn_a" else xcols + D
    split_inc = shape in ("rnn_avg", "rnn_sum", "cudnn_c")
    use_avg = shape in ("rnn_avg", "cudnn_c")
    acc_dx = shape == "cudnn_c"
    acc_dh = shape in ("cudnn_b", "cudnn_c")
    width = nseg_y * D
    dYbuf = rng.normal(size=(V, width + 8)).astype(np.float32)
    WT = (rng.uniform(-1, 1, (width, K)) * 2.0 / math.sqrt(width)).astype(np.float32)
    nin = rng.integers(0, 4, (V, T)).astype(np.float32)
    nin[0] = 0.0
    dx0 = rng.normal(size=(V, max(xcols, 4))).astype(np.float32)
    dh0 = rng.normal(size=(V, D)).astype(np.float32)
    pass_dx = xcols > 0 and not (split_inc and nx == 1 and not acc_dx)     # nx = 1 with split_inc and no += : dx = None
    return {"dYbuf": dYbuf, "width": width, "nseg_y": nseg_y, "WT": WT, "xcols": xcols, "split_inc": split_inc,
            "dx0": dx0[:, :xcols] if pass_dx else None, "nin": nin if split_inc else None, "use_avg": use_avg,
            "dh0": dh0 if K > xcols else None, "acc_dx": acc_dx, "acc_dh": acc_dh, "D": D}


def bwd_dx_args(c):
    """Positional arguments of bwd_dx / bwd_dx_bounds from a bwd_dx_inputs dict."""
    return (c["dYbuf"][:, :c["width"]], c["nseg_y"], c["WT"], c["xcols"], c["split_inc"], c["dx0"], c["nin"], c["use_avg"], c["dh0"],
            c["acc_dx"], c["acc_dh"], c["D"])


# ---- element-wise stages (csrc/ggnn_bwd.hip) ----------------------------------------------------------------------------------
def _dact(activation, c, dt):
    return (1 - c * c) if activation == "tanh" else (c > 0).astype(dt)


def _dact_abs(activation, c):
    return (1 + c * c) if activation == "tanh" else (c > 0).astype(np.float64)


def act_bwd(g, out, activation, dt=np.float64):
    """dP = g act'(out): tanh' = 1 - out^2, relu' = [out > 0]."""
    return g.astype(dt) * _dact(activation, out.astype(dt), dt)


def act_bwd_bound(g, out, activation):
    """8 eps |g| (1 + out^2); ReLU selects and is exact (bound 0)."""
    g, o = np.abs(g.astype(np.float64)), out.astype(np.float64)
    return 8 * EPS * g * (1 + o * o) if activation == "tanh" else np.zeros_like(g)


def cudnn_bwd_stage(g, h, r, u, c, hc, dt=np.float64):
    """dpc = g (1-u) (1-c^2); dpu = g (h-c) u (1-u); dh = g u; dhc = dpc r; dpr = dpc hc r (1-r) -> (dpc, [dpr | dpu], dh, dhc)"""
    g, h, r, u, c, hc = (t.astype(dt) for t in (g, h, r, u, c, hc))
    dpc = g * (1 - u) * (1 - c * c)
    return dpc, np.concatenate([dpc * hc * r * (1 - r), g * (h - c) * u * (1 - u)], axis=1), g * u, dpc * r


def cudnn_bwd_stage_bounds(g, h, r, u, c, hc):
    """8 eps times the product of |factors|, differences replaced by sums (|h| + |c| for h - c, 1 + c^2 for 1 - c^2, ...)."""
    g, h, r, u, c, hc = (np.abs(t.astype(np.float64)) for t in (g, h, r, u, c, hc))
    dpc = g * (1 + u) * (1 + c * c)
    k = 8 * EPS
    return k * dpc, k * np.concatenate([dpc * hc * r * (1 + r), g * (h + c) * u * (1 + u)], axis=1), k * g * u, k * dpc * r


def gru_bwd_stage1(g, h, r, u, c, activation, dt=np.float64):
    """dpc = g (1-u) act'(c); dpu = g (h-c) u (1-u); dh = g u; rh = r h -> (dpc, dpu, dh, rh)"""
    g, h, r, u, c = (t.astype(dt) for t in (g, h, r, u, c))
    return g * (1 - u) * _dact(activation, c, dt), g * (h - c) * u * (1 - u), g * u, r * h


def gru_bwd_stage1_bounds(g, h, r, u, c, activation):
    g, h, r, u, c = (np.abs(t.astype(np.float64)) for t in (g, h, r, u, c))
    k = 8 * EPS
    return k * g * (1 + u) * _dact_abs(activation, c), k * g * (h + c) * u * (1 + u), k * g * u, k * r * h


def gru_bwd_stage2(drh, h, r, dh0, dt=np.float64):
    """dh = dh0 + drh r; dpr = drh h r (1-r) -> (dh, dpr)"""
    drh, h, r, dh0 = (t.astype(dt) for t in (drh, h, r, dh0))
    return dh0 + drh * r, drh * h * r * (1 - r)


def gru_bwd_stage2_bounds(drh, h, r, dh0):
    drh, h, r, dh0 = (np.abs(t.astype(np.float64)) for t in (drh, h, r, dh0))
    return 8 * EPS * (dh0 + drh * r), 8 * EPS * drh * h * r * (1 + r)


ELEMENTWISE_SHAPES = ((1, 4), (3, 100), (41, 100), (1025, 64))          # float4 counts 1, 75, 1025, 16400


def elementwise_inputs(V, D, seed):
    """Gates in (0, 1), candidates in (-1, 1); `c_relu` holds +0.0, -0.0 and negatives next to positive values."""
    rng = np.random.default_rng(seed)
    n = lambda: rng.normal(size=(V, D)).astype(np.float32)
    c_relu = n()
    flat = c_relu.reshape(-1)
    flat[0::7] = 0.0
    flat[3::7] = -0.0
    return {"g": n(), "h": n(), "r": rng.uniform(0.01, 0.99, (V, D)).astype(np.float32),
            "u": rng.uniform(0.01, 0.99, (V, D)).astype(np.float32), "c": rng.uniform(-0.99, 0.99, (V, D)).astype(np.float32),
            "hc": n(), "c_relu": c_relu, "drh": n(), "dh0": n()}


# ---- the cases: one list for the GPU test and for the host test's float32 evaluation ------------------------------------------
ATTN_D = (32, 64, 100, 128, 132, 256)        # sub-wave 16 (8 lanes used / all), 32 (25 / all), 64 (33 / all)
ATTN_V = (1, 17, 33)                         # dead sub-waves at 16, 8 and 4 nodes per workgroup
ATTN_T = (1, 3, 4)
ATTN_SWITCHES = ((False, True), (True, False), (True, True), (False, False))       # (bias, use_avg)
WSS_D = (32, 100, 256, 260, 512)             # 260 and 512: the strided column loop
WSS_NSEG = (1, 17)
CELL_D = (32, 64, 96, 100, 160, 200, 256)    # KC = 32, 64, 32, 100, 32, 100, 64; every NT choice
CELL_V = (1, 127, 128, 129, 1025)
CELL_NX = (1, 2, 3, 7)
BWD_DX_D = (32, 64, 100, 200)
BWD_DX_V = (1, 129)
BWD_DX_NX = (1, 3)


def seed_of(*key):
    """A small deterministic seed from the case's parameters."""
    s = 12345
    for k in key:
        s = (s * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return s


# ---- one RNN timestep on a graph without messages (the `not index.num_messages` branch of variants._hip_backward) --------------
def empty_graph_rnn_step(h, g, W, b, dt=np.float64):
    """No message: the aggregated input is 0 whatever the attention, bias-free; out = tanh([0 | h] W + b), and the gradient
    of h is the cell's alone: dP = g (1 - out^2), dh = (dP W^T)[:, h block].  -> (out, dh)"""
    D = h.shape[1]
    out = rnn([np.zeros_like(h)], h, W, b, "tanh", dt)
    dP = act_bwd(g, out, "tanh", dt)
    WT = np.ascontiguousarray(W.T)
    return out, bwd_dx(dP, 1, WT, D, True, None, np.zeros((h.shape[0], 1), np.float32), True, None, False, False, D, dt)[2]


def empty_graph_rnn_step_bounds(h, g, W, b):
    """out: rnn_bound.  dh: the error of out enters dP times 2 |g out|, dP's own rounding on top; all of that goes through
    |W^T| into the product, next to the product's own bound."""
    D = h.shape[1]
    out, _ = empty_graph_rnn_step(h, g, W, b)
    B_out = rnn_bound([np.zeros_like(h)], h, W, b, "tanh")
    dP = act_bwd(g, out, "tanh")
    E_dP = 2 * np.abs(g.astype(np.float64) * out) * B_out + act_bwd_bound(g, out, "tanh")
    WT = np.ascontiguousarray(W.astype(np.float64).T)
    B_dh = bwd_dx_bounds(dP, 1, WT, D, True, None, np.zeros((h.shape[0], 1), np.float32), True, None, False, False, D)[2]
    return B_out, B_dh + (E_dP @ np.abs(WT))[:, D:]
