"""fp64 NumPy restatement of the sparse GCN layer stack (chem_tensorflow_gcn.py:62-82) and of its backward pass: the checker the GCN
tests hold the HIP kernels against.  Written from the reference's equations, not from the package."""
import numpy as np


def spmm(adj, w, x):
    """A x for the sparse A with entries (adj[k], w[k]) (duplicates add), fp64."""
    out = np.zeros((x.shape[0], x.shape[1]), np.float64)
    np.add.at(out, adj[:, 0], w[:, None].astype(np.float64) * x[adj[:, 1]].astype(np.float64))
    return out


def spmm_abs(adj, w, x):
    return spmm(adj, np.abs(w), np.abs(x))


def forward(h0, adj, w, Ws, bs=None, masks=None):
    """-> (final states, per layer (S, P, out))."""
    h = h0.astype(np.float64)
    saved = []
    L = len(Ws)
    for l in range(L):
        S = spmm(adj, w, h)
        P = S @ Ws[l].astype(np.float64)
        if bs is not None:
            P = P + bs[l].astype(np.float64)
        out = P
        if l < L - 1:
            out = np.maximum(P, 0.0)
            if masks is not None and masks[l] is not None:
                out = out * masks[l]
        saved.append((S, P, out))
        h = out
    return h, saved


def backward(adj, w, Ws, saved, d_final, masks=None):
    """Gradients of sum(final * d_final) -> (dWs, dbs).  dh_0 is not formed (h0 is a placeholder)."""
    L = len(Ws)
    g = d_final.astype(np.float64)
    dWs, dbs = [None] * L, [None] * L
    adj_t = adj[:, ::-1]
    for l in reversed(range(L)):
        S, P, _ = saved[l]
        dP = g
        if l < L - 1:
            if masks is not None and masks[l] is not None:
                dP = dP * masks[l]
            dP = dP * (P > 0)
        dWs[l] = S.T @ dP
        dbs[l] = dP.sum(axis=0)
        if l > 0:
            g = spmm(adj_t, w, dP @ Ws[l].astype(np.float64).T)
    return dWs, dbs
