"""Sparse GCN on the MI355X: the fused aggregate-transform kernel (csrc/ggnn_gcn.hip) and the composed path against the fp64
restatement, the dropout epilogue against ggnn_dropout_f32, determinism, the hand-written backward, the whole-stack call, and
the model's training loop and checkpoints."""
import os

import numpy as np
import pytest
import torch

import gcn_reference_math as ref

pytestmark = pytest.mark.gpu


def random_ahat(rng, V, nnz_per_row=3.1, symmetric=False):
    """Asymmetric (unless symmetric) sparse matrix, row-major sorted, with empty rows, duplicate (i, j) entries and negative
    weights.  -> (adj int64 [nnz, 2], w float32 [nnz])."""
    if V == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.float32)
    n = int(V * nnz_per_row)
    rows = rng.integers(0, V, n)
    rows = rows[rows % 7 != 3] if V > 7 else rows                  # rows 3, 10, 17, ... stay empty
    cols = (rows + rng.integers(-20, 21, len(rows))) % V
    adj = np.stack([rows, cols], 1)
    adj = np.concatenate([adj, adj[: len(adj) // 10]])             # duplicates
    w = rng.uniform(-0.3, 0.6, len(adj))
    if symmetric:
        adj = np.concatenate([adj, adj[:, ::-1]])
        w = np.concatenate([w, w])
    order = np.lexsort((adj[:, 1], adj[:, 0]))
    return adj[order], w[order].astype(np.float32)


def _graph(pkg, adj, w, V, cuda):
    return pkg.ops.gcn_graph(adj, w, V, cuda)


def _bound(adj, w, x, W):
    """4e-7 * sum_k |S_k| |W_kn| with |S| = |A_hat| |x|: the bound the exact compacted transform is held to (per K-term product)."""
    return 4e-7 * (ref.spmm_abs(adj, w, x) @ np.abs(W.astype(np.float64))) + 1e-30


@pytest.mark.parametrize("D", [32, 64, 100])
@pytest.mark.parametrize("V", [0, 1, 17, 5000, 100003])
def test_fused_layer_against_fp64(pkg, cuda, D, V):
    rng = np.random.default_rng(D * 7 + V)
    adj, w = random_ahat(rng, V)
    x = rng.standard_normal((V, D)).astype(np.float32)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    g = _graph(pkg, adj, w, V, cuda)
    xt, Wt, bt = (torch.from_numpy(a).to(cuda) for a in (x, W, b))
    S64 = ref.spmm(adj, w, x)
    for bias, relu, save in ((None, False, False), (bt, True, True), (bt, False, True), (None, True, False)):
        out, S = pkg.ops.gcn_layer(xt, g, Wt, bias, relu=relu, save_s=save)
        want = S64 @ W.astype(np.float64) + (b.astype(np.float64) if bias is not None else 0.0)
        if relu:
            want = np.maximum(want, 0.0)
        err = np.abs(out.cpu().numpy().astype(np.float64) - want)
        assert (err <= _bound(adj, w, x, W) + 4e-7 * np.abs(b if bias is not None else 0)).all(), (bias is None, relu, err.max())
        if save:
            np.testing.assert_allclose(S.cpu().numpy(), S64, rtol=0, atol=float((4e-7 * ref.spmm_abs(adj, w, x)).max(initial=0.0)) + 1e-30)
        else:
            assert S is None


@pytest.mark.parametrize("D", [48, 128])
def test_composed_fallback_against_fp64(pkg, cuda, D):
    assert not pkg.ops.gcn_fused_supported(D)
    rng = np.random.default_rng(D)
    V = 3000
    adj, w = random_ahat(rng, V)
    x = rng.standard_normal((V, D)).astype(np.float32)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    out, S = pkg.ops.gcn_layer(torch.from_numpy(x).to(cuda), _graph(pkg, adj, w, V, cuda), torch.from_numpy(W).to(cuda),
                               relu=True, save_s=True)
    want = np.maximum(ref.spmm(adj, w, x) @ W.astype(np.float64), 0)
    assert (np.abs(out.cpu().numpy() - want) <= _bound(adj, w, x, W)).all()


@pytest.mark.parametrize("D", [32, 64, 100])
def test_fused_against_composed(pkg, cuda, D):
    rng = np.random.default_rng(D + 1)
    V = 20000
    adj, w = random_ahat(rng, V)
    x = rng.standard_normal((V, D)).astype(np.float32)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    b = torch.from_numpy(rng.standard_normal(D).astype(np.float32)).to(cuda)
    g = _graph(pkg, adj, w, V, cuda)
    xt, Wt = torch.from_numpy(x).to(cuda), torch.from_numpy(W).to(cuda)
    for transpose in (False, True):
        f, _ = pkg.ops.gcn_layer(xt, g, Wt, b, relu=True, transpose=transpose, fused=True)
        c, _ = pkg.ops.gcn_layer(xt, g, Wt, b, relu=True, transpose=transpose, fused=False)
        bound = 2 * _bound(adj[:, ::-1] if transpose else adj, w, x, W.T if transpose else W)
        assert (np.abs(f.cpu().numpy() - c.cpu().numpy()) <= bound + 8e-7 * abs(b.cpu().numpy())).all(), transpose


@pytest.mark.parametrize("D", [32, 100, 48])
def test_dropout_epilogue_matches_ggnn_dropout(pkg, cuda, D):
    rng = np.random.default_rng(3)
    V = 4099
    adj, w = random_ahat(rng, V)
    g = _graph(pkg, adj, w, V, cuda)
    x = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).to(cuda)
    W = torch.from_numpy((rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)).to(cuda)
    keys = torch.from_numpy(rng.integers(0, 2 ** 40, V)).to(cuda)
    seed = 0x1234_5678_9ABC_DEF0
    plain, _ = pkg.ops.gcn_layer(x, g, W, relu=True)
    for row_key in (keys, None):
        dropped, _ = pkg.ops.gcn_layer(x, g, W, relu=True, keep_prob=0.7, seed=seed, row_key=row_key)
        want = pkg.ops.dropout(plain, 0.7, seed, row_key)
        assert torch.equal(dropped, want)
        assert 0.2 < float((dropped == 0).float().mean()) < 0.8


def test_determinism(pkg, cuda):
    rng = np.random.default_rng(4)
    V, D = 50000, 100
    adj, w = random_ahat(rng, V)
    g = _graph(pkg, adj, w, V, cuda)
    x = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).to(cuda)
    W = torch.from_numpy(rng.standard_normal((D, D)).astype(np.float32)).to(cuda)
    a = pkg.ops.gcn_layer(x, g, W, relu=True, save_s=True)
    b = pkg.ops.gcn_layer(x, g, W, relu=True, save_s=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("D,symmetric,keep", [(64, False, 1.0), (100, True, 1.0), (32, False, 0.75), (48, False, 0.75)])
def test_backward_against_fp64(pkg, cuda, D, symmetric, keep):
    gm = pkg.gcn_model
    rng = np.random.default_rng(D)
    V, L = 2000, 3
    adj, w = random_ahat(rng, V, symmetric=symmetric)
    g = _graph(pkg, adj, w, V, cuda)
    h0 = rng.standard_normal((V, D)).astype(np.float32)
    Ws = [(rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32) for _ in range(L)]
    bs = [(rng.standard_normal(D) * 0.1).astype(np.float32) for _ in range(L)]
    tW = [torch.from_numpy(a).to(cuda).requires_grad_(True) for a in Ws]
    tb = [torch.from_numpy(a).to(cuda).requires_grad_(True) for a in bs]
    keys = torch.arange(V, dtype=torch.int64, device=cuda) * 3 + 11
    seeds = [101, 202]
    masks = [pkg.ops.dropout(torch.ones((V, D), device=cuda), keep, s, keys).cpu().numpy().astype(np.float64) if keep < 1 else None
             for s in seeds] + [None]
    h = torch.from_numpy(h0).to(cuda)
    for l in range(L):
        last = l == L - 1
        h = gm.GCNLayerFn.apply(h, tW[l], tb[l], g, not last, 1.0 if last else keep, 0 if last else seeds[l], keys)
    d_final = rng.standard_normal((V, D)).astype(np.float32)
    (h * torch.from_numpy(d_final).to(cuda)).sum().backward()
    final, saved = ref.forward(h0, adj, w, Ws, bs, masks)
    dWs, dbs = ref.backward(adj, w, Ws, saved, d_final, masks)
    np.testing.assert_allclose(h.detach().cpu().numpy(), final, rtol=1e-4, atol=1e-4)
    for l in range(L):
        scale = float(np.abs(dWs[l]).max()) + 1e-30
        assert np.abs(tW[l].grad.cpu().numpy() - dWs[l]).max() <= 1e-4 * scale, l
        scale = float(np.abs(dbs[l]).max()) + 1e-30
        assert np.abs(tb[l].grad.cpu().numpy() - dbs[l]).max() <= 1e-4 * scale, l


@pytest.mark.parametrize("D", [32, 64, 100])
def test_propagate_equals_layer_path(pkg, cuda, D):
    rng = np.random.default_rng(9)
    V, L = 30011, 4
    adj, w = random_ahat(rng, V)
    g = _graph(pkg, adj, w, V, cuda)
    h0 = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).to(cuda)
    Ws = [torch.from_numpy((rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)).to(cuda) for _ in range(L)]
    bs = [torch.from_numpy(rng.standard_normal(D).astype(np.float32)).to(cuda) for _ in range(L)]
    for biases in (None, bs):
        h = h0
        for l in range(L):
            h = pkg.ops.gcn_layer(h, g, Ws[l], None if biases is None else biases[l], relu=l < L - 1)[0]
        assert torch.equal(pkg.ops.gcn_propagate(h0, g, Ws, biases), h)
    empty = _graph(pkg, *random_ahat(rng, 0), 0, cuda)
    assert pkg.ops.gcn_propagate(h0[:0], empty, Ws).shape == (0, D)


def _args(ms, config, **kw):
    a = {"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms, "--config": config}
    a.update(kw)
    return a


@pytest.mark.parametrize("config", [{"hidden_size": 100}, {"hidden_size": 64, "num_timesteps": 2, "gcn_use_bias": True},
                                    {"hidden_size": 48, "task_ids": [0, 1], "task_sample_ratios": {"1": 0.5}},
                                    {"hidden_size": 32, "graph_state_dropout_keep_prob": 0.8}])
def test_model_forward_and_train(pkg, cuda, config, tmp_path):
    import ggnn_amd
    ms = pkg.synthetic_qm9(300, seed=2, num_tasks=2)
    config = dict(config, num_epochs=3, batch_size=2000, random_seed=3)
    model = ggnn_amd.SparseGCNChemModel(_args(ms, config))
    assert not pkg.train_native.eligible(model, {})
    feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
    with torch.no_grad():
        model.feed(feed)
        got = model.compute_final_node_representations().cpu().numpy()
    Ws = [t.cpu().numpy() for t in model.weights['edge_weights']]
    bs = [t.cpu().numpy() for t in model.weights['edge_biases']] or None
    want, _ = ref.forward(feed['initial_node_representation'].cpu().numpy(), feed['adjacency_list'], feed['adjacency_weights'], Ws, bs)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5)
    log = model.train()
    assert len(log) == 3 and all(np.isfinite(e['train_results'][0]) and np.isfinite(e['valid_results'][0]) for e in log)
    # checkpoint round trip (the base class's pickle schema)
    path = str(tmp_path / "gcn.pickle")
    model.save_progress(path, model.train_step_id, model.valid_step_id)
    restored = ggnn_amd.SparseGCNChemModel(_args(ms, config, **{"--restore": path}))
    for name, t in model.named_variables().items():
        assert torch.equal(t, restored.named_variables()[name]), name
    with torch.no_grad():
        restored.feed(next(iter(restored.make_minibatch_iterator(restored.valid_data, is_training=False))))
        again = restored.compute_final_node_representations().cpu().numpy()
    with torch.no_grad():
        model.feed(feed)
        np.testing.assert_array_equal(again, model.compute_final_node_representations().cpu().numpy())
