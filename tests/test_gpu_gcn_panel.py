"""The column-panel GCN layer (csrc/ggnn_gcn_panel.hip, hidden sizes 128 / 192 / 256) on the MI355X: the layer, its transposed
form and its dropout epilogue against the fp64 restatement and the composed route, determinism, the whole-stack call, the
hand-written backward on the panel route, and the model behind params['gcn_panel_layers']."""
import numpy as np
import pytest
import torch

import gcn_reference_math as ref

pytestmark = pytest.mark.gpu

SIZES = [128, 192, 256]


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


def ahat_with_long_rows(rng, V):
    """random_ahat plus one row of degree 41 and one of degree 2 (rows 3 and 10, which random_ahat leaves empty; at V <= 10 row 0
    alone, with 41 entries): the tails of the gather loop's groups of 4 / 3 / 2 rows in flight."""
    adj, w = random_ahat(rng, V)
    if V == 0:
        return adj, w
    if V > 10:
        extra = np.concatenate([np.stack([np.full(41, 3), rng.integers(0, V, 41)], 1), np.stack([np.full(2, 10), rng.integers(0, V, 2)], 1)])
    else:
        adj, w = adj[:0], w[:0]
        extra = np.stack([np.zeros(41, np.int64), rng.integers(0, V, 41)], 1)
    adj = np.concatenate([adj, extra])
    w = np.concatenate([w, rng.uniform(-0.3, 0.6, len(extra)).astype(np.float32)])
    order = np.lexsort((adj[:, 1], adj[:, 0]))
    adj, w = adj[order], w[order]
    deg = np.bincount(adj[:, 0], minlength=V)
    assert 41 in deg and (V <= 10 or deg[10] == 2)
    return adj, w


def _bound(adj, w, x, W):
    """4e-7 * sum_k |S_k| |W_kn| with |S| = |A_hat| |x|: the project's bound for the exact three-piece product."""
    return 4e-7 * (ref.spmm_abs(adj, w, x) @ np.abs(W.astype(np.float64))) + 1e-30


def _inputs(rng, V, D):
    x = rng.standard_normal((V, D)).astype(np.float32)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    return x, W, b


def _wrap_rows(pkg):
    """One row block past what a launch covers without its grid-stride loop wrapping, from the launcher's own two factors."""
    rows, cap = pkg.ops.gcn_panel_launch_geometry()
    return rows * cap + 17


@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("V", [0, 1, 17, 129, 2049, "wrap"])
def test_layer_against_fp64(pkg, cuda, D, V):
    if V == "wrap":
        V = _wrap_rows(pkg)
    rng = np.random.default_rng(D * 7 + V)
    adj, w = ahat_with_long_rows(rng, V)
    x, W, b = _inputs(rng, V, D)
    g = pkg.ops.gcn_graph(adj, w, V, cuda)
    xt, Wt, bt = (torch.from_numpy(a).to(cuda) for a in (x, W, b))
    S64 = ref.spmm(adj, w, x)
    S_abs = ref.spmm_abs(adj, w, x)
    bound = 4e-7 * (S_abs @ np.abs(W.astype(np.float64))) + 1e-30
    for bias, relu, save in ((None, False, False), (bt, True, True), (bt, False, True), (None, True, False)):
        out, S = pkg.ops.gcn_layer(xt, g, Wt, bias, relu=relu, save_s=save, panel=True)
        assert out.shape == (V, D)
        want = S64 @ W.astype(np.float64) + (b.astype(np.float64) if bias is not None else 0.0)
        if relu:
            want = np.maximum(want, 0.0)
        err = np.abs(out.cpu().numpy().astype(np.float64) - want)
        ok = err <= bound + 4e-7 * np.abs(b if bias is not None else 0)
        print("D=%d V=%d bias=%s relu=%s: max err %.3e, max err / bound %.3f" % (
            D, V, bias is not None, relu, err.max(initial=0.0), (err / (bound + 4e-7 * np.abs(b if bias is not None else 0))).max(initial=0.0)))
        assert ok.all(), (bias is None, relu, err.max(), np.argwhere(~ok)[:4])
        if save:
            # (test_fused_layer_against_fp64's bound on S, in its form: the largest 4e-7 |A_hat| |x| of the matrix)
            np.testing.assert_allclose(S.cpu().numpy(), S64, rtol=0, atol=float((4e-7 * S_abs).max(initial=0.0)) + 1e-30)
        else:
            assert S is None


@pytest.mark.parametrize("D", SIZES)
def test_transposed_layer_against_fp64(pkg, cuda, D):
    """dx = A_hat^T (dP W^T) on an asymmetric W and A_hat: a swapped panel or operand layout shows here."""
    rng = np.random.default_rng(D + 5)
    V = 2049
    adj, w = ahat_with_long_rows(rng, V)
    x, W, _ = _inputs(rng, V, D)
    W = W * np.linspace(0.5, 2.0, D, dtype=np.float32)[None, :] + np.tri(D, dtype=np.float32) * 0.01     # far from symmetric
    g = pkg.ops.gcn_graph(adj, w, V, cuda)
    out, S = pkg.ops.gcn_layer(torch.from_numpy(x).to(cuda), g, torch.from_numpy(W).to(cuda), transpose=True, save_s=True, panel=True)
    adj_t = adj[:, ::-1]
    want = ref.spmm(adj_t, w, x) @ W.T.astype(np.float64)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)
    bound = _bound(adj_t, w, x, W.T)
    print("D=%d transposed: max err %.3e, max err / bound %.3f" % (D, err.max(), (err / bound).max()))
    assert (err <= bound).all()
    np.testing.assert_allclose(S.cpu().numpy(), ref.spmm(adj_t, w, x), rtol=0, atol=float((4e-7 * ref.spmm_abs(adj_t, w, x)).max()) + 1e-30)


@pytest.mark.parametrize("D", SIZES)
def test_panel_against_composed(pkg, cuda, D):
    rng = np.random.default_rng(D + 1)
    V = 5003
    adj, w = random_ahat(rng, V)
    x, W, b = _inputs(rng, V, D)
    bt = torch.from_numpy(b).to(cuda)
    g = pkg.ops.gcn_graph(adj, w, V, cuda)
    xt, Wt = torch.from_numpy(x).to(cuda), torch.from_numpy(W).to(cuda)
    for transpose in (False, True):
        p, _ = pkg.ops.gcn_layer(xt, g, Wt, bt, relu=True, transpose=transpose, panel=True)
        c, _ = pkg.ops.gcn_layer(xt, g, Wt, bt, relu=True, transpose=transpose, panel=False)
        bound = 2 * _bound(adj[:, ::-1] if transpose else adj, w, x, W.T if transpose else W)
        assert (np.abs(p.cpu().numpy() - c.cpu().numpy()) <= bound + 8e-7 * abs(b)).all(), transpose


@pytest.mark.parametrize("D", SIZES)
def test_dropout_epilogue_matches_ggnn_dropout(pkg, cuda, D):
    rng = np.random.default_rng(3)
    V = 4099
    adj, w = random_ahat(rng, V)
    g = pkg.ops.gcn_graph(adj, w, V, cuda)
    x = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).to(cuda)
    W = torch.from_numpy((rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)).to(cuda)
    keys = torch.from_numpy(rng.integers(0, 2 ** 40, V)).to(cuda)
    seed = 0x1234_5678_9ABC_DEF0
    plain, _ = pkg.ops.gcn_layer(x, g, W, relu=True, panel=True)
    for row_key in (keys, None):
        dropped, _ = pkg.ops.gcn_layer(x, g, W, relu=True, keep_prob=0.7, seed=seed, row_key=row_key, panel=True)
        want = pkg.ops.dropout(plain, 0.7, seed, row_key)
        assert torch.equal(dropped, want)
        assert 0.2 < float((dropped == 0).float().mean()) < 0.8


@pytest.mark.parametrize("D", SIZES)
def test_determinism(pkg, cuda, D):
    rng = np.random.default_rng(4)
    V = 20000
    adj, w = random_ahat(rng, V)
    g = pkg.ops.gcn_graph(adj, w, V, cuda)
    x = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).to(cuda)
    W = torch.from_numpy(rng.standard_normal((D, D)).astype(np.float32)).to(cuda)
    a = pkg.ops.gcn_layer(x, g, W, relu=True, save_s=True, panel=True)
    b = pkg.ops.gcn_layer(x, g, W, relu=True, save_s=True, panel=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("D", SIZES)
def test_propagate_equals_layer_path(pkg, cuda, D):
    rng = np.random.default_rng(9)
    V, L = 5003, 4
    adj, w = random_ahat(rng, V)
    g = pkg.ops.gcn_graph(adj, w, V, cuda)
    h0 = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32)).to(cuda)
    Ws = [torch.from_numpy((rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)).to(cuda) for _ in range(L)]
    bs = [torch.from_numpy(rng.standard_normal(D).astype(np.float32)).to(cuda) for _ in range(L)]
    for biases in (None, bs):
        h = h0
        for l in range(L):
            h = pkg.ops.gcn_layer(h, g, Ws[l], None if biases is None else biases[l], relu=l < L - 1, panel=True)[0]
        assert torch.equal(pkg.ops.gcn_panel_propagate(h0, g, Ws, biases), h)
    empty = pkg.ops.gcn_graph(*random_ahat(rng, 0), 0, cuda)
    assert pkg.ops.gcn_panel_propagate(h0[:0], empty, Ws).shape == (0, D)


@pytest.mark.parametrize("D,symmetric,keep", [(128, False, 1.0), (192, True, 0.75), (256, False, 0.75), (256, True, 1.0)])
def test_backward_against_fp64(pkg, cuda, launches, D, symmetric, keep):
    gm = pkg.gcn_model
    rng = np.random.default_rng(D)
    V, L = 2000, 3
    adj, w = random_ahat(rng, V, symmetric=symmetric)
    g = pkg.ops.gcn_graph(adj, w, V, cuda)
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
    del launches[:]
    for l in range(L):
        last = l == L - 1
        h = gm.GCNLayerFn.apply(h, tW[l], tb[l], g, not last, 1.0 if last else keep, 0 if last else seeds[l], keys, True)
    d_final = rng.standard_normal((V, D)).astype(np.float32)
    (h * torch.from_numpy(d_final).to(cuda)).sum().backward()
    names = list(launches)
    # forward: L panel launches; backward: dx of layers L-1 .. 1 (layer 0's input needs no gradient); nothing on the composed route
    assert sum(n.startswith("gcn_panel_layer") for n in names) == 2 * L - 1, names
    assert not any(n in ("gcn_epilogue", "gcn_pack") or n.startswith("gcn_layer[") for n in names), names
    final, saved = ref.forward(h0, adj, w, Ws, bs, masks)
    dWs, dbs = ref.backward(adj, w, Ws, saved, d_final, masks)
    np.testing.assert_allclose(h.detach().cpu().numpy(), final, rtol=1e-4, atol=1e-4)
    for l in range(L):
        scale = float(np.abs(dWs[l]).max()) + 1e-30
        assert np.abs(tW[l].grad.cpu().numpy() - dWs[l]).max() <= 1e-4 * scale, l
        scale = float(np.abs(dbs[l]).max()) + 1e-30
        assert np.abs(tb[l].grad.cpu().numpy() - dbs[l]).max() <= 1e-4 * scale, l


@pytest.fixture
def launches(pkg, monkeypatch):
    """Names of the launches the host layer makes, in order."""
    names = []
    launch = pkg.ops._launch

    def recording_launch(name, fn):
        names.append(name)
        return launch(name, fn)

    monkeypatch.setattr(pkg.ops, "_launch", recording_launch)
    return names


def _args(ms, config, **kw):
    a = {"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms, "--config": config}
    a.update(kw)
    return a


@pytest.mark.parametrize("config", [{"hidden_size": 128, "num_timesteps": 2, "gcn_use_bias": True},
                                    {"hidden_size": 256, "task_ids": [0, 1]}])
def test_model_with_the_key(pkg, cuda, launches, config, tmp_path):
    import ggnn_amd
    ms = pkg.synthetic_qm9(300, seed=2, num_tasks=2)
    config = dict(config, num_epochs=3, batch_size=2000, random_seed=3, gcn_panel_layers=True)
    model = ggnn_amd.SparseGCNChemModel(_args(ms, config))
    assert model.gcn_panel_route()
    feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
    del launches[:]
    with torch.no_grad():
        model.feed(feed)
        got = model.compute_final_node_representations().cpu().numpy()
    assert [n for n in launches if n.startswith("gcn_")] == ["gcn_panel_propagate[D=%d,L=%d]" % (config["hidden_size"], model.params["num_timesteps"])]
    Ws = [t.cpu().numpy() for t in model.weights['edge_weights']]
    bs = [t.cpu().numpy() for t in model.weights['edge_biases']] or None
    want, _ = ref.forward(feed['initial_node_representation'].cpu().numpy(), feed['adjacency_list'], feed['adjacency_weights'], Ws, bs)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5)
    del launches[:]
    log = model.train()
    # training runs GCNLayerFn on the panel route: no composed-route epilogue, no D <= 100 launch
    assert any(n.startswith("gcn_panel_layer[") for n in launches)
    assert not any(n in ("gcn_epilogue", "gcn_pack") or n.startswith("gcn_layer[") for n in launches)
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


@pytest.mark.parametrize("hidden", [100, 48])
def test_model_with_the_key_at_an_unsupported_size(pkg, cuda, hidden):
    """The key at a hidden size without the panel kernel: the forward output and one training step's weights are the key-off
    model's from the same seed, bit for bit."""
    import ggnn_amd
    ms = pkg.synthetic_qm9(200, seed=4)
    results = []
    for key in (False, True):
        config = {"hidden_size": hidden, "num_timesteps": 2, "num_epochs": 1, "batch_size": 100000, "random_seed": 5,
                  "graph_state_dropout_keep_prob": 0.9}
        if key:
            config["gcn_panel_layers"] = True
        model = ggnn_amd.SparseGCNChemModel(_args(ms, config))
        assert not model.gcn_panel_route()
        feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
        with torch.no_grad():
            model.feed(feed)
            out = model.compute_final_node_representations().clone()
        model.train()                                     # one epoch of one batch: one optimisation step
        assert model.train_step_id == 1
        results.append((out, {n: t.clone() for n, t in model.named_variables().items()}))
    assert torch.equal(results[0][0], results[1][0])
    for name, t in results[0][1].items():
        assert torch.equal(t, results[1][1][name]), name
