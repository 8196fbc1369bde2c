"""GPU tests of the sparse GCN's native training step at hidden sizes 128 / 192 / 256 (params['native_training'] together with
params['gcn_panel_layers']): the panel layer backward with the lower layer's gate in its epilogue (ggnn_gcn_panel_layer_bwd_f32)
against the three launches it replaces and against float64, the one-launch panel pack, and the step on
ggnn_gcn_panel_train_forward_f32 / ggnn_gcn_panel_train_backward_f32 -- gradients against float64, against the autograd panel route,
determinism, the fallbacks and train() (chem_tensorflow_gcn.py:62-93, chem_tensorflow.py:183-191)."""
import json
import pickle

import numpy as np
import pytest
import torch

import gcn_golden as GG
import gcn_reference_math as ref
import gcn_train_reference as GR
import train_reference as TR

pytestmark = pytest.mark.gpu
NATIVE, PANEL = "native_training", "gcn_panel_layers"
SIZES = [128, 192, 256]


def random_ahat(rng, V, nnz_per_row=3.1):
    """test_gpu_gcn_panel.random_ahat restated: asymmetric sparse matrix, row-major sorted, with empty rows, duplicate (i, j) entries
    and negative weights.  -> (adj int64 [nnz, 2], w float32 [nnz])."""
    n = int(V * nnz_per_row)
    rows = rng.integers(0, V, n)
    rows = rows[rows % 7 != 3] if V > 7 else rows                  # rows 3, 10, 17, ... stay empty
    cols = (rows + rng.integers(-20, 21, len(rows))) % V
    adj = np.stack([rows, cols], 1)
    adj = np.concatenate([adj, adj[: len(adj) // 10]])             # duplicates
    w = rng.uniform(-0.3, 0.6, len(adj))
    order = np.lexsort((adj[:, 1], adj[:, 0]))
    return adj[order], w[order].astype(np.float32)


def ahat_with_long_rows(rng, V):
    """test_gpu_gcn_panel.ahat_with_long_rows restated: random_ahat plus one row of degree 41 and one of degree 2 (at V <= 10 row 0
    alone, with 41 entries): the tails of the gather loop's groups of 4 / 3 / 2 rows in flight.  The layer backward walks the
    TRANSPOSED matrix, so the long rows are given as columns too: column 3 and column 10 of A_hat are rows 3 and 10 of A_hat^T."""
    adj, w = random_ahat(rng, V)
    if V > 10:
        extra = np.concatenate([np.stack([np.full(41, 3), rng.integers(0, V, 41)], 1), np.stack([np.full(2, 10), rng.integers(0, V, 2)], 1)])
        keep = (adj[:, 1] != 3) & (adj[:, 1] != 10)
        adj, w = adj[keep], w[keep]
        extra = np.concatenate([extra, extra[:, ::-1]])
    else:
        adj, w = adj[:0], w[:0]
        extra = np.stack([np.zeros(41, np.int64), rng.integers(0, V, 41)], 1)
    adj = np.concatenate([adj, extra])
    w = np.concatenate([w, rng.uniform(-0.3, 0.6, len(extra)).astype(np.float32)])
    order = np.lexsort((adj[:, 1], adj[:, 0]))
    adj, w = adj[order], w[order]
    if V > 10:
        deg_t = np.bincount(adj[:, 1], minlength=V)
        assert deg_t[3] >= 41 and deg_t[10] >= 2 and np.bincount(adj[:, 0], minlength=V)[3] >= 41
    return adj, w


def _bound(adj, w, x, W):
    """test_gpu_gcn_panel._bound: 4e-7 * sum_k |S_k| |W_kn| with |S| = |A| |x|."""
    return 4e-7 * (ref.spmm_abs(adj, w, x) @ np.abs(W.astype(np.float64))) + 1e-30


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def _wrap_rows(pkg):
    """One row block past what a launch covers without its pass loop wrapping, from the launcher's own two factors."""
    rows, cap = pkg.ops.gcn_panel_launch_geometry()
    return rows * cap + 17


def _bwd_inputs(V, D):
    rng = np.random.default_rng(100 * D + V)
    adj, w = ahat_with_long_rows(rng, V)
    dP = rng.standard_normal((V, D)).astype(np.float32)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    W = W * np.linspace(0.5, 2.0, D, dtype=np.float32)[None, :] + np.tri(D, dtype=np.float32) * 0.01     # far from symmetric
    # the lower layer's forward output dropout(relu(P)): positives, exact zeros and negative zeros
    out = np.maximum(rng.standard_normal((V, D)), 0).astype(np.float32)
    out[rng.random((V, D)) < 0.1] = -0.0
    out[0, :3] = (0.0, -0.0, 1.5)
    keys = rng.integers(0, 2 ** 40, V)
    return adj, w, dP, W, out, keys


@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("V,keep", [(1, 1.0), (1, 0.75), (17, 1.0), (17, 0.75), (129, 1.0), (129, 0.75), (2049, 1.0), (2049, 0.75),
                                    ("wrap", 0.75)])
def test_panel_layer_bwd_equals_its_composition(pkg, cuda, V, D, keep):
    """One ggnn_gcn_panel_layer_bwd_f32 launch against the panel layer launch on the transposed CSR -> ggnn_dropout_f32 ->
    ggnn_act_bwd_f32, bit for bit; V = 1 is a single row, V = 17 a partial second tile, V = 129 a second workgroup, V = 2049 has
    rows of degree 41 and 2 in A_hat^T (the gather tails), "wrap" a second pass per workgroup (the ring re-armed with the gate loads
    of the first pass behind it).  At V = 2049 also against float64 A_hat^T (dP W^T) * mask * [out > 0], W asymmetric, under the
    project bound 4e-7 |A_hat^T| |dP| |W^T|."""
    ops = pkg.ops
    if V == "wrap":
        V = _wrap_rows(pkg)
    adj, w, dP, W, out, keys = _bwd_inputs(V, D)
    g = ops.gcn_graph(adj, w, V, cuda)
    t = lambda a: torch.from_numpy(a).to(cuda)
    dPt, Wt, outt = t(dP), t(W), t(out)
    assert bool((outt == 0).any()) and bool(torch.signbit(outt).any()) and bool((outt > 0).any())
    assert bool(((outt == 0) & ~torch.signbit(outt)).any())           # +0.0 as well as -0.0
    seed = 0x0FED_CBA9_8765_4321
    img = ops.gcn_panel_pack(Wt, True)
    for row_key in (t(keys), None):
        got = ops.gcn_panel_layer_bwd(dPt, g, Wt, outt, keep, seed, row_key)
        dx = ops.gcn_layer(dPt, g, Wt, transpose=True, panel=True)[0]
        if keep < 1.0:
            dx = ops.dropout(dx, keep, seed, row_key)
        want = ops.act_bwd(dx, outt, "relu")
        assert torch.equal(got, want), (V, D, keep, row_key is None)
        assert torch.equal(_bits(got), _bits(want)), (V, D, keep, row_key is None)
        assert bool((got != 0).any())
        assert torch.equal(_bits(ops.gcn_panel_layer_bwd(dPt, g, Wt, outt, keep, seed, row_key, img=img)), _bits(got))
        if V == 2049:
            mask = ops.dropout(torch.ones((V, D), device=cuda), keep, seed, row_key).cpu().numpy().astype(np.float64) if keep < 1.0 else 1.0
            want64 = ref.spmm(adj[:, ::-1], w, dP.astype(np.float64) @ W.astype(np.float64).T) * mask * (out > 0)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want64)
            bound = _bound(adj[:, ::-1], w, dP, W.T)
            print("V=%d D=%d keep=%g: max err / bound = %.3f" % (V, D, keep, float((err / bound).max())))
            assert (err <= bound).all(), float((err / bound).max())
            if keep < 1.0:
                assert 0.1 < float((np.asarray(mask) == 0).mean()) < 0.4


@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("L", [1, 3])
def test_panel_train_pack_equals_single_packs(pkg, cuda, L, D):
    rng = np.random.default_rng(L * 1000 + D)
    Ws = [torch.from_numpy(rng.standard_normal((D, D)).astype(np.float32)).to(cuda) for _ in range(L)]
    images = pkg.ops.gcn_panel_train_pack(Ws)
    n = pkg._lib.load().ggnn_gcn_panel_image_bytes(D) // 4
    assert images.shape[0] == 2 * L - 1 and images.shape[1] >= n
    for l in range(L):
        assert torch.equal(_bits(images[l, :n]), _bits(pkg.ops.gcn_panel_pack(Ws[l]))), l
        if l >= 1:
            assert torch.equal(_bits(images[L + l - 1, :n]), _bits(pkg.ops.gcn_panel_pack(Ws[l], True))), l
            assert not torch.equal(_bits(images[L + l - 1, :n]), _bits(images[l, :n]))


# ---- the step ------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Names of the launches ops._launch issues and the autograd backward passes entered (the pattern of test_gpu_gcn_native.py)."""

    def __init__(self, pkg, monkeypatch):
        self.names, self.backwards = [], 0
        original, tb, ab = pkg.ops._launch, torch.Tensor.backward, torch.autograd.backward

        def launch(name, fn):
            self.names.append(name)
            return original(name, fn)

        def tensor_backward(t, *a, **k):
            self.backwards += 1
            return tb(t, *a, **k)

        def autograd_backward(*a, **k):
            self.backwards += 1
            return ab(*a, **k)

        monkeypatch.setattr(pkg.ops, "_launch", launch)
        monkeypatch.setattr(torch.Tensor, "backward", tensor_backward)
        monkeypatch.setattr(torch.autograd, "backward", autograd_backward)
        self.forwards = lambda: sum(n.startswith("gcn_panel_train_forward[") for n in self.names)
        self.native_backwards = lambda: sum(n.startswith("gcn_panel_train_backward[") for n in self.names)
        self.panel_calls = lambda: [n for n in self.names if n.startswith("gcn_panel_train_")]


AUTOGRAD_ROUTE = ("gemm_tn", "colsum", "act_bwd", "dropout", "gcn_panel_layer[", "gcn_panel_pack")      # launches of GCNLayerFn


@pytest.fixture(scope="module")
def molecules(pkg):
    return pkg.synthetic_qm9(300, seed=2, num_tasks=2)


def _model(pkg, ms, cuda, keys, config, **args):
    cfg = dict(config, batch_size=2000, random_seed=3)
    for k in keys:
        cfg[k] = True
    a = {"--quiet": True, "--device": str(cuda), "train_data": ms, "valid_data": ms, "--config": json.dumps(cfg)}
    a.update(args)
    return pkg.SparseGCNChemModel(a)


def _randomise(model, seed=0):
    """Random weights and NON-ZERO biases (the fresh model's are zero, which hides db errors)."""
    rng = np.random.default_rng(seed)
    D, L = model.params["hidden_size"], model.params["num_timesteps"]
    model.set_graph_weights([(rng.standard_normal((D, D)) * np.sqrt(2.0 / D)).astype(np.float32) for _ in range(L)],
                            [(rng.standard_normal(D) * 0.1).astype(np.float32) for _ in range(L)])


def _state_masks(pkg, model, feed, cuda):
    """The dropout factors (0 or 1/keep) the NEXT train_batch applies to the hidden layers' states, restated through ops.dropout on
    ones; None without state dropout."""
    keep = float(feed.get("graph_state_keep_prob", 1.0))
    L = model.params["num_timesteps"]
    if keep >= 1.0:
        return None
    V, D = feed["initial_node_representation"].shape
    ones = torch.ones((V, D), device=cuda)
    return [pkg.ops.dropout(ones, keep, model.dropout_seed("gcn_state", l), feed["node_uid"]).cpu().numpy().astype(np.float64)
            for l in range(L - 1)] + [None]


def _seeded_feed(model, seed=17):
    np.random.seed(seed)
    return next(iter(model.make_minibatch_iterator(model.train_data, True)))


def _alias(grads):
    """train_reference.assert_comparison_has_teeth looks for the sparse model's edge-weight name: give the GCN weights it."""
    return {(k + " /gnn_edge_weights_0" if "/gcn_weights_" in k else k): t for k, t in grads.items()}


STEP_CONFIGS = [{"hidden_size": 128, "num_timesteps": 2, "gcn_use_bias": True, "task_ids": [0, 1], "task_sample_ratios": {"1": 0.5}},
                {"hidden_size": 192, "graph_state_dropout_keep_prob": 0.8, "gcn_use_bias": True},
                {"hidden_size": 256},
                {"hidden_size": 256, "num_timesteps": 1}]


@pytest.mark.parametrize("config", STEP_CONFIGS)
def test_panel_native_step_gradients_against_fp64(pkg, oracle_torch, cuda, monkeypatch, molecules, config):
    """One train_batch under both keys: every variable's gradient as the optimiser consumes it against float64 at the project bound
    (train_reference.assert_gradients_match), the loss within 1e-5 relative; one native forward and one native backward call on the
    panel entry points, no launch of the autograd route and no autograd backward."""
    m = _model(pkg, molecules, cuda, (NATIVE, PANEL), config)
    _randomise(m)
    assert m.gcn_panel_route()
    assert pkg.train_native.gcn_model_eligible(m) and not pkg.train_native.model_eligible(m)
    assert m.threaded_batches_default() is False
    feed = _seeded_feed(m)
    assert pkg.train_native.gcn_eligible(m, feed)
    assert float(feed["graph_state_keep_prob"]) == config.get("graph_state_dropout_keep_prob", 1.0)
    masks = _state_masks(pkg, m, feed, cuda)
    want_loss, want = GR.model_fp64_step(oracle_torch, m, feed, masks)
    rec = _Recorder(pkg, monkeypatch)
    with TR.capture_step_gradients(m) as steps:
        loss = float(m.train_batch(feed))
    L = m.params["num_timesteps"]
    assert rec.names.count("gcn_panel_train_forward[L=%d]" % L) == 1 and rec.names.count("gcn_panel_train_backward[L=%d]" % L) == 1
    assert rec.forwards() == 1 and rec.native_backwards() == 1
    assert not [n for n in rec.names if n.startswith(AUTOGRAD_ROUTE)], rec.names
    assert not [n for n in rec.names if n.startswith("gcn_train_")], rec.names
    assert rec.backwards == 0
    print("loss", loss, "float64", want_loss)
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    got = steps[0]
    assert set(got) == set(want) and ("graph_model/gcn_scope/gcn_bias_0:0" in got) == bool(config.get("gcn_use_bias"))
    print({k: v for k, v in TR.normwise_errors({k: t.cpu() for k, t in got.items()}, want).items()})
    TR.assert_gradients_match(got, want)
    TR.assert_comparison_has_teeth(_alias(got), _alias(want))
    # model.ops / model.output as the autograd route leaves them
    assert tuple(m.ops["final_node_representations"].shape) == tuple(feed["initial_node_representation"].shape)
    assert float(m.ops["loss"]) == loss and len(m.ops["losses"]) == len(m.params["task_ids"])
    assert m.output.numel() == feed["num_graphs"]


@pytest.mark.parametrize("config", STEP_CONFIGS[:3])
def test_panel_native_step_against_the_autograd_panel_route(pkg, oracle_torch, cuda, molecules, config):
    """Same seeded feed and weights with gcn_panel_layers on both sides and native_training off / on: the loss and the readout
    variables' gradients bit for bit (the same forward launches on the same bits), each gcn_bias_* gradient bit for bit
    (ggnn_colsum_f32 of the same dP bits on both routes, which test_panel_layer_bwd_equals_its_composition guarantees), each
    gcn_weights_* gradient -- ggnn_xty_acc_f32 here, ggnn_gemm_tn_f32 there -- apart by at most twice the autograd route's own error
    against float64, normwise and max-abs (the rule of test_gpu_gcn_native.test_native_step_against_the_autograd_route).

    Measured on an MI355X (normwise / max-abs): the gcn_weights_* gradients are apart by 1.0e-7 .. 2.2e-7 / 1.6e-7 .. 6.4e-7, the
    autograd panel route against float64 1.3e-7 .. 4.1e-7 / 1.6e-7 .. 5.0e-7 (the native route against float64 1.3e-7 .. 4.2e-7 /
    2.2e-7 .. 5.7e-7); the closest pair is gcn_weights_0 at hidden size 128, apart 2.41e-7 max-abs against 2 x 1.62e-7.  The rule
    holds at the wide sizes as stated."""
    out = {}
    for native in (False, True):
        m = _model(pkg, molecules, cuda, (NATIVE, PANEL) if native else (PANEL,), config)
        _randomise(m)
        assert m.gcn_panel_route()
        feed = _seeded_feed(m)
        assert pkg.train_native.gcn_eligible(m, feed) == native
        want = GR.model_fp64_step(oracle_torch, m, feed, _state_masks(pkg, m, feed, cuda))[1]
        with TR.capture_step_gradients(m) as steps:
            loss = float(m.train_batch(feed))
        out[native] = (loss, steps[0], want)
    (la, ga, want), (ln, gn, _) = out[False], out[True]
    assert la == ln
    assert set(ga) == set(gn)
    graph = [k for k in ga if k.startswith("graph_model/")]
    assert len(graph) == m.params["num_timesteps"] * (2 if config.get("gcn_use_bias") else 1)
    for k in ga:
        if k not in graph or "/gcn_bias_" in k:
            assert torch.equal(_bits(ga[k]), _bits(gn[k])), k
    weights = [k for k in graph if "/gcn_weights_" in k]
    assert len(weights) == m.params["num_timesteps"]
    own = TR.normwise_errors({k: ga[k].cpu() for k in weights}, {k: want[k] for k in weights})
    native_own = TR.normwise_errors({k: gn[k].cpu() for k in weights}, {k: want[k] for k in weights})
    for k in weights:
        w = want[k].double()
        d = gn[k].cpu().double().reshape(w.shape) - ga[k].cpu().double().reshape(w.shape)
        apart = (float(d.norm() / w.norm()), float(d.abs().max() / w.abs().max()))
        print(k, "apart", apart, "autograd route against float64", own[k], "native route against float64", native_own[k])
        assert apart[0] <= 2 * own[k][0] and apart[1] <= 2 * own[k][1], (k, apart, own[k])


def _seeded_steps(pkg, cuda, ms, n, keys, config, timing=False, **args):
    m = _model(pkg, ms, cuda, keys, config, **args)
    _randomise(m, seed=1)
    np.random.seed(11)
    feeds = list(m.make_minibatch_iterator(m.train_data, True))[:n]
    assert len(feeds) == n
    with TR.capture_step_gradients(m) as steps:
        if timing:
            with pkg.ops.kernel_timing():
                losses = [float(m.train_batch(f)) for f in feeds]
        else:
            losses = [float(m.train_batch(f)) for f in feeds]
    return losses, steps, {k: t.detach().clone() for k, t in m.named_variables().items()}


def _assert_same_bits(a, b):
    assert a[0] == b[0]
    assert len(a[1]) == len(b[1])
    for sa, sb in zip(a[1], b[1]):
        assert set(sa) == set(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_panel_native_seeded_steps_are_deterministic(pkg, cuda, monkeypatch, molecules):
    config = {"hidden_size": 256, "graph_state_dropout_keep_prob": 0.8, "gcn_use_bias": True}
    rec = _Recorder(pkg, monkeypatch)
    runs = [_seeded_steps(pkg, cuda, molecules, 3, (NATIVE, PANEL), config) for _ in range(2)]
    assert rec.forwards() == 6 and rec.native_backwards() == 6 and rec.backwards == 0
    _assert_same_bits(*runs)


@pytest.mark.parametrize("case", ["native_alone_128", "hidden_size_160", "freeze_graph_model", "kernel_timing"])
def test_steps_the_panel_native_route_cannot_take_fall_back(pkg, cuda, monkeypatch, molecules, case):
    """native_training alone at 128 (the composed autograd step), both keys at a hidden size without the panel kernel, with frozen
    graph variables, or with per-launch timing active: a seeded step equals the step of the same model without native_training bit
    for bit and issues no gcn_panel_train_* call (nor a gcn_train_* one)."""
    config = {"hidden_size": 160 if case == "hidden_size_160" else 128, "gcn_use_bias": True}
    args = {"--freeze-graph-model": True} if case == "freeze_graph_model" else {}
    timing = case == "kernel_timing"
    other = () if case == "native_alone_128" else (PANEL,)
    rec = _Recorder(pkg, monkeypatch)
    native = _seeded_steps(pkg, cuda, molecules, 1, (NATIVE,) + other, config, timing, **args)
    assert not rec.panel_calls() and not [n for n in rec.names if n.startswith("gcn_train_")]
    assert rec.names and rec.backwards >= 1
    assert any(n.startswith("gcn_panel_layer[") for n in rec.names) == (case in ("freeze_graph_model", "kernel_timing"))
    _assert_same_bits(native, _seeded_steps(pkg, cuda, molecules, 1, other, config, timing, **args))


def test_both_keys_at_100_keep_the_fused_native_route(pkg, cuda, monkeypatch, molecules):
    rec = _Recorder(pkg, monkeypatch)
    _seeded_steps(pkg, cuda, molecules, 1, (NATIVE, PANEL), {"hidden_size": 100, "gcn_use_bias": True})
    assert sum(n.startswith("gcn_train_forward[") for n in rec.names) == 1
    assert sum(n.startswith("gcn_train_backward[") for n in rec.names) == 1
    assert not rec.panel_calls() and rec.backwards == 0


# ---- train() -------------------------------------------------------------------------------------------------------------------
def _train_loop(pkg, cuda, z, log_dir, **extra):
    params = dict(json.loads(str(z["params"])), **{NATIVE: True, PANEL: True, "hidden_size": 128, "num_epochs": 3}, **extra)
    m = pkg.SparseGCNChemModel({"--device": str(cuda), "--log_dir": str(log_dir), "--config": json.dumps(params),
                                "train_data": json.loads(str(z["train_molecules"])),
                                "valid_data": json.loads(str(z["valid_molecules"]))})
    assert m.gcn_panel_route() and pkg.train_native.gcn_model_eligible(m)
    log = m.train()
    with open(m.best_model_file, "rb") as f:
        return log, pickle.load(f), m.train_step_id


def test_device_packing_equals_host_packing_on_the_panel_native_step(pkg, cuda, tmp_path, monkeypatch):
    """pack_on_device and both keys at hidden size 128: the seeded three-epoch train() prints the same log and saves the same
    checkpoint as host packing under the keys, bit for bit; every optimisation step is a native one."""
    z = np.load(GG.path("loop"), allow_pickle=False)
    rec = _Recorder(pkg, monkeypatch)
    (log_h, best_h, steps_h), (log_d, best_d, steps_d) = (_train_loop(pkg, cuda, z, tmp_path / str(dev), pack_on_device=dev)
                                                          for dev in (False, True))
    assert steps_h == steps_d and steps_h > 0
    assert rec.forwards() == rec.native_backwards() == steps_h + steps_d and rec.backwards == 0
    assert not [n for n in rec.names if n.startswith(("gemm_tn", "act_bwd", "gcn_panel_pack"))]
    assert "gcn_assemble_batch" in rec.names
    assert len(log_d) == len(log_h) == 3
    for eh, ed in zip(log_h, log_d):
        for part in ("train_results", "valid_results"):
            assert float(eh[part][0]) == float(ed[part][0]), part
            assert np.isfinite(float(eh[part][0]))
            np.testing.assert_array_equal(np.asarray(eh[part][1]), np.asarray(ed[part][1]))
            np.testing.assert_array_equal(np.asarray(eh[part][2]), np.asarray(ed[part][2]))
    assert set(best_h["weights"]) == set(best_d["weights"])
    for n in best_h["weights"]:
        assert np.asarray(best_h["weights"][n]).tobytes() == np.asarray(best_d["weights"][n]).tobytes(), n
