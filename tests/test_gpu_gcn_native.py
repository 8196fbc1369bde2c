"""GPU tests of the sparse GCN's native training step (params['native_training']): the layer backward with the lower layer's gate in
its epilogue (ggnn_gcn_layer_bwd_f32) against the three launches it replaces and against float64, the one-launch weight pack, and
the step on ggnn_gcn_train_forward_f32 / ggnn_gcn_train_backward_f32 -- gradients against float64, against the autograd route,
determinism, the fallbacks and the reference's recorded runs (chem_tensorflow_gcn.py:62-93, chem_tensorflow.py:183-191)."""
import json
import pickle

import numpy as np
import pytest
import torch

import gcn_golden as GG
import gcn_reference_math as ref
import gcn_train_reference as GR
import reference_golden as RG
import train_reference as TR

pytestmark = pytest.mark.gpu
KEY = "native_training"


def random_ahat(rng, V, nnz_per_row=3.1):
    """test_gpu_gcn.random_ahat restated: asymmetric sparse matrix, row-major sorted, with empty rows, duplicate (i, j) entries and
    negative weights.  -> (adj int64 [nnz, 2], w float32 [nnz])."""
    n = int(V * nnz_per_row)
    rows = rng.integers(0, V, n)
    rows = rows[rows % 7 != 3] if V > 7 else rows                  # rows 3, 10, 17, ... stay empty
    cols = (rows + rng.integers(-20, 21, len(rows))) % V
    adj = np.stack([rows, cols], 1)
    adj = np.concatenate([adj, adj[: len(adj) // 10]])             # duplicates
    w = rng.uniform(-0.3, 0.6, len(adj))
    order = np.lexsort((adj[:, 1], adj[:, 0]))
    return adj[order], w[order].astype(np.float32)


def _bound(adj, w, x, W):
    """test_gpu_gcn._bound: 4e-7 * sum_k |S_k| |W_kn| with |S| = |A| |x|."""
    return 4e-7 * (ref.spmm_abs(adj, w, x) @ np.abs(W.astype(np.float64))) + 1e-30


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def _bwd_inputs(V, D, cuda):
    rng = np.random.default_rng(100 * D + V)
    adj, w = random_ahat(rng, V)
    dP = rng.standard_normal((V, D)).astype(np.float32)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    # the lower layer's forward output dropout(relu(P)): positives, exact zeros and negative zeros
    out = np.maximum(rng.standard_normal((V, D)), 0).astype(np.float32)
    out[rng.random((V, D)) < 0.1] = -0.0
    out[0, :3] = (0.0, -0.0, 1.5)
    keys = rng.integers(0, 2 ** 40, V)
    return adj, w, dP, W, out, keys


@pytest.mark.parametrize("keep", [1.0, 0.75])
@pytest.mark.parametrize("D", [32, 64, 100])
@pytest.mark.parametrize("V", [1, 17, 2000])
def test_layer_bwd_equals_its_composition(pkg, cuda, V, D, keep):
    """One ggnn_gcn_layer_bwd_f32 launch against layer launch on the transposed CSR -> ggnn_dropout_f32 -> ggnn_act_bwd_f32, bit for
    bit; V = 1 is a single row, V = 17 a partial second tile, V = 2000 more than one workgroup's tiles.  At V = 2000 also against
    float64 A_hat^T (dP W^T) * mask * [out > 0] under test_gpu_gcn's bound 4e-7 |A_hat^T| |dP| |W^T|."""
    ops = pkg.ops
    adj, w, dP, W, out, keys = _bwd_inputs(V, D, cuda)
    g = ops.gcn_graph(adj, w, V, cuda)
    t = lambda a: torch.from_numpy(a).to(cuda)
    dPt, Wt, outt = t(dP), t(W), t(out)
    assert bool((outt == 0).any()) and bool(torch.signbit(outt).any()) and bool((outt > 0).any())
    seed = 0x0FED_CBA9_8765_4321
    for row_key in (t(keys), None):
        got = ops.gcn_layer_bwd(dPt, g, Wt, outt, keep, seed, row_key)
        dx = ops.gcn_layer(dPt, g, Wt, transpose=True)[0]
        if keep < 1.0:
            dx = ops.dropout(dx, keep, seed, row_key)
        want = ops.act_bwd(dx, outt, "relu")
        assert torch.equal(got, want), (V, D, keep, row_key is None)
        assert torch.equal(_bits(got), _bits(want)), (V, D, keep, row_key is None)
        assert bool((got != 0).any())
        if V == 2000:
            mask = ops.dropout(torch.ones((V, D), device=cuda), keep, seed, row_key).cpu().numpy().astype(np.float64) if keep < 1.0 else 1.0
            want64 = ref.spmm(adj[:, ::-1], w, dP.astype(np.float64) @ W.astype(np.float64).T) * mask * (out > 0)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want64)
            bound = _bound(adj[:, ::-1], w, dP, W.T)
            print("V=%d D=%d keep=%g: max err / bound = %.3f" % (V, D, keep, float((err / bound).max())))
            assert (err <= bound).all(), float((err / bound).max())
            if keep < 1.0:
                assert 0.1 < float((np.asarray(mask) == 0).mean()) < 0.4


@pytest.mark.parametrize("D", [32, 64, 100])
@pytest.mark.parametrize("L", [1, 3])
def test_train_pack_equals_single_packs(pkg, cuda, L, D):
    rng = np.random.default_rng(L * 1000 + D)
    Ws = [torch.from_numpy(rng.standard_normal((D, D)).astype(np.float32)).to(cuda) for _ in range(L)]
    images = pkg.ops.gcn_train_pack(Ws)
    n = pkg._lib.load().ggnn_gcn_image_bytes(D) // 4
    assert images.shape[0] == 2 * L - 1 and images.shape[1] >= n
    for l in range(L):
        assert torch.equal(_bits(images[l, :n]), _bits(pkg.ops.gcn_pack(Ws[l]))), l
        if l >= 1:
            assert torch.equal(_bits(images[L + l - 1, :n]), _bits(pkg.ops.gcn_pack(Ws[l], True))), l


# ---- the step ------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Names of the launches ops._launch issues and the autograd backward passes entered (the pattern of test_gpu_dense_native.py)."""

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
        self.forwards = lambda: sum(n.startswith("gcn_train_forward[") for n in self.names)
        self.native_backwards = lambda: sum(n.startswith("gcn_train_backward[") for n in self.names)


AUTOGRAD_ROUTE = ("gemm_tn", "colsum", "act_bwd", "dropout", "gcn_layer", "gcn_pack")      # launches of GCNLayerFn


def _molecules(pkg):
    return pkg.synthetic_qm9(300, seed=2, num_tasks=2)


def _model(pkg, ms, cuda, native, config, **args):
    cfg = dict(config, batch_size=2000, random_seed=3)
    if native:
        cfg[KEY] = True
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
    ones (as test_gpu_gcn.test_backward_against_fp64 does); None without state dropout."""
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


STEP_CONFIGS = [{"hidden_size": 100},
                {"hidden_size": 64, "num_timesteps": 2, "gcn_use_bias": True, "task_ids": [0, 1], "task_sample_ratios": {"1": 0.5}},
                {"hidden_size": 32, "graph_state_dropout_keep_prob": 0.8, "gcn_use_bias": True},
                {"hidden_size": 32, "num_timesteps": 1}]


@pytest.mark.parametrize("config", STEP_CONFIGS)
def test_native_step_gradients_against_fp64(pkg, oracle_torch, cuda, monkeypatch, config):
    """One train_batch under the key: every variable's gradient as the optimiser consumes it against float64 at the project bound
    (2e-4 max|want| + 1e-7), the loss within 1e-5 relative; one native forward and one native backward call, no launch of the
    autograd route and no autograd backward."""
    m = _model(pkg, _molecules(pkg), cuda, True, config)
    _randomise(m)
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
    assert rec.names.count("gcn_train_forward[L=%d]" % L) == 1 and rec.names.count("gcn_train_backward[L=%d]" % L) == 1
    assert rec.forwards() == 1 and rec.native_backwards() == 1
    assert not [n for n in rec.names if n.startswith(AUTOGRAD_ROUTE)], rec.names
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
    for t in m.params["task_ids"]:
        assert np.isfinite(float(m.ops["accuracy_task%i" % t]))


@pytest.mark.parametrize("config", STEP_CONFIGS[:3])
def test_native_step_against_the_autograd_route(pkg, oracle_torch, cuda, config):
    """Same seeded feed and weights with and without the key: the loss and the readout variables' gradients bit for bit (the same
    kernels on the same final states); each gcn_weights_* / gcn_bias_* gradient -- ggnn_xty_acc_f32 here, ggnn_gemm_tn_f32
    there, ggnn_colsum_f32 on both -- apart by at most twice the autograd route's own error against float64, normwise and max-abs (the rule
    of test_gpu_dense_native.test_native_step_against_the_autograd_graph_resident_route).

    Measured on an MI355X (normwise / max-abs): the gcn_weights_* gradients are apart by 1.0e-7 .. 1.3e-7 / 1.3e-7 .. 2.9e-7, the
    autograd route against float64 1.0e-7 .. 3.3e-7 / 1.4e-7 .. 5.0e-7.  The bias gradients are ggnn_colsum_f32 of the same dP bits on
    both routes: apart 0.  (Taken from the ones row of ggnn_xty_acc_f32 they were apart by up to 1.09e-7 / 1.89e-7 against an own error
    of 4.98e-8 / 6.33e-8 and missed the rule in two configs, which is why the native backward does not use the ones row.)"""
    ms = _molecules(pkg)
    out = {}
    for native in (False, True):
        m = _model(pkg, ms, cuda, native, config)
        _randomise(m)
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
        if k not in graph:
            assert torch.equal(ga[k], gn[k]), k
    own = TR.normwise_errors({k: ga[k].cpu() for k in graph}, {k: want[k] for k in graph})
    for k in graph:
        w = want[k].double()
        d = gn[k].cpu().double().reshape(w.shape) - ga[k].cpu().double().reshape(w.shape)
        apart = (float(d.norm() / w.norm()), float(d.abs().max() / w.abs().max()))
        print(k, "apart", apart, "autograd route against float64", own[k])
        assert apart[0] <= 2 * own[k][0] and apart[1] <= 2 * own[k][1], (k, apart, own[k])


def _seeded_steps(pkg, cuda, ms, n, native, config, timing=False, **args):
    m = _model(pkg, ms, cuda, native, config, **args)
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


def test_native_seeded_steps_are_deterministic(pkg, cuda, monkeypatch):
    config = {"hidden_size": 100, "graph_state_dropout_keep_prob": 0.8, "gcn_use_bias": True}
    rec = _Recorder(pkg, monkeypatch)
    runs = [_seeded_steps(pkg, cuda, _molecules(pkg), 3, True, config) for _ in range(2)]
    assert rec.forwards() == 6 and rec.native_backwards() == 6
    _assert_same_bits(*runs)


@pytest.mark.parametrize("case", ["hidden_size_48", "freeze_graph_model", "kernel_timing"])
def test_steps_the_native_route_cannot_take_fall_back(pkg, cuda, monkeypatch, case):
    """With the key set but no native kernels for the hidden size, frozen graph variables, or per-launch timing active, a seeded step
    equals the step of a model without the key bit for bit and issues no native call."""
    config = {"hidden_size": 48 if case == "hidden_size_48" else 32, "gcn_use_bias": True}
    args = {"--freeze-graph-model": True} if case == "freeze_graph_model" else {}
    timing = case == "kernel_timing"
    ms = _molecules(pkg)
    rec = _Recorder(pkg, monkeypatch)
    native = _seeded_steps(pkg, cuda, ms, 1, True, config, timing, **args)
    assert rec.forwards() == 0 and rec.native_backwards() == 0 and rec.names and rec.backwards >= 1
    _assert_same_bits(native, _seeded_steps(pkg, cuda, ms, 1, False, config, timing, **args))


# ---- the reference's recorded runs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GG.CASES)
def test_training_follows_reference_run_on_the_native_step(pkg, cuda, tmp_path, monkeypatch, case):
    """test_gpu_gcn_reference_golden.test_training_follows_reference_run under the key, its tolerances copied; the checkpoint's params
    get the key first (restore_progress compares the params' lengths).  Case h48 has no native kernels: it falls back."""
    g = GG.GCNGolden(case)
    path = g.write_checkpoint(str(tmp_path / "ref.pickle"))
    with open(path, "rb") as f:
        ckpt = pickle.load(f)
    ckpt["params"] = dict(ckpt["params"], **{KEY: True})
    with open(path, "wb") as f:
        pickle.dump(ckpt, f)
    args = g.model_args(str(cuda), **{"--restore": path})
    args["--config"] = json.dumps(dict(g.params, **{KEY: True}))
    m = pkg.SparseGCNChemModel(args)
    for n, t in m.named_variables().items():
        np.testing.assert_array_equal(t.detach().cpu().numpy().reshape(g.weights[n].shape), g.weights[n])
    batches = list(m.make_minibatch_iterator(m.train_data, False))
    rec = _Recorder(pkg, monkeypatch)
    losses = []
    for s in range(len(g.z["train_losses"])):
        b = batches[s % len(batches)]
        GG.assert_feed_equal(b, g.feed("train%d" % s))
        losses.append(float(m.train_batch(b)))
    if case == "h48":
        assert rec.forwards() == 0 and rec.native_backwards() == 0 and rec.backwards >= len(losses)
    else:
        assert rec.forwards() == rec.native_backwards() == len(losses) and rec.backwards == 0
    np.testing.assert_allclose(losses, g.z["train_losses"], rtol=5e-4)
    nv = m.named_variables()
    for i, n in enumerate(g.names):
        a = nv[n].detach().cpu().numpy()
        np.testing.assert_allclose(RG.stats(a), g.z["trained_stats"][i], rtol=1e-3, atol=5e-3, err_msg=n)
        if "trained/" + n in g.z.files:
            np.testing.assert_allclose(a.reshape(g.z["trained/" + n].shape), g.z["trained/" + n], rtol=1e-2, atol=3e-3, err_msg=n)


def _train_loop(pkg, cuda, z, log_dir, **extra):
    params = dict(json.loads(str(z["params"])), **{KEY: True}, **extra)
    m = pkg.SparseGCNChemModel({"--device": str(cuda), "--log_dir": str(log_dir), "--config": json.dumps(params),
                                "train_data": json.loads(str(z["train_molecules"])),
                                "valid_data": json.loads(str(z["valid_molecules"]))})
    log = m.train()
    with open(m.best_model_file, "rb") as f:
        return log, pickle.load(f), params


def test_train_loop_reproduces_reference_log_on_the_native_step(pkg, cuda, tmp_path, monkeypatch):
    """test_gpu_gcn_reference_golden.test_train_loop_reproduces_reference_log under the key, its tolerances copied; the checkpoint's
    params are the fixture's plus the key."""
    z = np.load(GG.path("loop"), allow_pickle=False)
    rec = _Recorder(pkg, monkeypatch)
    log, best, params = _train_loop(pkg, cuda, z, tmp_path)
    assert rec.forwards() > 0 and rec.forwards() == rec.native_backwards() and rec.backwards == 0
    assert len(log) == len(z["train_loss"])
    np.testing.assert_allclose([e["train_results"][0] for e in log], z["train_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["train_results"][1] for e in log], z["train_accuracy"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][0] for e in log], z["valid_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][1] for e in log], z["valid_accuracy"], rtol=1e-3)
    assert best["params"] == params and best["params"][KEY] is True
    assert (best["train_step"], best["valid_step"]) == (int(z["best_train_step"]), int(z["best_valid_step"]))
    names = [str(n) for n in z["best_names"]]
    assert set(best["weights"]) - {"ggnn_amd/adam_step:0"} == set(names)
    for i, n in enumerate(names):
        a = np.asarray(best["weights"][n], dtype=np.float64)
        want = z["best_stats"][i]
        np.testing.assert_allclose(RG.stats(a)[1:], want[1:], rtol=2e-3, atol=1e-6, err_msg=n)
        assert abs(RG.stats(a)[0] - want[0]) <= 2e-3 * max(want[1], 1e-3), n


def test_device_packing_equals_host_packing_on_the_native_step(pkg, cuda, tmp_path, monkeypatch):
    """pack_on_device and the key both set: the seeded three-epoch train() prints the same log and saves the same checkpoint as host
    packing under the key, bit for bit."""
    z = np.load(GG.path("loop"), allow_pickle=False)
    rec = _Recorder(pkg, monkeypatch)
    (log_h, best_h, _), (log_d, best_d, _) = (_train_loop(pkg, cuda, z, tmp_path / str(dev), pack_on_device=dev) for dev in (False, True))
    assert rec.forwards() > 0 and rec.forwards() == rec.native_backwards() and rec.backwards == 0
    assert "gcn_assemble_batch" in rec.names
    assert len(log_d) == len(log_h) == len(z["train_loss"])
    for eh, ed in zip(log_h, log_d):
        for part in ("train_results", "valid_results"):
            assert float(eh[part][0]) == float(ed[part][0]), part
            np.testing.assert_array_equal(np.asarray(eh[part][1]), np.asarray(ed[part][1]))
            np.testing.assert_array_equal(np.asarray(eh[part][2]), np.asarray(ed[part][2]))
    assert set(best_h["weights"]) == set(best_d["weights"])
    for n in best_h["weights"]:
        assert np.asarray(best_h["weights"][n]).tobytes() == np.asarray(best_d["weights"][n]).tobytes(), n
