"""GPU tests of the native training step of the sparse GGNN with the BasicRNNCell (params['compact_rnn'] == 'native';
train_native.ROUTES, entry `rnn`, on ggnn_sparse_rnn_train_forward_f32 / ggnn_sparse_rnn_train_backward_f32): gradients against
float64 with the cell's kernel and bias as leaves, the route taken, the step against the key-True route (variants.CompactRnnStepFn),
determinism, consecutive steps, the fall-backs and the reference's recorded run (chem_tensorflow_sparse.py:109-110, 117-218,
chem_tensorflow.py:183-191).

ReLU: the hand-written backward gates by the sign of the kernel's float32 output, float64 autograd by the sign of its own
pre-activation; where a pre-activation lies within float32 rounding of 0 the derivative is not a property of the inputs
(tests/test_gpu_rnn_route.py).  So a ReLU config draws its weights with the first seed in 0 .. 7 for which every pre-activation of
the step stays beyond twice its a-priori float32 rounding bound (test_gpu_rnn_route._kink_recorder), evaluated on a key-True model
-- whose states are the same bits as the native step's.  No such seed: the test fails."""
from importlib import import_module

import numpy as np
import pytest
import torch

import reference_golden as RG
import rnn_train_reference as RR
import train_reference as TR
from test_gpu_gcn_native import _Recorder, _assert_same_bits
from test_gpu_rnn_route import README, _kink_recorder

pytestmark = pytest.mark.gpu
KEY = "compact_rnn"
FORWARD, BACKWARD = "sparse_rnn_train_forward[", "sparse_rnn_train_backward["
# launches of the key-True route's step (variants.CompactRnnStepFn / _hip_backward, backward.transform_backward / weight_grad)
AUTOGRAD_ROUTE = ("msg_transform_compact", "rnn_fused_gather", "act_bwd", "bwd_dx", "xty", "gemm_tn", "colsum", "gather_segment_sum",
                  "rnn_bwd_fused")
KINK_FACTOR = 2.0

STEP_CONFIGS = [
    (dict(README, hidden_size=100), 1.0),
    ({"graph_rnn_cell": "RNN", "hidden_size": 64, "graph_rnn_activation": "tanh", "use_edge_msg_avg_aggregation": False,
      "layer_timesteps": [2, 1], "residual_connections": {"1": [0]}, "task_ids": [0, 1], "task_sample_ratios": {"1": 0.5, 1: 0.5},
      "multitask_readout": True}, 1.0),
    (dict(README, hidden_size=32, edge_weight_dropout_keep_prob=0.8), 0.8),
    (dict(README, hidden_size=32, layer_timesteps=[1]), 1.0),
]
STEP_IDS = ["readme-h100", "h64-tanh-sum-residual-two-tasks-multitask", "h32-edge-dropout", "h32-one-step"]


def _native_calls(rec):
    return (sum(n.startswith(FORWARD) for n in rec.names), sum(n.startswith(BACKWARD) for n in rec.names))


@pytest.fixture(scope="module")
def molecules(pkg):
    return pkg.synthetic_qm9(80, mean_nodes=10, seed=6, num_tasks=2)


def _model(pkg, oracle, ms, cuda, key, config, seed=6, **args):
    cfg = dict(config)
    if key is not None:
        cfg[KEY] = key
    a = {"--quiet": True, "--device": str(cuda), "train_data": ms, "valid_data": ms, "--config": cfg}
    a.update(args)
    model = pkg.SparseGGNNChemModel(a)
    layers = oracle.make_sparse_layers(np.random.default_rng(seed), model.params, model.num_edge_types, random_bias=True)
    model.set_graph_weights(layers)
    return model


def _feed(model, edge_keep):
    feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=False))))
    feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"] = edge_keep, 1.0
    return feed


_SEEDS = {}


def _weight_seed(pkg, oracle, ms, cuda, monkeypatch, config, edge_keep):
    """The weight seed of a config: 6 for tanh; for ReLU the first of 0 .. 7 whose step keeps every pre-activation off the kink (see
    the module docstring), found once per config on throw-away key-True models."""
    if str(config.get("graph_rnn_activation", "tanh")).lower() != "relu":
        return 6
    ident = repr(sorted(config.items(), key=str)) + repr(edge_keep)
    if ident not in _SEEDS:
        variants = import_module(pkg.__name__ + ".variants")
        tried = []
        for seed in range(8):
            ratios = []
            with monkeypatch.context() as mp:
                _kink_recorder(variants, mp, ratios)
                m = _model(pkg, oracle, ms, cuda, True, config, seed=seed)
                m.train_batch(_feed(m, edge_keep))
                torch.cuda.synchronize()
            assert len(ratios) == sum(m.params["layer_timesteps"])
            tried.append((seed, min(ratios)))
            if min(ratios) > KINK_FACTOR:
                _SEEDS[ident] = seed
                break
        else:
            raise AssertionError("no weight seed in 0 .. 7 keeps every ReLU pre-activation off the kink: %s" % tried)
        print("weight seed %d: smallest |pre| / rounding bound %.3g (tried %s)" % (seed, min(ratios), tried))
    return _SEEDS[ident]


def _fp64(oracle, oracle_torch, model, feed):
    """Loss, gradients and dropout masks of the step train_batch is about to take (take them first: train_batch advances the
    dropout step)."""
    masks = TR.dropout_masks(oracle, model, feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"])
    return RR.oracle_loss_and_grads(oracle_torch, model, feed, masks) + (masks,)


@pytest.mark.parametrize("config,edge_keep", STEP_CONFIGS, ids=STEP_IDS)
def test_native_step_gradients_against_fp64(pkg, oracle, oracle_torch, cuda, molecules, monkeypatch, config, edge_keep):
    """One train_batch under the key: every variable's gradient as the optimiser consumes it against float64 autograd of the oracle
    at the project bound (2e-4 max|want| + 1e-7), the loss within 1e-5 relative; exactly one native forward and one native backward
    call, no launch named as the key-True route names its own, no autograd backward."""
    seed = _weight_seed(pkg, oracle, molecules, cuda, monkeypatch, config, edge_keep)
    m = _model(pkg, oracle, molecules, cuda, "native", config, seed=seed)
    assert m.rnn_route() and pkg.train_native.rnn_model_eligible(m) and not pkg.train_native.model_eligible(m)
    assert m.threaded_batches_default() is False
    feed = _feed(m, edge_keep)
    assert pkg.train_native.rnn_eligible(m, feed) and not pkg.train_native.eligible(m, feed)
    want_loss, want, masks = _fp64(oracle, oracle_torch, m, feed)
    rec = _Recorder(pkg, monkeypatch)
    with TR.capture_step_gradients(m) as steps:
        loss = float(m.train_batch(feed))
    torch.cuda.synchronize()
    total = sum(m.params["layer_timesteps"])
    assert rec.names.count("%ssteps=%d]" % (FORWARD, total)) == 1 and rec.names.count("%ssteps=%d]" % (BACKWARD, total)) == 1
    assert _native_calls(rec) == (1, 1)
    assert not [n for n in rec.names if n.startswith(AUTOGRAD_ROUTE)], rec.names
    assert rec.backwards == 0
    print("loss", loss, "float64", want_loss)
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    got = steps[0]
    L = len(m.params["layer_timesteps"])
    assert set(got) == set(want) and sum("basic_rnn_cell" in k for k in got) == 2 * L
    print(TR.normwise_errors({k: t.cpu() for k, t in got.items()}, want))
    TR.assert_gradients_match(got, want)
    TR.assert_comparison_has_teeth(got, want)
    for l in range(L):                         # the cell's gradients are real ones
        assert float(want["graph_model/gnn_layer_%i/timestep_0/basic_rnn_cell/kernel:0" % l].abs().max()) > 0
    if edge_keep < 1.0:
        for l, mask in enumerate(masks["edge"]):
            g = got["graph_model/gnn_layer_%i/gnn_edge_weights_%i:0" % (l, l)].cpu().numpy()
            assert (g[mask == 0] == 0).all() and 0.1 < float((mask == 0).mean()) < 0.3
    # model.ops / model.output as the autograd route leaves them
    assert tuple(m.ops["final_node_representations"].shape) == tuple(feed["initial_node_representation"].shape)
    assert float(m.ops["loss"]) == loss and len(m.ops["losses"]) == len(m.params["task_ids"])
    for t in m.params["task_ids"]:
        assert np.isfinite(float(m.ops["accuracy_task%i" % t]))
    assert m.output is not None


@pytest.mark.parametrize("config,edge_keep", STEP_CONFIGS, ids=STEP_IDS)
def test_native_step_against_the_key_true_route(pkg, oracle, oracle_torch, cuda, molecules, monkeypatch, config, edge_keep):
    """Same seeded feed and weights under compact_rnn True and 'native': the final node states, the loss and the readout variables'
    gradients bit for bit (the same forward launches on the same weight images); each graph-model gradient -- the cell's input
    gradients come from ggnn_rnn_bwd_fused_f32 here and from ggnn_bwd_dx_f32 there, the products are ggnn_xty_acc_f32 into the
    gradient views here and ggnn_xty_f32 per timestep summed by autograd there, merged over a residual-free layer's timesteps here
    -- apart by at most twice the key-True route's own error against float64, normwise and max-abs (the rule of
    test_gpu_gcn_native.test_native_step_against_the_autograd_route).

    Measured on an MI355X (worst variable of each config, normwise / max-abs): apart 1.3e-7 / 2.1e-7 (README, h100), 1.6e-7 / 2.3e-7
    (h64, tanh, sum, residual), 2.7e-7 / 2.8e-7 (h32, edge dropout), 7.6e-8 / 1.2e-7 (h32, one step); the key-True route against
    float64 3.1e-7 / 5.6e-7, 3.5e-7 / 4.2e-7, 2.9e-7 / 4.5e-7, 9.3e-8 / 1.3e-7.  Final states, losses and readout gradients are equal
    bit for bit in all four.  With the split format's six piece products in the cell backward (instead of the eight it runs now:
    csrc/ggnn_rnn_fused.hip) the two eight-layer configs were apart 4.0e-7 / 4.8e-7 and 4.3e-7 / 5.6e-7 and failed this rule at layer
    0 (bias: 3.9e-7 / 3.5e-7 against an own error of 2.2e-7 / 1.7e-7): the dropped terms all have the sign of their product, and the
    shortfall adds up over the layers."""
    seed = _weight_seed(pkg, oracle, molecules, cuda, monkeypatch, config, edge_keep)
    out = {}
    for key in (True, "native"):
        m = _model(pkg, oracle, molecules, cuda, key, config, seed=seed)
        feed = _feed(m, edge_keep)
        assert pkg.train_native.rnn_eligible(m, feed) == (key == "native")
        want = _fp64(oracle, oracle_torch, m, feed)[1]
        with TR.capture_step_gradients(m) as steps:
            loss = float(m.train_batch(feed))
        torch.cuda.synchronize()
        out[key] = (loss, steps[0], want, m.ops["final_node_representations"].detach().clone())
    (la, ga, want, fa), (ln, gn, _, fn) = out[True], out["native"]
    assert torch.equal(fa, fn) and torch.equal(fa.view(torch.int32), fn.view(torch.int32))
    assert la == ln
    assert set(ga) == set(gn)
    graph = [k for k in ga if k.startswith("graph_model/")]
    assert len(graph) == 3 * len(m.params["layer_timesteps"])
    for k in ga:
        if k not in graph:
            assert torch.equal(ga[k], gn[k]), k
    own = TR.normwise_errors({k: ga[k].cpu() for k in graph}, {k: want[k] for k in graph})
    worst = [0.0, 0.0, 0.0, 0.0]
    apart = {}
    for k in graph:
        w = want[k].double()
        d = gn[k].cpu().double().reshape(w.shape) - ga[k].cpu().double().reshape(w.shape)
        apart[k] = (float(d.norm() / w.norm()), float(d.abs().max() / w.abs().max()))
        print(k, "apart", apart[k], "key-True route against float64", own[k])
        worst = [max(a, b) for a, b in zip(worst, apart[k] + tuple(own[k]))]
    print("worst apart %.3e / %.3e, worst own error %.3e / %.3e" % tuple(worst))
    for k in graph:
        assert apart[k][0] <= 2 * own[k][0] and apart[k][1] <= 2 * own[k][1], (k, apart[k], own[k])


def _seeded_steps(pkg, oracle, cuda, ms, n, key, config, timing=False, **args):
    m = _model(pkg, oracle, ms, cuda, key, config, seed=1, **args)
    np.random.seed(11)
    feeds = []
    for _ in range(n):                                    # (a training epoch of this data is one batch: n seeded epochs)
        feeds += list(m.make_minibatch_iterator(m.train_data, True))[:1]
    eligible = [pkg.train_native.rnn_eligible(m, f) for f in feeds]
    with TR.capture_step_gradients(m) as steps:
        if timing:
            with pkg.ops.kernel_timing():
                eligible = [pkg.train_native.rnn_eligible(m, f) for f in feeds]
                losses = [float(m.train_batch(f)) for f in feeds]
        else:
            losses = [float(m.train_batch(f)) for f in feeds]
    torch.cuda.synchronize()
    return (losses, steps, {k: t.detach().clone() for k, t in m.named_variables().items()}), eligible


def test_native_seeded_steps_are_deterministic(pkg, oracle, cuda, molecules, monkeypatch):
    """Three seeded steps (shuffled batches, edge-weight dropout 0.8 from the config) run twice from the same state: identical bits
    for the losses, every captured gradient and every variable afterwards."""
    rec = _Recorder(pkg, monkeypatch)
    runs = [_seeded_steps(pkg, oracle, cuda, molecules, 3, "native", dict(README, hidden_size=100)) for _ in range(2)]
    assert all(all(e) for _, e in runs)
    assert _native_calls(rec) == (6, 6) and rec.backwards == 0
    assert len(runs[0][0][1]) == 3
    _assert_same_bits(runs[0][0], runs[1][0])


def test_three_steps_follow_the_key_true_route(pkg, oracle, cuda, molecules, monkeypatch):
    """Three consecutive steps on one feed (edge-weight dropout 0.8: a new mask per step) under True and 'native': the losses within
    1e-5 relative, the first step's gradients within the project bound of each other (the tolerances of
    test_gpu_rnn_route.test_three_training_steps_follow_the_key_off_route)."""
    config = dict(README, hidden_size=64, edge_weight_dropout_keep_prob=0.8)
    results = []
    for key in (True, "native"):
        m = _model(pkg, oracle, molecules, cuda, key, config, seed=5)
        feed = _feed(m, 0.8)
        rec = _Recorder(pkg, monkeypatch)
        with TR.capture_step_gradients(m) as grads:
            losses = [float(m.train_batch(feed)) for _ in range(3)]
        torch.cuda.synchronize()
        assert _native_calls(rec) == ((3, 3) if key == "native" else (0, 0))
        assert len(grads) == 3
        results.append((losses, grads[0]))
    (l1, g1), (l0, g0) = results
    print("losses key True %s, key 'native' %s" % (l1, l0))
    assert l1[0] == l0[0]                                # (the first step's forward is the same launches on the same weights)
    np.testing.assert_allclose(l0, l1, rtol=1e-5)
    TR.assert_gradients_match(g0, g1)


FALLBACKS = {"h100_residual_nx2": (dict(README, hidden_size=100, layer_timesteps=[2, 1], residual_connections={"1": [0]}), {}),
             "hidden_size_84": (dict(README, hidden_size=84, layer_timesteps=[2, 1]), {}),
             "use_edge_bias": (dict(README, hidden_size=32, layer_timesteps=[2, 1], use_edge_bias=True), {}),
             "graph_state_dropout": (dict(README, hidden_size=32, layer_timesteps=[2, 1], graph_state_dropout_keep_prob=0.8), {}),
             "freeze_graph_model": (dict(README, hidden_size=32, layer_timesteps=[2, 1]), {"--freeze-graph-model": True}),
             "kernel_timing": (dict(README, hidden_size=32, layer_timesteps=[2, 1]), {})}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_steps_the_native_route_cannot_take_fall_back(pkg, oracle, cuda, molecules, monkeypatch, case):
    """With the key 'native' but a layer outside ggnn_rnn_fused_supported (hidden 100 with a residual input: nx = 2), a padded hidden
    size (84 runs at width 100), an edge bias, graph-state dropout, frozen graph variables or per-launch timing active, rnn_eligible
    is False, a seeded step equals the step of the key-True model bit for bit and issues no native call."""
    config, args = FALLBACKS[case]
    timing = case == "kernel_timing"
    rec = _Recorder(pkg, monkeypatch)
    native, eligible = _seeded_steps(pkg, oracle, cuda, molecules, 1, "native", config, timing, **args)
    assert eligible == [False]
    assert _native_calls(rec) == (0, 0) and rec.names and rec.backwards >= 1
    _assert_same_bits(native, _seeded_steps(pkg, oracle, cuda, molecules, 1, True, config, timing, **args)[0])


def test_training_follows_reference_run_on_the_native_step(pkg, cuda, tmp_path, monkeypatch):
    """test_gpu_rnn_route.test_training_follows_reference_run under the key 'native', its tolerance copied; the key goes into the
    model's config and into the checkpoint's params.  The recorded run is hidden 100 with layer_timesteps [2, 2] and a residual
    input into layer 1 (nx = 2 at D = 100: outside ggnn_rnn_fused_supported), so under 'native' it is reproduced through the
    fall-back; the same run with the residual input dropped from the config is eligible and takes the native calls (its losses
    have no recorded counterpart: they are held to the key-True model's)."""
    g = RG.Golden("sparse_relu_rnn")
    g.params = dict(g.params, **{KEY: "native"})
    path = g.write_checkpoint(str(tmp_path / "sparse_relu_rnn.pickle"))
    m = pkg.SparseGGNNChemModel(g.model_args(str(cuda), **{"--restore": path}))
    assert m.rnn_route() and m.params[KEY] == "native"
    assert m.params["hidden_size"] == 100 and m.params["residual_connections"] == {"1": [0]}
    assert not pkg.train_native.rnn_model_eligible(m)
    for n, t in m.named_variables().items():
        np.testing.assert_array_equal(t.detach().cpu().numpy().reshape(g.weights[n].shape), g.weights[n])
    assert len(g.train_losses) == 2
    batches = list(m.make_minibatch_iterator(m.train_data, False))    # unshuffled, keep-probs 1: as recorded
    assert len(batches) == int(g.z["num_train_batches"])
    rec = _Recorder(pkg, monkeypatch)
    losses = [float(m.train_batch(batches[s % len(batches)])) for s in range(len(g.train_losses))]
    assert _native_calls(rec) == (0, 0) and rec.backwards >= 2
    np.testing.assert_allclose(losses, g.train_losses, rtol=5e-4)
    # the recorded weights and data without the residual input: eligible, two native steps, the key-True model's losses
    results = []
    for key in ("native", True):
        g2 = RG.Golden("sparse_relu_rnn")
        g2.params = dict(g2.params, residual_connections={}, **{KEY: key})
        m2 = pkg.SparseGGNNChemModel(g2.model_args(str(cuda)))
        assert pkg.train_native.rnn_model_eligible(m2) == (key == "native")
        with torch.no_grad():
            for n, t in m2.named_variables().items():
                if t.numel() == g.weights[n].size:
                    t.copy_(torch.from_numpy(g.weights[n]).to(t.device).reshape(t.shape))
                else:                                       # layer 1's kernel: its [incoming | h] rows of the recorded [x | incoming | h]
                    assert "gnn_layer_1/timestep_0/basic_rnn_cell/kernel" in n
                    t.copy_(torch.from_numpy(g.weights[n][100:]).to(t.device))
        b2 = list(m2.make_minibatch_iterator(m2.train_data, False))
        rec2 = _Recorder(pkg, monkeypatch)
        results.append([float(m2.train_batch(b2[s % len(b2)])) for s in range(2)])
        assert _native_calls(rec2) == ((2, 2) if key == "native" else (0, 0))
    assert results[0][0] == results[1][0]
    np.testing.assert_allclose(results[0], results[1], rtol=1e-5)
