"""GPU tests of the native training step of the sparse GGNN with propagation attention (params['compact_attention'] == 'native';
train_native.ROUTES, entry `attention`, on ggnn_sparse_attn_train_forward_f32 / ggnn_sparse_attn_train_backward_f32): gradients against
float64 with the attention factors as leaves, the route taken, the step against the key-True route (variants.CompactAttentionStepFn),
determinism, the fall-backs and the reference's recorded run (chem_tensorflow_sparse.py:117-218, chem_tensorflow.py:183-191)."""
import numpy as np
import pytest
import torch

import attention_train_reference as AR
import reference_golden as RG
import train_reference as TR
from test_gpu_gcn_native import _Recorder, _assert_same_bits

pytestmark = pytest.mark.gpu
KEY = "compact_attention"
FORWARD, BACKWARD = "sparse_attn_train_forward[", "sparse_attn_train_backward["
# launches of the key-True route's step (variants.CompactAttentionStepFn / _hip_backward, backward.transform_backward)
AUTOGRAD_ROUTE = ("msg_transform_compact", "gather_segment_sum_attn_compact", "gru_fused", "gru_bwd_fused", "attn_bwd_target_compact",
                  "weighted_segment_sum", "gather_segment_sum", "xty", "attn_bwd_source_compact")

STEP_CONFIGS = [
    ({"hidden_size": 100}, 1.0),
    ({"hidden_size": 64, "use_edge_msg_avg_aggregation": False, "graph_rnn_activation": "ReLU", "task_ids": [0, 1],
      "task_sample_ratios": {"1": 0.5, 1: 0.5}, "multitask_readout": True}, 1.0),
    ({"hidden_size": 32, "edge_weight_dropout_keep_prob": 0.8}, 0.8),
    ({"hidden_size": 32, "layer_timesteps": [1], "residual_connections": {}}, 1.0),
]
STEP_IDS = ["h100-default-layers", "h64-sum-relu-two-tasks-multitask", "h32-edge-dropout", "h32-one-step"]


def _native_calls(rec):
    return (sum(n.startswith(FORWARD) for n in rec.names), sum(n.startswith(BACKWARD) for n in rec.names))


@pytest.fixture(scope="module")
def molecules(pkg):
    return pkg.synthetic_qm9(80, mean_nodes=10, seed=6, num_tasks=2)


def _model(pkg, oracle, ms, cuda, key, config, seed=6, **args):
    cfg = dict(config, use_propagation_attention=True)
    if key is not None:
        cfg[KEY] = key
    a = {"--quiet": True, "--device": str(cuda), "train_data": ms, "valid_data": ms, "--config": cfg}
    a.update(args)
    model = pkg.SparseGGNNChemModel(a)
    layers = oracle.make_sparse_layers(np.random.default_rng(seed), model.params, model.num_edge_types, random_bias=True)
    model.set_graph_weights(layers)           # (random biases and attention factors: the fresh model's are zeros / ones)
    return model


def _feed(model, edge_keep):
    feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=False))))
    feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"] = edge_keep, 1.0
    return feed


def _fp64(oracle, oracle_torch, model, feed):
    """Loss, gradients and dropout masks of the step train_batch is about to take (take them first: train_batch advances the
    dropout step)."""
    masks = TR.dropout_masks(oracle, model, feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"])
    return AR.oracle_loss_and_grads(oracle_torch, model, feed, masks) + (masks,)


@pytest.mark.parametrize("config,edge_keep", STEP_CONFIGS, ids=STEP_IDS)
def test_native_step_gradients_against_fp64(pkg, oracle, oracle_torch, cuda, molecules, monkeypatch, config, edge_keep):
    """One train_batch under the key: every variable's gradient as the optimiser consumes it -- the attention factors' included --
    against float64 autograd of the oracle at the project bound (2e-4 max|want| + 1e-7), the loss within 1e-5 relative; exactly one
    native forward and one native backward call, no launch named as the key-True route names its own, no autograd backward."""
    m = _model(pkg, oracle, molecules, cuda, "native", config)
    assert m.attention_route() and pkg.train_native.attn_model_eligible(m) and not pkg.train_native.model_eligible(m)
    assert m.threaded_batches_default() is False
    feed = _feed(m, edge_keep)
    assert pkg.train_native.attn_eligible(m, feed) and not pkg.train_native.eligible(m, feed)
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
    assert set(got) == set(want) and sum("edge_type_attention_weights" in k for k in got) == L
    print(TR.normwise_errors({k: t.cpu() for k, t in got.items()}, want))
    TR.assert_gradients_match(got, want)
    TR.assert_comparison_has_teeth(got, want)
    for l in range(L):                         # the attention factors' gradient is a real one
        assert float(want["graph_model/gnn_layer_%i/edge_type_attention_weights_%i:0" % (l, l)].abs().max()) > 0
    if edge_keep < 1.0:
        for l, mask in enumerate(masks["edge"]):
            g = got["graph_model/gnn_layer_%i/gnn_edge_weights_%i:0" % (l, l)].cpu().numpy()
            assert (g[mask == 0] == 0).all() and 0.1 < float((mask == 0).mean()) < 0.3
    # model.ops / model.output as the autograd route leaves them
    assert tuple(m.ops["final_node_representations"].shape) == tuple(feed["initial_node_representation"].shape)
    assert float(m.ops["loss"]) == loss and len(m.ops["losses"]) == len(m.params["task_ids"])
    for t in m.params["task_ids"]:
        assert np.isfinite(float(m.ops["accuracy_task%i" % t]))


@pytest.mark.parametrize("config,edge_keep", STEP_CONFIGS[:3], ids=STEP_IDS[:3])
def test_native_step_against_the_key_true_route(pkg, oracle, oracle_torch, cuda, molecules, config, edge_keep):
    """Same seeded feed and weights under compact_attention True and 'native': the final node states, the loss and the readout
    variables' gradients bit for bit (the same kernels on the same weight images); each graph-model gradient -- the products are
    ggnn_xty_acc_f32 into the gradient views here, ggnn_xty_f32 per timestep summed by autograd there, merged over a residual-free
    layer's timesteps here -- apart by at most twice the key-True route's own error against float64, normwise and max-abs (the
    rule of test_gpu_gcn_native.test_native_step_against_the_autograd_route).

    Measured on an MI355X (worst variable of each config, normwise / max-abs): apart 1.1e-7 / 2.1e-7 (h100), 2.6e-7 / 5.8e-7 (h64,
    sum, ReLU), 1.8e-7 / 2.6e-7 (h32, edge dropout); the key-True route against float64 2.0e-7 .. 3.1e-6 / 1.4e-7 .. 3.3e-6 (9.6e-5 /
    1.2e-4 for layer 0's attention factors at h64 with sum aggregation and ReLU); the tightest variable, layer 3's gates kernel at
    h64, is apart 2.1e-7 / 5.8e-7 against an own error of 2.5e-7 / 4.6e-7.  Layers of one timestep are apart 0: the same launches
    in the same order.  Final states, losses and readout gradients are equal bit for bit in all three."""
    out = {}
    for key in (True, "native"):
        m = _model(pkg, oracle, molecules, cuda, key, config)
        feed = _feed(m, edge_keep)
        assert pkg.train_native.attn_eligible(m, feed) == (key == "native")
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
    assert len(graph) == 6 * len(m.params["layer_timesteps"])
    for k in ga:
        if k not in graph:
            assert torch.equal(ga[k], gn[k]), k
    own = TR.normwise_errors({k: ga[k].cpu() for k in graph}, {k: want[k] for k in graph})
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in graph:
        w = want[k].double()
        d = gn[k].cpu().double().reshape(w.shape) - ga[k].cpu().double().reshape(w.shape)
        apart = (float(d.norm() / w.norm()), float(d.abs().max() / w.abs().max()))
        print(k, "apart", apart, "key-True route against float64", own[k])
        worst = [max(a, b) for a, b in zip(worst, apart + tuple(own[k]))]
    print("worst apart %.3e / %.3e, worst own error %.3e / %.3e" % tuple(worst))
    for k in graph:
        w = want[k].double()
        d = gn[k].cpu().double().reshape(w.shape) - ga[k].cpu().double().reshape(w.shape)
        apart = (float(d.norm() / w.norm()), float(d.abs().max() / w.abs().max()))
        assert apart[0] <= 2 * own[k][0] and apart[1] <= 2 * own[k][1], (k, apart, own[k])


def _seeded_steps(pkg, oracle, cuda, ms, n, key, config, timing=False, **args):
    m = _model(pkg, oracle, ms, cuda, key, config, seed=1, **args)
    np.random.seed(11)
    feeds = []
    for _ in range(n):                                    # (a training epoch of this data is one batch: n seeded epochs)
        feeds += list(m.make_minibatch_iterator(m.train_data, True))[:1]
    with TR.capture_step_gradients(m) as steps:
        if timing:
            with pkg.ops.kernel_timing():
                losses = [float(m.train_batch(f)) for f in feeds]
        else:
            losses = [float(m.train_batch(f)) for f in feeds]
    torch.cuda.synchronize()
    return losses, steps, {k: t.detach().clone() for k, t in m.named_variables().items()}


def test_native_seeded_steps_are_deterministic(pkg, oracle, cuda, molecules, monkeypatch):
    """Three seeded steps (shuffled batches, edge-weight dropout 0.8 from the config) run twice: identical bits for the losses, every
    captured gradient and every variable afterwards."""
    rec = _Recorder(pkg, monkeypatch)
    runs = [_seeded_steps(pkg, oracle, cuda, molecules, 3, "native", {"hidden_size": 100}) for _ in range(2)]
    assert _native_calls(rec) == (6, 6) and rec.backwards == 0
    assert len(runs[0][1]) == 3
    _assert_same_bits(*runs)


FALLBACKS = {"hidden_size_128": ({"hidden_size": 128, "layer_timesteps": [2, 1], "residual_connections": {"1": [0]}}, {}),
             "hidden_size_84": ({"hidden_size": 84, "layer_timesteps": [2, 1], "residual_connections": {"1": [0]}}, {}),
             "use_edge_bias": ({"hidden_size": 32, "use_edge_bias": True}, {}),
             "graph_state_dropout": ({"hidden_size": 32, "graph_state_dropout_keep_prob": 0.8}, {}),
             "freeze_graph_model": ({"hidden_size": 32}, {"--freeze-graph-model": True}),
             "kernel_timing": ({"hidden_size": 32}, {})}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_steps_the_native_route_cannot_take_fall_back(pkg, oracle, cuda, molecules, monkeypatch, case):
    """With the key 'native' but a hidden size outside 32 / 64 / 100 (128: column-panel kernels; 84: padded to 100), an edge bias,
    graph-state dropout, frozen graph variables or per-launch timing active, a seeded step equals the step of the key-True model bit
    for bit and issues no native call."""
    config, args = FALLBACKS[case]
    timing = case == "kernel_timing"
    rec = _Recorder(pkg, monkeypatch)
    native = _seeded_steps(pkg, oracle, cuda, molecules, 1, "native", config, timing, **args)
    assert _native_calls(rec) == (0, 0) and rec.names and rec.backwards >= 1
    _assert_same_bits(native, _seeded_steps(pkg, oracle, cuda, molecules, 1, True, config, timing, **args))


def test_training_follows_reference_run_on_the_native_step(pkg, cuda, tmp_path, monkeypatch):
    """test_gpu_attention_route.test_training_follows_reference_run under the key 'native', its tolerance copied; the key goes into
    the model's config and into the checkpoint's params."""
    g = RG.Golden("sparse_attention")
    g.params = dict(g.params, **{KEY: "native"})
    path = g.write_checkpoint(str(tmp_path / "sparse_attention.pickle"))
    m = pkg.SparseGGNNChemModel(g.model_args(str(cuda), **{"--restore": path}))
    assert m.attention_route() and pkg.train_native.attn_model_eligible(m)
    for n, t in m.named_variables().items():
        np.testing.assert_array_equal(t.detach().cpu().numpy().reshape(g.weights[n].shape), g.weights[n])
    assert len(g.train_losses) == 2
    batches = list(m.make_minibatch_iterator(m.train_data, False))    # unshuffled, keep-probs 1: as recorded
    assert len(batches) == int(g.z["num_train_batches"])
    rec = _Recorder(pkg, monkeypatch)
    losses = [float(m.train_batch(batches[s % len(batches)])) for s in range(len(g.train_losses))]
    assert _native_calls(rec) == (2, 2) and rec.backwards == 0
    np.testing.assert_allclose(losses, g.train_losses, rtol=5e-4)
