"""params['compact_attention']: propagation attention (chem_tensorflow_sparse.py:147-149, 170-196) on the compacted route --
ggnn_sparse_propagate_attn_f32 for inference, compacted transform + ggnn_gather_segment_sum_attn_compact_f32 + packed GRU per
timestep elsewhere, variants.CompactAttentionStepFn in training.

(a) forward against the fp64 oracle through both the one-call and the per-timestep route, (b) the route is really taken (no
dense transform, none of the dense-row attention kernels), (c) everything outside SparseGGNNChemModel.attention_route() is bit
for bit the key-off model, (d) training gradients against torch autograd of the restated timestep and against the key-off
route, (e) the run recorded from the reference's own source (tests/golden/reference_sparse_attention.npz).
"""
from importlib import import_module

import numpy as np
import pytest
import torch

import reference_golden as RG
import train_reference
import variant_oracle

pytestmark = pytest.mark.gpu

MODEL_TOL = dict(atol=1e-5, rtol=1e-4)          # tests/test_gpu_parity.py
STATE_TOL = dict(rtol=1e-4, atol=1e-5)          # tests/test_gpu_reference_golden.py
ATTENTION = {"use_propagation_attention": True}
SMALL = dict(ATTENTION, layer_timesteps=[2, 1], residual_connections={"1": [0]})
OLD_OPS = ("msg_transform", "gather_segment_sum_attn", "attn_backward_target")
NEW_OPS = ("msg_transform_compact_packed", "gather_segment_sum_attn_compact", "attn_backward_target_compact", "sparse_propagate")


def _model(pkg, oracle, ms, config, key, seed=0, device="cuda:0"):
    cfg = dict(config)
    if key:
        cfg["compact_attention"] = True
    model = pkg.SparseGGNNChemModel({"--quiet": True, "--device": device, "train_data": ms, "valid_data": ms, "--config": cfg})
    layers = oracle.make_sparse_layers(np.random.default_rng(seed), model.params, model.num_edge_types, random_bias=True)
    model.set_graph_weights(layers)
    return model, layers


def _feed(model):
    return dict(next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False))))


def _oracle_states(oracle, feed, layers, params):
    adj = [a.cpu().numpy() for a in feed["adjacency_lists"]]
    return oracle.sparse_propagate(feed["initial_node_representation"].cpu().numpy()[:, :params["hidden_size"]], adj,
                                   feed["num_incoming_edges_per_type"].cpu().numpy(), layers, params)


def _count(pkg, monkeypatch, names):
    """Wrap pkg.ops.<name> with call counters -> {name: [count]}; sparse_propagate counts only its attention form."""
    counts = {}
    for name in names:
        counts[name] = [0]

        def wrapper(*a, _orig=getattr(pkg.ops, name), _c=counts[name], _name=name, **k):
            if _name != "sparse_propagate" or k.get("attn") is not None:
                _c[0] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(pkg.ops, name, wrapper)
    return counts


# ---- (a) forward against the fp64 oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [
    dict(ATTENTION),
    dict(ATTENTION, use_edge_bias=True, use_edge_msg_avg_aggregation=False, hidden_size=64),
    dict(ATTENTION, hidden_size=128, layer_timesteps=[2, 1], residual_connections={"1": [0]}),
    dict(ATTENTION, hidden_size=84),                       # runs zero-padded at width 100
], ids=["attention", "attention-bias-sum-h64", "attention-h128-residual", "attention-h84"])
def test_forward_matches_oracle_on_both_routes(pkg, oracle, cuda, config, monkeypatch):
    ms = pkg.synthetic_qm9(120, mean_nodes=14, seed=1)
    model, layers = _model(pkg, oracle, ms, config, key=True)
    assert model.attention_route()
    feed = _feed(model)
    want = _oracle_states(oracle, feed, layers, model.params)
    counts = _count(pkg, monkeypatch, OLD_OPS + NEW_OPS)
    steps = sum(model.params["layer_timesteps"])
    with torch.no_grad():
        model.feed(feed)
        one_call = model.compute_final_node_representations().cpu().numpy()
        assert counts["sparse_propagate"][0] == 1 and counts["gather_segment_sum_attn_compact"][0] == 0
        with pkg.ops.kernel_timing():                      # per-launch timing: the per-timestep form of the same route
            per_step = model.compute_final_node_representations().cpu().numpy()
        assert counts["sparse_propagate"][0] == 1 and counts["gather_segment_sum_attn_compact"][0] == steps
    assert all(counts[n][0] == 0 for n in OLD_OPS)
    np.testing.assert_allclose(one_call, want, err_msg="one-call route", **MODEL_TOL)
    np.testing.assert_allclose(per_step, want, err_msg="per-timestep route", **MODEL_TOL)


# ---- (b) the route is really taken ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [True, False])
def test_route_launches(pkg, oracle, cuda, key, monkeypatch):
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=2)
    model, _ = _model(pkg, oracle, ms, SMALL, key)
    assert model.attention_route() == key
    feed = _feed(model)
    steps = sum(model.params["layer_timesteps"])
    counts = _count(pkg, monkeypatch, OLD_OPS + NEW_OPS)
    with torch.no_grad():
        model.forward_batch(feed)
    if key:
        assert all(counts[n][0] == 0 for n in OLD_OPS), counts
        assert counts["sparse_propagate"][0] == 1
    else:
        assert [counts[n][0] for n in OLD_OPS] == [steps, steps, 0], counts
        assert all(counts[n][0] == 0 for n in NEW_OPS), counts
    for c in counts.values():
        c[0] = 0
    assert np.isfinite(float(model.train_batch(feed)))
    if key:
        assert all(counts[n][0] == 0 for n in OLD_OPS), counts
        assert counts["gather_segment_sum_attn_compact"][0] == steps and counts["attn_backward_target_compact"][0] == steps
        assert counts["msg_transform_compact_packed"][0] >= 2 * steps          # forward, recomputed in the backward (+ dHc W^T)
    else:
        assert [counts[n][0] for n in OLD_OPS] == [2 * steps, steps, steps], counts
        assert all(counts[n][0] == 0 for n in NEW_OPS if n != "msg_transform_compact_packed"), counts


# ---- (c) fall-backs: bit-identical to the model without the key -------------------------------------------------------------------
@pytest.mark.parametrize("config", [
    dict(SMALL, hidden_size=96),                           # keeps its width, has no compacted transform kernel
    dict(SMALL, graph_rnn_cell="RNN"),
], ids=["attention-h96", "attention-rnn"])
def test_fallbacks_are_bit_identical(pkg, oracle, cuda, config):
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=3)
    results = []
    for key in (True, False):
        model, _ = _model(pkg, oracle, ms, config, key)
        assert not model.attention_route()
        feed = _feed(model)
        with torch.no_grad():
            model.feed(feed)
            states = model.compute_final_node_representations().clone()
        with train_reference.capture_step_gradients(model) as grads:
            loss = float(model.train_batch(feed))
        torch.cuda.synchronize()
        results.append((states, loss, grads[0]))
    (s1, l1, g1), (s0, l0, g0) = results
    assert torch.equal(s1, s0) and l1 == l0 and set(g1) == set(g0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


# ---- (d) training ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [
    dict(ATTENTION),
    dict(ATTENTION, use_edge_bias=True, use_edge_msg_avg_aggregation=False, hidden_size=64),
    dict(ATTENTION, hidden_size=128, layer_timesteps=[2, 1], residual_connections={"1": [0]}),
    dict(SMALL, hidden_size=84),                           # zero-padded width: the gradients are sliced back to the variables
], ids=["attention", "attention-bias-sum-h64", "attention-h128-residual", "attention-h84"])
def test_backward_equals_autograd_of_torch_restatement(pkg, oracle, cuda, config, monkeypatch):
    """The bounds of test_gpu_train.test_variant_hip_backward_equals_autograd_of_torch_restatement, every variable."""
    variants = import_module(pkg.__name__ + ".variants")
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=4)
    grads = {}
    for mode in (False, True):
        monkeypatch.setattr(variants, "BACKWARD_ORACLE", variant_oracle.autograd_backward if mode else None)
        model, _ = _model(pkg, oracle, ms, dict(config, edge_weight_dropout_keep_prob=1.0), key=True, seed=4)
        assert model.attention_route()
        feed = _feed(model)
        variables = model.trainable_variables
        for v in variables.values():
            v.requires_grad_(True); v.grad = None
        model.training = True
        loss = model.forward_batch(feed)
        loss.backward()
        model.training = False
        grads[mode] = {k: v.grad.detach().double().cpu() for k, v in variables.items()}
        grads[(mode, "loss")] = float(loss.detach())
    assert any("edge_type_attention_weights" in k for k in grads[True])
    assert abs(grads[(False, "loss")] - grads[(True, "loss")]) <= 1e-6 * max(1.0, abs(grads[(True, "loss")]))
    for name, want in grads[True].items():
        got = grads[False][name]
        scale = float(want.abs().max()) + 1e-12
        err = float((got - want).abs().max())
        print("%s: err %.3e scale %.3e" % (name, err, scale))
        assert err <= 3e-4 * scale + 1e-7, (name, err, scale)


def test_three_training_steps_follow_the_key_off_route(pkg, oracle, cuda):
    ms = pkg.synthetic_qm9(100, mean_nodes=10, seed=5)
    results = []
    for key in (True, False):
        model, _ = _model(pkg, oracle, ms, dict(ATTENTION, edge_weight_dropout_keep_prob=0.8), key, seed=5)
        assert model.attention_route() == key
        feed = _feed(model)
        feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"] = 0.8, 1.0
        with train_reference.capture_step_gradients(model) as grads:
            losses = [float(model.train_batch(feed)) for _ in range(3)]
        torch.cuda.synchronize()
        assert len(grads) == 3
        results.append((losses, grads[0]))
    (l1, g1), (l0, g0) = results
    print("losses key on %s, key off %s" % (l1, l0))
    np.testing.assert_allclose(l1, l0, rtol=1e-5)
    train_reference.assert_gradients_match(g1, g0)


# ---- (e) the recorded reference run -----------------------------------------------------------------------------------------------
def _golden_model(pkg, tmp_path, cuda):
    g = RG.Golden("sparse_attention")
    g.params = dict(g.params, compact_attention=True)      # in the model's config and in the checkpoint's params
    path = g.write_checkpoint(str(tmp_path / "sparse_attention.pickle"))
    m = pkg.SparseGGNNChemModel(g.model_args(str(cuda), **{"--restore": path}))
    assert m.attention_route()
    for n, t in m.named_variables().items():
        np.testing.assert_array_equal(t.detach().cpu().numpy().reshape(g.weights[n].shape), g.weights[n])
    return g, m


def test_forward_matches_reference_run(pkg, cuda, tmp_path):
    g, m = _golden_model(pkg, tmp_path, cuda)
    batches = list(m.make_minibatch_iterator(m.valid_data, False))
    assert len(batches) == g.num_valid_batches
    for k, b in enumerate(batches):
        with torch.no_grad():
            loss = m.forward_batch(b)
        pre = "valid%d" % k
        h = m.ops["final_node_representations"].detach().cpu().numpy()
        np.testing.assert_allclose(h, g.result(pre, "final_node_representations"), **STATE_TOL)
        np.testing.assert_allclose(m.output.detach().cpu().numpy().reshape(-1), g.result(pre, "output"), rtol=2e-4, atol=5e-5)
        np.testing.assert_allclose(float(loss), g.result(pre, "loss"), rtol=5e-4)
        np.testing.assert_allclose(float(m.ops["accuracy_task0"]), g.result(pre, "accuracy"), rtol=5e-4)


def test_training_follows_reference_run(pkg, cuda, tmp_path):
    g, m = _golden_model(pkg, tmp_path, cuda)
    assert len(g.train_losses) == 2
    batches = list(m.make_minibatch_iterator(m.train_data, False))    # unshuffled, keep-probs 1: as recorded
    assert len(batches) == int(g.z["num_train_batches"])
    losses = [float(m.train_batch(batches[s % len(batches)])) for s in range(len(g.train_losses))]
    np.testing.assert_allclose(losses, g.train_losses, rtol=5e-4)
