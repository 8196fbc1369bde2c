"""params['compact_cudnn_gru']: the CudnnCompatibleGRUCell of the sparse GGNN (graph_rnn_cell = CudnnCompatibleGRUCell) on the
compacted route -- ggnn_sparse_propagate_cudnn_f32 for inference; compacted transform, segment sum over the compact rows and
ggnn_cudnn_gru_packed_f32 (or the composed ggnn_cudnn_gru_train_f32) per timestep elsewhere; variants.CompactCudnnStepFn in training.

(a) forward against the fp64 oracle through both the one-call and the per-timestep route, (b) the route is really taken (no dense
transform, no composed cell where every layer is fused), (c) everything outside SparseGGNNChemModel.cudnn_route() is bit for bit the
key-off model, (d) training gradients against the key-off route and against torch autograd of the restated timestep, (e) the run
recorded from the reference's own source (tests/golden/reference_sparse_cudnn_gru.npz).
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
CUDNN = {"graph_rnn_cell": "CudnnCompatibleGRUCell"}
BIAS_SUM_64 = dict(CUDNN, use_edge_bias=True, use_edge_msg_avg_aggregation=False, hidden_size=64)
BIAS_64 = dict(CUDNN, use_edge_bias=True, hidden_size=64)
H128 = dict(CUDNN, hidden_size=128, layer_timesteps=[2, 1], residual_connections={"1": [0]})
SMALL = dict(CUDNN, layer_timesteps=[2, 1], residual_connections={"1": [0]})
OLD_OPS = ("msg_transform", "gather_segment_sum", "cudnn_gru", "cudnn_gru_train")
NEW_OPS = ("msg_transform_compact_packed", "gather_segment_sum_compact", "cudnn_gru_packed", "sparse_propagate")


def _model(pkg, oracle, ms, config, key, seed=0, device="cuda:0", key_name="compact_cudnn_gru"):
    cfg = dict(config)
    if key:
        cfg[key_name] = True
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
    """Wrap pkg.ops.<name> with call counters -> {name: [count]}; sparse_propagate counts only its Cudnn form."""
    counts = {}
    for name in names:
        counts[name] = [0]

        def wrapper(*a, _orig=getattr(pkg.ops, name), _c=counts[name], _name=name, **k):
            if _name != "sparse_propagate" or k.get("cudnn") is not None:
                _c[0] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(pkg.ops, name, wrapper)
    return counts


def _fused_steps(pkg, model):
    """Timesteps of the model whose layer the fused cell takes (a supported (width, nx))."""
    p = model.params
    return sum(int(t) for l, t in enumerate(p["layer_timesteps"])
               if pkg.ops.cudnn_gru_fused_supported(model._kw, len(p["residual_connections"].get(str(l)) or ()) + 1))


# ---- (a) forward against the fp64 oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,all_fused", [
    (dict(CUDNN), True),                                    # default layers at hidden 100: nx = 1, 2, 3
    (dict(CUDNN, hidden_size=64), True),
    (dict(CUDNN, hidden_size=32, tie_fwd_bkwd=False), True),
    (BIAS_SUM_64, True),                                    # edge bias + sum aggregation: fused like any other layer
    (dict(CUDNN, hidden_size=84), True),                    # runs zero-padded at width 100
    (H128, False),                                          # compacted transform, composed cell
], ids=["default-h100", "default-h64", "default-h32-untied", "bias-sum-h64", "default-h84", "h128-residual"])
def test_forward_matches_oracle_on_both_routes(pkg, oracle, cuda, config, all_fused, monkeypatch):
    ms = pkg.synthetic_qm9(120, mean_nodes=14, seed=1)
    model, layers = _model(pkg, oracle, ms, config, key=True)
    assert model.cudnn_route()
    feed = _feed(model)
    want = _oracle_states(oracle, feed, layers, model.params)
    assert np.count_nonzero(want == 0.0) < 0.75 * want.size, "a comparison of zeros with zeros would pass"
    counts = _count(pkg, monkeypatch, OLD_OPS + NEW_OPS)
    steps = sum(model.params["layer_timesteps"])
    n_fused = _fused_steps(pkg, model)
    assert n_fused == (steps if all_fused else 0)
    if all_fused:
        assert {len(model.params["residual_connections"].get(str(l)) or ()) + 1
                for l in range(len(model.params["layer_timesteps"]))} == {1, 2, 3}
    with torch.no_grad():
        model.feed(feed)
        one_call = model.compute_final_node_representations().cpu().numpy()
        assert counts["sparse_propagate"][0] == 1 and counts["msg_transform_compact_packed"][0] == 0
        with pkg.ops.kernel_timing():                      # per-launch timing: the per-timestep form of the same route
            per_step = model.compute_final_node_representations().cpu().numpy()
        assert counts["sparse_propagate"][0] == 1
        assert counts["msg_transform_compact_packed"][0] == counts["gather_segment_sum_compact"][0] == steps
        assert counts["cudnn_gru_packed"][0] == n_fused
        assert counts["cudnn_gru_train"][0] + counts["cudnn_gru"][0] == steps - n_fused
    assert counts["msg_transform"][0] == 0 and counts["gather_segment_sum"][0] == 0
    assert model.last_gru_formats == [pkg.formats.BF16X3] * len(model.params["layer_timesteps"])
    np.testing.assert_allclose(one_call, want, err_msg="one-call route", **MODEL_TOL)
    np.testing.assert_allclose(per_step, want, err_msg="per-timestep route", **MODEL_TOL)


# ---- (b) the route is really taken ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [True, False])
def test_route_launches(pkg, oracle, cuda, key, monkeypatch):
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=2)
    model, _ = _model(pkg, oracle, ms, dict(SMALL, hidden_size=64), key)
    assert model.cudnn_route() == key
    feed = _feed(model)
    steps = sum(model.params["layer_timesteps"])
    counts = _count(pkg, monkeypatch, OLD_OPS + NEW_OPS)
    with torch.no_grad():
        model.forward_batch(feed)
    if key:
        assert all(counts[n][0] == 0 for n in OLD_OPS), counts
        assert counts["sparse_propagate"][0] == 1 and counts["cudnn_gru_packed"][0] == 0
    else:
        assert [counts[n][0] for n in OLD_OPS] == [steps, steps, steps, 0], counts
        assert all(counts[n][0] == 0 for n in NEW_OPS), counts
    for c in counts.values():
        c[0] = 0
    assert np.isfinite(float(model.train_batch(feed)))
    if key:
        assert all(counts[n][0] == 0 for n in OLD_OPS), counts
        assert counts["cudnn_gru_packed"][0] == steps and counts["gather_segment_sum_compact"][0] == steps
        assert counts["msg_transform_compact_packed"][0] >= steps           # forward (+ dHc W^T in the backward)
        assert counts["sparse_propagate"][0] == 0
    else:
        assert [counts[n][0] for n in OLD_OPS] == [steps, steps, 0, steps], counts
        assert all(counts[n][0] == 0 for n in NEW_OPS if n != "msg_transform_compact_packed"), counts


# ---- (c) fall-backs: bit-identical to the model without the key -------------------------------------------------------------------
@pytest.mark.parametrize("config", [
    dict(layer_timesteps=[2, 1], residual_connections={"1": [0]}),                      # the key on the default GRU
    dict(layer_timesteps=[2, 1], residual_connections={"1": [0]}, graph_rnn_cell="RNN"),   # the key on the RNN cell
    dict(SMALL, use_propagation_attention=True),                                        # the key with attention + Cudnn cell
], ids=["gru", "rnn", "attention-cudnn"])
def test_fallbacks_are_bit_identical(pkg, oracle, cuda, config):
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=3)
    results = []
    for key in (True, False):
        model, _ = _model(pkg, oracle, ms, config, key)
        assert not model.cudnn_route()
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
TRAIN_CONFIGS = [(dict(CUDNN), 0.8), (BIAS_64, 1.0)]
TRAIN_IDS = ["default-h100-dropout", "bias-h64"]


@pytest.mark.parametrize("config,ew_keep", TRAIN_CONFIGS, ids=TRAIN_IDS)
def test_backward_equals_autograd_of_torch_restatement(pkg, oracle, cuda, config, ew_keep, monkeypatch):
    """The bounds of tests/test_gpu_rnn_route.py's twin, every variable.  Both backward passes start from the same HIP forward;
    sigmoid and tanh have no kink, so any weight seed serves."""
    variants = import_module(pkg.__name__ + ".variants")
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=4)

    def run(mode):
        monkeypatch.setattr(variants, "BACKWARD_ORACLE", variant_oracle.autograd_backward if mode else None)
        model, _ = _model(pkg, oracle, ms, dict(config, edge_weight_dropout_keep_prob=ew_keep), key=True, seed=4)
        assert model.cudnn_route()
        feed = _feed(model)
        feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"] = ew_keep, 1.0
        variables = model.trainable_variables
        for v in variables.values():
            v.requires_grad_(True); v.grad = None
        model.training = True
        loss = model.forward_batch(feed)
        loss.backward()
        model.training = False
        return {k: v.grad.detach().double().cpu() for k, v in variables.items()}, float(loss.detach())

    got_all, loss_hip = run(False)
    want_all, loss_auto = run(True)
    assert any("cudnn" in k.lower() or "gru" in k.lower() for k in want_all)
    assert abs(loss_hip - loss_auto) <= 1e-6 * max(1.0, abs(loss_auto))
    for name, want in want_all.items():
        got = got_all[name]
        scale = float(want.abs().max()) + 1e-12
        err = float((got - want).abs().max())
        print("%s: err %.3e scale %.3e" % (name, err, scale))
        assert err <= 3e-4 * scale + 1e-7, (name, err, scale)


@pytest.mark.parametrize("config,ew_keep", TRAIN_CONFIGS, ids=TRAIN_IDS)
def test_training_step_follows_the_key_off_route(pkg, oracle, cuda, config, ew_keep):
    ms = pkg.synthetic_qm9(100, mean_nodes=10, seed=5)
    results = []
    for key in (True, False):
        model, _ = _model(pkg, oracle, ms, dict(config, edge_weight_dropout_keep_prob=ew_keep), key, seed=5)
        assert model.cudnn_route() == key
        feed = _feed(model)
        feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"] = ew_keep, 1.0
        with train_reference.capture_step_gradients(model) as grads:
            losses = [float(model.train_batch(feed)) for _ in range(2)]
        torch.cuda.synchronize()
        assert len(grads) == 2
        assert all(np.isfinite(l) for l in losses)
        for n, t in model.named_variables().items():
            assert bool(torch.isfinite(t).all()), n
        results.append((losses, grads[0]))
    (l1, g1), (l0, g0) = results
    print("losses key on %s, key off %s" % (l1, l0))
    np.testing.assert_allclose(l1, l0, rtol=1e-5)
    train_reference.assert_gradients_match(g1, g0)


# ---- (e) the recorded reference run -----------------------------------------------------------------------------------------------
def _golden_model(pkg, tmp_path, cuda):
    g = RG.Golden("sparse_cudnn_gru")
    g.params = dict(g.params, compact_cudnn_gru=True)      # in the model's config and in the checkpoint's params
    path = g.write_checkpoint(str(tmp_path / "sparse_cudnn_gru.pickle"))
    m = pkg.SparseGGNNChemModel(g.model_args(str(cuda), **{"--restore": path}))
    assert m.cudnn_route()
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
    """The Adam step as tests/test_gpu_reference_golden.py checks it for the key-off model."""
    g, m = _golden_model(pkg, tmp_path, cuda)
    assert len(g.train_losses) > 0
    batches = list(m.make_minibatch_iterator(m.train_data, False))    # unshuffled, keep-probs 1: as recorded
    assert len(batches) == int(g.z["num_train_batches"])
    losses = [float(m.train_batch(batches[s % len(batches)])) for s in range(len(g.train_losses))]
    np.testing.assert_allclose(losses, g.train_losses, rtol=5e-4)
    nv = m.named_variables()
    for i, n in enumerate(g.names):
        a = nv[n].detach().cpu().numpy()
        np.testing.assert_allclose(RG.stats(a), g.z["trained_stats"][i], rtol=1e-3, atol=5e-3, err_msg=n)
        if "trained/" + n in g.z.files:
            np.testing.assert_allclose(a.reshape(g.z["trained/" + n].shape), g.z["trained/" + n], rtol=1e-2, atol=3e-3, err_msg=n)
