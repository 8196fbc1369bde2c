"""params['compact_rnn']: the BasicRNNCell of the sparse GGNN (graph_rnn_cell = RNN, the reference README's R-GCN command) on the
compacted route -- ggnn_sparse_propagate_rnn_f32 for inference, compacted transform + ggnn_rnn_packed_gather_f32 (or the segment sum
over the compact rows + ggnn_rnn_f32) per timestep elsewhere, variants.CompactRnnStepFn in training.

(a) forward against the fp64 oracle through both the one-call and the per-timestep route, (b) the route is really taken (no dense
transform), (c) everything outside SparseGGNNChemModel.rnn_route() is bit for bit the key-off model, (d) training gradients against
torch autograd of the restated timestep and against the key-off route, (e) the run recorded from the reference's own source
(tests/golden/reference_sparse_relu_rnn.npz).
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
README = {"use_edge_bias": False, "use_edge_msg_avg_aggregation": True, "residual_connections": {},
          "layer_timesteps": [1, 1, 1, 1, 1, 1, 1, 1], "graph_rnn_cell": "RNN", "graph_rnn_activation": "ReLU"}
RNN = {"graph_rnn_cell": "RNN"}
BIAS_SUM_64 = dict(RNN, graph_rnn_activation="ReLU", use_edge_bias=True, use_edge_msg_avg_aggregation=False, hidden_size=64)
H128 = dict(RNN, hidden_size=128, layer_timesteps=[2, 1], residual_connections={"1": [0]})
SMALL = dict(RNN, layer_timesteps=[2, 1], residual_connections={"1": [0]})
OLD_OPS = ("msg_transform", "gather_segment_sum", "rnn")
NEW_OPS = ("msg_transform_compact_packed", "rnn_packed_gather", "gather_segment_sum_compact", "sparse_propagate")


def _model(pkg, oracle, ms, config, key, seed=0, device="cuda:0"):
    cfg = dict(config)
    if key:
        cfg["compact_rnn"] = True
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
    """Wrap pkg.ops.<name> with call counters -> {name: [count]}; sparse_propagate counts only its RNN form."""
    counts = {}
    for name in names:
        counts[name] = [0]

        def wrapper(*a, _orig=getattr(pkg.ops, name), _c=counts[name], _name=name, **k):
            if _name != "sparse_propagate" or k.get("rnn") is not None:
                _c[0] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(pkg.ops, name, wrapper)
    return counts


def _fused_steps(pkg, model):
    """Timesteps of the model whose layer the gather-fused cell takes (supported (width, nx), no edge bias)."""
    p = model.params
    if p["use_edge_bias"]:
        return 0
    return sum(int(t) for l, t in enumerate(p["layer_timesteps"])
               if pkg.ops.rnn_fused_supported(model._kw, len(p["residual_connections"].get(str(l)) or ()) + 1))


# ---- (a) forward against the fp64 oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,fused", [
    (dict(README), 8),
    (dict(README, hidden_size=64), 8),
    (dict(README, hidden_size=32, tie_fwd_bkwd=False), 8),
    (dict(RNN), None),                                      # default layers: residual layers with nx = 2, 3 (composed at width 100)
    (dict(RNN, hidden_size=64), None),                      # ... fused at width 64: nx = 1, 2, 3 through the model
    (BIAS_SUM_64, 0),                                       # edge bias: composed layers
    (H128, 0),                                              # compacted transform, composed cell
    (dict(README, hidden_size=84), 8),                      # runs zero-padded at width 100
], ids=["readme-h100", "readme-h64", "readme-h32-untied", "rnn-default-layers", "rnn-default-layers-h64", "relu-bias-sum-h64",
        "rnn-h128-residual", "readme-h84"])
def test_forward_matches_oracle_on_both_routes(pkg, oracle, cuda, config, fused, monkeypatch):
    ms = pkg.synthetic_qm9(120, mean_nodes=14, seed=1)
    model, layers = _model(pkg, oracle, ms, config, key=True)
    assert model.rnn_route()
    feed = _feed(model)
    want = _oracle_states(oracle, feed, layers, model.params)
    assert np.count_nonzero(want == 0.0) < 0.75 * want.size, "a comparison of zeros with zeros would pass"
    counts = _count(pkg, monkeypatch, OLD_OPS + NEW_OPS)
    steps = sum(model.params["layer_timesteps"])
    n_fused = _fused_steps(pkg, model)
    if fused is not None:
        assert n_fused == fused
    else:
        assert 0 < n_fused
    with torch.no_grad():
        model.feed(feed)
        one_call = model.compute_final_node_representations().cpu().numpy()
        assert counts["sparse_propagate"][0] == 1 and counts["msg_transform_compact_packed"][0] == 0
        with pkg.ops.kernel_timing():                      # per-launch timing: the per-timestep form of the same route
            per_step = model.compute_final_node_representations().cpu().numpy()
        assert counts["sparse_propagate"][0] == 1 and counts["msg_transform_compact_packed"][0] == steps
        assert counts["rnn_packed_gather"][0] == n_fused
        assert counts["gather_segment_sum_compact"][0] == counts["rnn"][0] == steps - n_fused
    assert counts["msg_transform"][0] == 0 and counts["gather_segment_sum"][0] == 0
    assert model.last_gru_formats == [pkg.formats.BF16X3] * len(model.params["layer_timesteps"])
    np.testing.assert_allclose(one_call, want, err_msg="one-call route", **MODEL_TOL)
    np.testing.assert_allclose(per_step, want, err_msg="per-timestep route", **MODEL_TOL)


# ---- (b) the route is really taken ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [True, False])
def test_route_launches(pkg, oracle, cuda, key, monkeypatch):
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=2)
    model, _ = _model(pkg, oracle, ms, dict(README, hidden_size=64, layer_timesteps=[2, 1]), key)
    assert model.rnn_route() == key
    feed = _feed(model)
    steps = sum(model.params["layer_timesteps"])
    counts = _count(pkg, monkeypatch, OLD_OPS + NEW_OPS)
    with torch.no_grad():
        model.forward_batch(feed)
    if key:
        assert all(counts[n][0] == 0 for n in OLD_OPS), counts
        assert counts["sparse_propagate"][0] == 1 and counts["rnn_packed_gather"][0] == 0
    else:
        assert [counts[n][0] for n in OLD_OPS] == [steps, steps, steps], counts
        assert all(counts[n][0] == 0 for n in NEW_OPS), counts
    for c in counts.values():
        c[0] = 0
    assert np.isfinite(float(model.train_batch(feed)))
    if key:
        assert all(counts[n][0] == 0 for n in OLD_OPS), counts
        assert counts["rnn_packed_gather"][0] == steps and counts["gather_segment_sum_compact"][0] == 0
        assert counts["msg_transform_compact_packed"][0] >= steps           # forward (+ dHc W^T in the backward)
        assert counts["sparse_propagate"][0] == 0
    else:
        assert [counts[n][0] for n in OLD_OPS] == [steps, steps, steps], counts
        assert all(counts[n][0] == 0 for n in NEW_OPS if n != "msg_transform_compact_packed"), counts


# ---- (c) fall-backs: bit-identical to the model without the key -------------------------------------------------------------------
@pytest.mark.parametrize("config", [
    dict(layer_timesteps=[2, 1], residual_connections={"1": [0]}),                      # the default GRU
    dict(SMALL, use_propagation_attention=True),                                        # attention + RNN
    dict(layer_timesteps=[2, 1], residual_connections={"1": [0]}, graph_rnn_cell="CudnnCompatibleGRUCell"),
    dict(SMALL, hidden_size=96),                                                        # keeps its width, no compacted transform
], ids=["gru", "attention-rnn", "cudnn-gru", "rnn-h96"])
def test_fallbacks_are_bit_identical(pkg, oracle, cuda, config):
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=3)
    results = []
    for key in (True, False):
        model, _ = _model(pkg, oracle, ms, config, key)
        assert not model.rnn_route()
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
def _kink_recorder(variants, monkeypatch, ratios):
    """Wrap variants.compact_rnn_forward: per timestep, the smallest |pre-activation| / (its float32 rounding bound) over the
    elements of [x | incoming | h] W + b, evaluated in float64 on the step's own float32 inputs.  The bound is the project's product
    bound per element without its absolute floor, 4e-7 (|A| @ |W|) (variant_kernel_ref.gemm_atol), plus eps |b|.  Elements that are
    exactly 0 with a zero bound (zero-padded columns: 0 in any summation order) are left out."""
    orig = variants.compact_rnn_forward
    if hasattr(orig, "_kink_orig"):
        orig = orig._kink_orig

    def wrapper(h, index, nin, edge_weights, edge_biases, use_avg, residual_states, W, b, activation):
        out, incoming = orig(h, index, nin, edge_weights, edge_biases, use_avg, residual_states, W, b, activation)
        A = torch.cat(list(residual_states) + [incoming, h], dim=1).detach().double()
        W64, b64 = W.detach().double(), b.detach().double()
        pre = (A @ W64 + b64).abs()
        bound = 4e-7 * (A.abs() @ W64.abs()) + 2.0 ** -24 * b64.abs()
        live = bound > 0
        ratios.append(float((pre[live] / bound[live]).min()) if bool(live.any()) else float("inf"))
        return out, incoming
    wrapper._kink_orig = orig
    monkeypatch.setattr(variants, "compact_rnn_forward", wrapper)


@pytest.mark.parametrize("config", [
    dict(README),
    BIAS_SUM_64,
    H128,
    dict(README, hidden_size=84),                           # zero-padded width: the gradients are sliced back to the variables
], ids=["readme-h100", "relu-bias-sum-h64", "rnn-h128-residual", "readme-h84"])
def test_backward_equals_autograd_of_torch_restatement(pkg, oracle, cuda, config, monkeypatch):
    """The bounds of tests/test_gpu_attention_route.py's twin, every variable.

    Both backward passes start from the same HIP forward.  The hand-written one gates ReLU by the sign of the kernel's float32
    output, autograd by the sign of torch's own float32 pre-activation: where a pre-activation lies within float32 rounding of 0
    the two may disagree, and the derivative there is not a property of the inputs (measured with weight seed 4 at hidden 84: one
    such element in layer 2, |pre| < 1e-6, moved the gradients of layers 0 .. 2 by up to 6e-4 of their scale while layers 3 .. 7
    agreed to 1e-6; the key-off route and seeds 5, 6 agreed to 4e-6 everywhere).  So for ReLU the weights are drawn with the first
    seed from 4 on for which every pre-activation of the run stays beyond KINK_FACTOR x its a-priori float32 rounding bound
    (_kink_recorder; the factor 2 of tests/test_gpu_variant_kernels.py).  The criterion reads the forward's inputs and float64
    arithmetic only, never a gradient."""
    variants = import_module(pkg.__name__ + ".variants")
    KINK_FACTOR = 2.0
    relu = str(config.get("graph_rnn_activation", "tanh")).lower() == "relu"
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=4)

    def run(seed, mode):
        monkeypatch.setattr(variants, "BACKWARD_ORACLE", variant_oracle.autograd_backward if mode else None)
        model, _ = _model(pkg, oracle, ms, dict(config, edge_weight_dropout_keep_prob=1.0), key=True, seed=seed)
        assert model.rnn_route()
        feed = _feed(model)
        variables = model.trainable_variables
        for v in variables.values():
            v.requires_grad_(True); v.grad = None
        model.training = True
        loss = model.forward_batch(feed)
        loss.backward()
        model.training = False
        return {k: v.grad.detach().double().cpu() for k, v in variables.items()}, float(loss.detach()), \
            sum(model.params["layer_timesteps"])

    grads = {}
    for seed in range(4, 20):
        ratios = []
        _kink_recorder(variants, monkeypatch, ratios)       # (both runs of a seed are recorded: the forward is the same)
        grads[False], grads[(False, "loss")], steps = run(seed, False)
        assert len(ratios) == steps
        print("weight seed %d: smallest |pre| / rounding bound per timestep %s" % (seed, ["%.3g" % r for r in ratios]))
        if not relu or min(ratios) > KINK_FACTOR:
            break
    else:
        raise AssertionError("no weight seed in 4 .. 19 keeps every ReLU pre-activation off the kink")
    grads[True], grads[(True, "loss")], _ = run(seed, True)
    assert any("basic_rnn_cell" in k for k in grads[True])
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
        model, _ = _model(pkg, oracle, ms, dict(README, edge_weight_dropout_keep_prob=0.8), key, seed=5)
        assert model.rnn_route() == key
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
    g = RG.Golden("sparse_relu_rnn")
    g.params = dict(g.params, compact_rnn=True)            # in the model's config and in the checkpoint's params
    path = g.write_checkpoint(str(tmp_path / "sparse_relu_rnn.pickle"))
    m = pkg.SparseGGNNChemModel(g.model_args(str(cuda), **{"--restore": path}))
    assert m.rnn_route()
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
