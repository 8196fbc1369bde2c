"""params['rnn_panel_cell'] on top of params['compact_rnn']: layers of the R-GCN configuration at kernel width 128 / 192 / 256 run the
column-panel cell (ggnn_rnn_panel_gather_f32) in place of the segment sum over the compact rows + ggnn_rnn_f32 -- inside
ggnn_sparse_propagate_rnn_f32 for inference, per timestep elsewhere, in variants.CompactRnnPanelStepFn's forward in training.

(a) forward against the fp64 oracle through the one-call and the per-timestep route, with the launches counted, (b) everything the
key does not cover is bit for bit compact_rnn = True alone, (c) training: gradients against torch autograd of the restated timestep
and three steps against the key-off route.  The pattern and the bounds are tests/test_gpu_rnn_route.py's.
"""
from importlib import import_module

import numpy as np
import pytest
import torch

import train_reference
import variant_oracle

pytestmark = pytest.mark.gpu

MODEL_TOL = dict(atol=1e-5, rtol=1e-4)          # tests/test_gpu_parity.py
README = {"use_edge_bias": False, "use_edge_msg_avg_aggregation": True, "residual_connections": {},
          "layer_timesteps": [1, 1, 1, 1, 1, 1, 1, 1], "graph_rnn_cell": "RNN", "graph_rnn_activation": "ReLU"}
RNN = {"graph_rnn_cell": "RNN"}
BIAS_SUM_64 = dict(RNN, graph_rnn_activation="ReLU", use_edge_bias=True, use_edge_msg_avg_aggregation=False, hidden_size=64)
H128 = dict(RNN, hidden_size=128, layer_timesteps=[2, 1], residual_connections={"1": [0]})
SMALL = dict(RNN, layer_timesteps=[2, 1], residual_connections={"1": [0]})
OPS = ("msg_transform", "gather_segment_sum", "rnn", "msg_transform_compact_packed", "rnn_packed_gather", "rnn_panel_gather",
       "gather_segment_sum_compact", "sparse_propagate")


def _model(pkg, oracle, ms, config, panel, compact=True, seed=0, device="cuda:0"):
    cfg = dict(config)
    cfg["compact_rnn"] = compact
    if panel:
        cfg["rnn_panel_cell"] = True
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


def _panel_steps(pkg, model):
    """Timesteps of the model whose layer the panel cell takes (supported (width, nx), no edge bias)."""
    p = model.params
    if p["use_edge_bias"]:
        return 0
    return sum(int(t) for l, t in enumerate(p["layer_timesteps"])
               if pkg.ops.rnn_panel_supported(model._kw, len(p["residual_connections"].get(str(l)) or ()) + 1))


# ---- (a) forward against the fp64 oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,width,panel_steps", [
    (H128, 128, 3),
    (dict(README, hidden_size=128), 128, 8),
    (dict(README, hidden_size=192), 192, 8),
    (dict(README, hidden_size=256), 256, 8),
    (dict(README, hidden_size=150), 192, 8),                # runs zero-padded at width 192
    (dict(RNN, hidden_size=128), 128, 8),                   # the default residual layers: nx = 1, 2, 3 through the model
], ids=["rnn-h128-residual", "readme-h128", "readme-h192", "readme-h256", "readme-h150", "rnn-default-layers-h128"])
def test_forward_matches_oracle_on_both_routes(pkg, oracle, cuda, config, width, panel_steps, monkeypatch):
    ms = pkg.synthetic_qm9(120, mean_nodes=14, seed=1)
    model, layers = _model(pkg, oracle, ms, config, panel=True)
    assert model.rnn_route() and model.rnn_panel_route() and model._kw == width
    feed = _feed(model)
    want = _oracle_states(oracle, feed, layers, model.params)
    assert np.count_nonzero(want == 0.0) < 0.75 * want.size, "a comparison of zeros with zeros would pass"
    counts = _count(pkg, monkeypatch, OPS)
    steps = sum(model.params["layer_timesteps"])
    assert _panel_steps(pkg, model) == panel_steps == steps
    seen = []                                               # the packed images the one-call driver is handed, per layer
    orig = pkg.ops.sparse_propagate

    def spy(*a, **k):
        seen.append(k["rnn"][2])
        return orig(*a, **k)
    monkeypatch.setattr(pkg.ops, "sparse_propagate", spy)
    with torch.no_grad():
        model.feed(feed)
        one_call = model.compute_final_node_representations().cpu().numpy()
        assert counts["sparse_propagate"][0] == 1 and counts["msg_transform_compact_packed"][0] == 0
        # every layer goes in with its panel images: the driver then has no composed launch to fall back to silently
        nxs = [len(model.params["residual_connections"].get(str(l)) or ()) + 1 for l in range(len(model.params["layer_timesteps"]))]
        assert len(seen) == 1 and [None if t is None else t.numel() * 4 for t in seen[0]] == \
            [pkg._lib.load().ggnn_rnn_panel_packed_bytes(width, nx) for nx in nxs]
        with pkg.ops.kernel_timing():                      # per-launch timing: the per-timestep form of the same route
            per_step = model.compute_final_node_representations().cpu().numpy()
        assert counts["sparse_propagate"][0] == 1 and counts["msg_transform_compact_packed"][0] == steps
        assert counts["rnn_panel_gather"][0] == panel_steps
        assert counts["gather_segment_sum_compact"][0] == counts["rnn"][0] == counts["rnn_packed_gather"][0] == 0
    assert counts["msg_transform"][0] == 0 and counts["gather_segment_sum"][0] == 0
    np.testing.assert_allclose(one_call, want, err_msg="one-call route", **MODEL_TOL)
    np.testing.assert_allclose(per_step, want, err_msg="per-timestep route", **MODEL_TOL)


def test_one_call_route_launches_the_panel_kernel(pkg, oracle, cuda):
    """The one-call driver's launches are not visible to the ops counters: with the key the states differ from the composed route's
    in the last bits (another product arithmetic), and they are the per-timestep panel route's bit for bit."""
    ms = pkg.synthetic_qm9(120, mean_nodes=14, seed=1)
    states = {}
    for panel in (True, False):
        model, _ = _model(pkg, oracle, ms, dict(README, hidden_size=128), panel=panel)
        feed = _feed(model)
        with torch.no_grad():
            model.feed(feed)
            states[panel] = model.compute_final_node_representations().clone()
            if panel:
                with pkg.ops.kernel_timing():
                    states["steps"] = model.compute_final_node_representations().clone()
    assert torch.equal(states[True], states["steps"])
    assert not torch.equal(states[True], states[False])


# ---- (b) fall-backs: bit-identical to compact_rnn = True alone --------------------------------------------------------------------
@pytest.mark.parametrize("config,compact", [
    (dict(SMALL, hidden_size=64), True),                                                # the resident-image cell's width
    (dict(SMALL), True),                                                                # width 100
    (dict(BIAS_SUM_64, hidden_size=128), True),                                         # edge bias: composed layers
    (dict(H128), "native"),                                                             # not eligible: stays compact_rnn = True
], ids=["h64", "h100", "relu-bias-sum-h128", "native-h128"])
def test_fallbacks_are_bit_identical(pkg, oracle, cuda, config, compact, monkeypatch):
    ms = pkg.synthetic_qm9(80, mean_nodes=10, seed=3)
    results = []
    for panel in (True, False):
        model, _ = _model(pkg, oracle, ms, config, panel=panel, compact=compact if panel else True)
        assert model.rnn_route()
        counts = _count(pkg, monkeypatch, ("rnn_panel_gather",))
        feed = _feed(model)
        with torch.no_grad():
            model.feed(feed)
            states = model.compute_final_node_representations().clone()
        with train_reference.capture_step_gradients(model) as grads:
            loss = float(model.train_batch(feed))
        torch.cuda.synchronize()
        assert counts["rnn_panel_gather"][0] == 0
        results.append((states, loss, grads[0]))
    (s1, l1, g1), (s0, l0, g0) = results
    assert torch.equal(s1, s0) and l1 == l0 and set(g1) == set(g0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


# ---- (c) training ---------------------------------------------------------------------------------------------------------------
def _kink_recorder(variants, monkeypatch, ratios):
    """tests/test_gpu_rnn_route.py's recorder: per timestep, the smallest |pre-activation| / (its float32 rounding bound) over the
    elements of [x | incoming | h] W + b, in float64 on the step's own float32 inputs; the bound is 4e-7 (|A| @ |W|) + eps |b|.
    Elements that are exactly 0 with a zero bound (zero-padded columns) are left out."""
    orig = variants.compact_rnn_forward
    if hasattr(orig, "_kink_orig"):
        orig = orig._kink_orig

    def wrapper(h, index, nin, edge_weights, edge_biases, use_avg, residual_states, W, b, activation, **kw):
        out, incoming = orig(h, index, nin, edge_weights, edge_biases, use_avg, residual_states, W, b, activation, **kw)
        A = torch.cat(list(residual_states) + [incoming, h], dim=1).detach().double()
        W64, b64 = W.detach().double(), b.detach().double()
        pre = (A @ W64 + b64).abs()
        bound = 4e-7 * (A.abs() @ W64.abs()) + 2.0 ** -24 * b64.abs()
        live = bound > 0
        ratios.append(float((pre[live] / bound[live]).min()) if bool(live.any()) else float("inf"))
        return out, incoming
    wrapper._kink_orig = orig
    monkeypatch.setattr(variants, "compact_rnn_forward", wrapper)


@pytest.mark.parametrize("config", [H128, dict(README, hidden_size=128)], ids=["rnn-h128-residual", "readme-h128"])
def test_backward_equals_autograd_of_torch_restatement(pkg, oracle, cuda, config, monkeypatch):
    """Section (d) of tests/test_gpu_rnn_route.py with the panel cell in the forward: both backward passes start from the same HIP
    forward; for ReLU the weights are drawn with the first seed from 4 on for which every pre-activation of the run stays beyond
    KINK_FACTOR x its a-priori float32 rounding bound (a criterion on the forward's inputs and float64 arithmetic only).  Eight ReLU
    layers at width 128 have 1.6 x the pre-activations of that file's widest ReLU case and no seed in its range 4 .. 19 clears the
    factor on its 80-graph batch (smallest ratios 0.02 .. 1.4 per seed), so the batch here is 24 graphs and the range 4 .. 99."""
    variants = import_module(pkg.__name__ + ".variants")
    KINK_FACTOR = 2.0
    relu = str(config.get("graph_rnn_activation", "tanh")).lower() == "relu"
    ms = pkg.synthetic_qm9(24, mean_nodes=10, seed=4)

    def run(seed, mode):
        monkeypatch.setattr(variants, "BACKWARD_ORACLE", variant_oracle.autograd_backward if mode else None)
        model, _ = _model(pkg, oracle, ms, dict(config, edge_weight_dropout_keep_prob=1.0), panel=True, seed=seed)
        assert model.rnn_panel_route()
        feed = _feed(model)
        variables = model.trainable_variables
        for v in variables.values():
            v.requires_grad_(True); v.grad = None
        model.training = True
        counts = _count(pkg, monkeypatch, ("rnn_panel_gather", "rnn"))
        loss = model.forward_batch(feed)
        loss.backward()
        model.training = False
        steps = sum(model.params["layer_timesteps"])
        assert counts["rnn_panel_gather"][0] == steps and counts["rnn"][0] == 0
        return {k: v.grad.detach().double().cpu() for k, v in variables.items()}, float(loss.detach()), steps

    grads = {}
    for seed in range(4, 100):
        ratios = []
        _kink_recorder(variants, monkeypatch, ratios)       # (both runs of a seed are recorded: the forward is the same)
        grads[False], grads[(False, "loss")], steps = run(seed, False)
        assert len(ratios) == steps
        print("weight seed %d: smallest |pre| / rounding bound per timestep %s" % (seed, ["%.3g" % r for r in ratios]))
        if not relu or min(ratios) > KINK_FACTOR:
            break
    else:
        raise AssertionError("no weight seed in 4 .. 99 keeps every ReLU pre-activation off the kink")
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
    for panel in (True, False):
        model, _ = _model(pkg, oracle, ms, dict(README, hidden_size=128, edge_weight_dropout_keep_prob=0.8), panel=panel, seed=5)
        assert model.rnn_route() and model.rnn_panel_route() == panel
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
