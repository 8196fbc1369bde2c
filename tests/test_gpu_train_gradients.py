"""The gradient the optimiser consumes in one training step -- the flat buffer TFAdam.clip_and_apply clips and applies --
against float64 torch autograd of the oracle (tests/train_reference.py): the native step of the default model (train_native.py,
csrc/ggnn_train.hip) and the autograd path with its weight-gradient sink, at test size and at the benchmark's batch size; and
the fused GRU backward kernel against its formulas in float64 at shape edges.

Adam's first update is lr * g / (|g| + eps'), so tests of the weights after a step see the sign of every gradient entry and
little of its size; these compare the gradient itself."""
import numpy as np
import pytest
import torch

import train_reference as tr

pytestmark = pytest.mark.gpu

SMALL_CONFIGS = [                                                                  # (those of test_native_training_step_equals_autograd_path)
    ({}, (1.0, 1.0)),
    ({}, (0.8, 0.9)),
    ({"hidden_size": 64, "layer_timesteps": [2, 1, 2], "residual_connections": {"1": [0], "2": [0, 1]},
      "use_edge_msg_avg_aggregation": False, "graph_rnn_activation": "ReLU"}, (0.8, 1.0)),
    # two tasks; the int key is what chem_tensorflow.py:168 reads (the str key only drives the label sampling), so the second
    # task's loss and gradients carry the factor 1 / 0.5
    ({"layer_timesteps": [1, 2], "residual_connections": {"1": [1, 0]}, "task_ids": [0, 1], "task_sample_ratios": {"1": 0.5, 1: 0.5}},
     (1.0, 1.0)),
]
SMALL_IDS = ["default", "dropout", "h64-sum-relu", "two-tasks"]


def _small(pkg, oracle, config, keeps):
    ms = pkg.synthetic_qm9(300, mean_nodes=10, seed=4, num_tasks=max(config.get("task_ids", [0])) + 1)
    model = pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms, "--config": dict(config)})
    layers = oracle.make_sparse_layers(np.random.default_rng(4), model.params, model.num_edge_types, random_bias=True)
    model.set_graph_weights(layers)
    feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=False))))
    feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"] = keeps
    return model, layers, feed


def _step_against_oracle(pkg, oracle, oracle_torch, model, layers, feed, device="cpu"):
    """One train_batch under the capture -> (loss, captured gradients, oracle loss, oracle gradients, masks)."""
    masks = tr.dropout_masks(oracle, model, feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"])
    want_loss, want = tr.oracle_loss_and_grads(oracle_torch, model, layers, feed, masks, device=device)
    with tr.capture_step_gradients(model) as steps:
        loss = float(model.train_batch(feed))
    torch.cuda.synchronize()
    assert len(steps) == 1
    return loss, steps[0], want_loss, want, masks


def _check_masked_entries(got, masks):
    if masks["edge"] is not None:
        for l, m in enumerate(masks["edge"]):
            g = got["graph_model/gnn_layer_%i/gnn_edge_weights_%i:0" % (l, l)].cpu().numpy()
            assert (g[m == 0] == 0).all(), "layer %d: a dropped edge weight has a gradient" % l
            assert (g[m != 0] != 0).mean() > 0.5                      # (and the kept ones mostly do)
    if masks["readout"] is not None:
        for (kind, task_id), m in masks["readout"].items():
            name = "out_layer_task%i/%s/MLP_W_layer0:0" % (task_id, "regression_gate" if kind == "regression_gate" else "regression")
            assert (got[name].cpu().numpy()[m == 0] == 0).all(), name


def _expected_gru_formats(pkg, model):
    p = model.params
    provable = p["graph_rnn_activation"].lower() == "tanh" and p["use_edge_msg_avg_aggregation"]
    return [pkg.formats.F16X2 if provable else pkg.formats.BF16X3] * len(p["layer_timesteps"])


@pytest.mark.parametrize("config,keeps", SMALL_CONFIGS, ids=SMALL_IDS)
def test_native_step_gradients_match_fp64(pkg, oracle, oracle_torch, cuda, config, keeps, monkeypatch):
    """train_native.native_step on the default route: forward and backward launch sequences, readout + loss backward, the 1 / keep scaling of
    the dropped weights' gradient views and the per-task d_stats factors -- the gradient handed to clip + Adam equals the fp64
    oracle's (2e-4 of the variable's largest entry, as the other gradient tests)."""
    monkeypatch.setattr(pkg.formats._local, "policy", "auto", raising=False)
    model, layers, feed = _small(pkg, oracle, config, keeps)
    assert pkg.train_native.eligible(model, feed)
    loss, got, want_loss, want, masks = _step_against_oracle(pkg, oracle, oracle_torch, model, layers, feed)
    assert abs(loss - want_loss) < 1e-5 * max(1.0, abs(want_loss)), (loss, want_loss)
    if pkg.formats.split_path():
        assert model.last_gru_formats == _expected_gru_formats(pkg, model)
    tr.assert_gradients_match(got, want)
    _check_masked_entries(got, masks)
    tr.assert_comparison_has_teeth(got, want)


@pytest.mark.parametrize("config,keeps", SMALL_CONFIGS + [({"use_edge_bias": True, "layer_timesteps": [2, 1], "residual_connections": {"1": [0]}},
                                                           (0.8, 0.9))], ids=SMALL_IDS + ["edge-bias"])
def test_autograd_train_batch_gradients_match_fp64(pkg, oracle, oracle_torch, cuda, config, keeps, monkeypatch):
    """The autograd path of train_step (backward.PropagationStepFn) with the side-stream weight-gradient sink on and
    TFAdam.load_gradients adding the autograd part in place: the same fp64 check on the flat buffer."""
    monkeypatch.setattr(pkg.backward, "USE_NATIVE_STEP", False)
    monkeypatch.setattr(pkg.backward, "USE_WGRAD_STREAM", True)
    model, layers, feed = _small(pkg, oracle, config, keeps)
    assert not pkg.train_native.eligible(model, feed)
    loss, got, want_loss, want, masks = _step_against_oracle(pkg, oracle, oracle_torch, model, layers, feed)
    assert abs(loss - want_loss) < 1e-5 * max(1.0, abs(want_loss)), (loss, want_loss)
    assert pkg.backward._SINK.stream is not None
    for l in range(len(model.params["layer_timesteps"])):
        assert model._edge_weight_vars[l].data_ptr() in pkg.backward._SINK.used
    tr.assert_gradients_match(got, want)
    _check_masked_entries(got, masks)
    tr.assert_comparison_has_teeth(got, want)


# ---- the benchmark's training batch ---------------------------------------------------------------------------------------------
BENCH_SEED = 1


@pytest.fixture(scope="module")
def bench_molecules(pkg):
    return pkg.synthetic_qm9(5700, mean_nodes=18, seed=BENCH_SEED)


@pytest.mark.parametrize("policy", ["auto", "exact"])
def test_bench_size_native_step_gradients_match_fp64(pkg, oracle, oracle_torch, cuda, bench_molecules, policy, monkeypatch):
    """One native step of the default model (hidden 100, layer_timesteps [2,2,1,2,1] with its residual inputs, 4 edge types) on
    a ~100k-node batch packed as bench.py --mode train packs it: h0 uniform in (-1, 1) and declared so, edge-weight keep 0.8,
    readout keep 1.0.  The oracle runs in float64 on the device.  Per variable:
        normwise  ||got - want|| / ||want||    <= NORM_TOL
        max-abs   max |got - want| / max |want| <= MAX_TOL
    Measured on the MI355X (V = 99,989; worst of the 30 variables, both policies): normwise 3.7e-7 (layer 0 candidate
    kernel), max-abs 4.7e-7 (layer 0 gates kernel), loss 2.1e-8 relative.  The bounds are 8x those; 2e-4, the small-batch
    tests' bound, would let a 1e-4 relative error in any variable's gradient through."""
    monkeypatch.setattr(pkg.formats._local, "policy", policy, raising=False)
    model = pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": None, "valid_data": bench_molecules})
    p = model.params
    assert (p["hidden_size"], p["layer_timesteps"], model.num_edge_types) == (100, [2, 2, 1, 2, 1], 4)
    layers = oracle.make_sparse_layers(np.random.default_rng(7), p, model.num_edge_types, random_bias=True)
    model.set_graph_weights(layers)
    feed = dict(next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False))))
    V = int(feed["initial_node_representation"].shape[0])
    assert 90000 < V <= 100000 and V % 16 != 0, V
    gen = torch.Generator(device="cpu").manual_seed(1234)
    feed["initial_node_representation"] = (torch.rand((V, 100), generator=gen) * 2 - 1).to(cuda)
    pkg.formats.declare_h0_absmax(feed, 1.0)
    feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"] = p["edge_weight_dropout_keep_prob"], 1.0
    assert feed["edge_weight_dropout_keep_prob"] == 0.8
    assert pkg.train_native.eligible(model, feed)
    loss, got, want_loss, want, masks = _step_against_oracle(pkg, oracle, oracle_torch, model, layers, feed, device=cuda)
    if pkg.formats.split_path():
        fmt = pkg.formats.F16X2 if policy == "auto" else pkg.formats.BF16X3
        assert model.last_gru_formats == [fmt] * 5
    errs = tr.normwise_errors(got, want)
    assert abs(loss - want_loss) <= 2e-7 * abs(want_loss), (loss, want_loss)
    bad = {k: e for k, e in errs.items() if not (e[0] <= NORM_TOL and e[1] <= MAX_TOL)}
    assert not bad, bad
    _check_masked_entries(got, masks)
    tr.assert_comparison_has_teeth(got, want, rtol=MAX_TOL, atol=0.0)


NORM_TOL, MAX_TOL = 3e-6, 4e-6


# ---- the fused GRU backward kernel ---------------------------------------------------------------------------------------------
U32 = 2.0 ** -24


def _gru_bwd_formulas(g, h, r, u, c, Wg, Wc, nx, act, den):
    """include/ggnn_hip.h (ggnn_gru_bwd_fused_f32), every operand float64:
    dpc = g (1-u) act'(c); dpu = g (h-c) u (1-u); drh = dpc Wc^T[h rows]; dpr = drh h r (1-r);
    dh = g u + drh r + [dpr|dpu] Wg^T[h rows]; dx[s] = dpc Wc^T[x_s rows] + [dpr|dpu] Wg^T[x_s rows], the last / den."""
    D = h.shape[1]
    dact = (1 - c * c) if act == "tanh" else (c > 0).to(c.dtype)
    dpc = g * (1 - u) * dact
    dpu = g * (h - c) * u * (1 - u)
    drh = dpc @ Wc[nx * D:].t()
    dpr = drh * h * r * (1 - r)
    dpg = torch.cat([dpr, dpu], 1)
    dh = g * u + drh * r + dpg @ Wg[nx * D:].t()
    dx = [dpc @ Wc[s * D:(s + 1) * D].t() + dpg @ Wg[s * D:(s + 1) * D].t() for s in range(nx)]
    if den is not None:
        dx[-1] = dx[-1] / den
    return dpc, dpg, r * h, dh, dx


@pytest.mark.parametrize("nx", [1, 2, 3])
@pytest.mark.parametrize("D", [32, 64, 100])
@pytest.mark.parametrize("V", [1, 17, 4099, 37571, 100003])
def test_fused_gru_backward_against_fp64(pkg, oracle_torch, cuda, V, D, nx):
    """ggnn_gru_bwd_fused_f32 and its gather form, tanh and ReLU, mean (with in-degree-0 rows) and sum aggregation, against the
    header's formulas evaluated in float64 on the kernel's own fp32 inputs (r, u, c of an fp64 forward rounded to fp32).  The
    formulas are first checked against fp64 autograd of oracle_torch.gru.  Per element |got - want| <= C 2^-24 m, m the same
    formula on absolute values (|1 - c^2| -> 1 + c^2, |h - c| -> |h| + |c|).  Measured worst C over all cases: 13.9 (V = 100003,
    D = 100, nx = 3), 10-12 at V = 4099; C = 32 is below the worst case of a K-term fp32 sum (K = 2D .. 4D), far above a
    wrong formula or operand (a dropped term or factor is an O(1 / 2^-24) error).
    V = 37571 is the smallest V at 256 CUs where a workgroup runs a full-round pass followed by a tail pass (2349 tiles: 2048 in
    the full round, the rest as thin tail tickets): the carry of the prefetched inputs across passes, the ring parity and the
    next-tile prefetch, without the 100003-row case."""
    ops = pkg.ops
    T = 4
    gen = torch.Generator(device=cuda).manual_seed(V * 1000 + D * 10 + nx)
    rnd = lambda *s, scale=1.0: ((torch.rand(*s, generator=gen, device=cuda, dtype=torch.float64) * 2 - 1) * scale).float()
    h = rnd(V, D)
    xs = [rnd(V, D) for _ in range(nx)]
    Wg = rnd((nx + 1) * D, 2 * D, scale=(6.0 / ((nx + 2) * D)) ** 0.5)
    Wc = rnd((nx + 1) * D, D, scale=(6.0 / ((nx + 2) * D)) ** 0.5)
    bg, bc = 1 + rnd(2 * D, scale=0.2), rnd(D, scale=0.2)
    g = rnd(V, D)
    nin = torch.randint(0, 3, (V, T), generator=gen, device=cuda).float()
    nin[torch.rand(V, generator=gen, device=cuda) < 0.2] = 0                      # rows without incoming messages
    packed = ops.PackedWeights().gru_bwd(Wg, Wc, nx, D)
    # the gather form's extra rows: node v owns 0..4 rows of Z, not adjacent
    counts = torch.randint(0, 5, (V,), generator=gen, device=cuda)
    R = int(counts.sum())
    Z = rnd(max(R, 1), D)
    perm = torch.randperm(max(R, 1), generator=gen, device=cuda)[:R].to(torch.int32)
    start = torch.cumsum(counts, 0) - counts
    heads = torch.full((V, 4), -1, dtype=torch.int32, device=cuda)
    zsum = torch.zeros(V, D, dtype=torch.float64, device=cuda); zabs = torch.zeros_like(zsum)
    for k in range(4):
        has = counts > k
        heads[has, k] = perm[start[has] + k]
        zk = Z.double()[heads[:, k].clamp_min(0).long()] * has[:, None]
        zsum += zk; zabs += zk.abs()
    f64 = lambda t: t.double()
    for act in ("tanh", "relu"):
        fn = torch.tanh if act == "tanh" else torch.relu
        # fp64 forward -> r, u, c; the formulas against autograd (unrounded), then rounded to fp32 as the kernel's inputs
        X = torch.cat([f64(x) for x in xs], 1)
        hh = f64(h).requires_grad_(True)
        xl = [f64(x).requires_grad_(True) for x in xs]
        Wg64, Wc64 = f64(Wg).requires_grad_(True), f64(Wc).requires_grad_(True)
        out = oracle_torch.gru(torch.cat(xl, 1), hh, Wg64, f64(bg), Wc64, f64(bc), fn)
        (out * f64(g)).sum().backward()
        gates = torch.sigmoid(torch.cat([X, f64(h)], 1) @ f64(Wg) + f64(bg))
        r64, u64 = gates[:, :D], gates[:, D:]
        c64 = fn(torch.cat([X, r64 * f64(h)], 1) @ f64(Wc) + f64(bc))
        chk = _gru_bwd_formulas(f64(g), f64(h), r64, u64, c64, f64(Wg), f64(Wc), nx, act, None)
        for a, b in [(chk[3], hh.grad)] + list(zip(chk[4], [x.grad for x in xl])):
            assert float((a - b).abs().max()) <= 1e-12 * (1 + float(b.abs().max()))
        dWc = torch.cat([X, r64 * f64(h)], 1).t() @ chk[0]
        assert float((dWc - Wc64.grad).abs().max()) <= 1e-12 * (1 + float(dWc.abs().max()))
        r, u, c = r64.float().contiguous(), u64.float().contiguous(), c64.float().contiguous()
        for use_avg in (True, False):
            deg = nin.double().sum(1, keepdim=True)
            den = deg + float(np.float32(1e-7)) if use_avg else None
            for gather in (False, True):
                got = ops.gru_bwd_fused(g, h, r, u, c, packed, nin, use_avg, nx, act, gather=(Z, heads) if gather else None)
                geff = f64(g) + (zsum if gather else 0)
                want = _gru_bwd_formulas(geff, f64(h), f64(r), f64(u), f64(c), f64(Wg), f64(Wc), nx, act, den)
                # magnitudes: the same formulas on absolute values
                ga = f64(g).abs() + (zabs if gather else 0)
                ra, ua, ca, ha = f64(r), f64(u), f64(c), f64(h).abs()
                mdact = (1 + ca * ca) if act == "tanh" else (ca > 0).double()
                mpc = ga * (1 - ua) * mdact
                mpu = ga * (ha + ca.abs()) * ua * (1 - ua)
                mrh = mpc @ f64(Wc)[nx * D:].abs().t()
                mpg = torch.cat([mrh * ha * ra * (1 - ra), mpu], 1)
                mags = [mpc, mpg, ra * ha, ga * ua + mrh * ra + mpg @ f64(Wg)[nx * D:].abs().t(),
                        [mpc @ f64(Wc)[s * D:(s + 1) * D].abs().t() + mpg @ f64(Wg)[s * D:(s + 1) * D].abs().t() for s in range(nx)]]
                if use_avg:
                    mags[4][-1] = mags[4][-1] / den
                flat = lambda o: list(o[:4]) + list(o[4])
                ratios = []
                for a, b, m in zip(flat(got), flat(want), flat(mags)):
                    err = (f64(a) - b).abs()
                    ratios.append(float((err / (U32 * m + 1e-300)).max()) if err.numel() else 0.0)
                print("gru_bwd V=%d D=%d nx=%d %s avg=%d gather=%d worst C %.2f" % (V, D, nx, act, use_avg, gather, max(ratios)))
                for i, ratio in enumerate(ratios):
                    assert ratio <= GRU_BWD_C, (act, use_avg, gather, ["dpc", "dpg", "rh", "dh"][i] if i < 4 else "dx%d" % (i - 4), ratio)


GRU_BWD_C = 32.0
