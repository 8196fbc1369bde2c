"""The native training step of the default sparse model at hidden sizes 128 / 192 / 256 (params['native_panel_training'];
train_native.ROUTES, entry `panel`, on the panel route of csrc/ggnn_train.hip): the gradient the optimiser consumes against float64
autograd of the oracle with proof that the two-call step ran, the step against the autograd step it replaces, its determinism,
the one-launch image preparation against per-layer packing bit for bit, the accumulate form of the row-split product
(ggnn_gemm_tn_acc_f32), and everything that keeps the old step."""
import ctypes

import numpy as np
import pytest
import torch

import train_reference as tr
from test_gpu_train import NATIVE_VS_AUTOGRAD_GRAD_RTOL
from test_gpu_train_gradients import _check_masked_entries, _small

pytestmark = pytest.mark.gpu

KEY = "native_panel_training"

PANEL_CONFIGS = [
    ({"hidden_size": 128}, (1.0, 1.0)),
    ({"hidden_size": 192, "layer_timesteps": [2, 1], "residual_connections": {"1": [0]}, "graph_rnn_activation": "ReLU",
      "use_edge_msg_avg_aggregation": False}, (1.0, 1.0)),
    ({"hidden_size": 256, "task_ids": [0, 1], "task_sample_ratios": {"1": 0.5, 1: 0.5}}, (0.8, 0.9)),
    # 8 edge types: T > 4 runs the stand-alone node sums instead of the sum gathered by the next GRU backward
    ({"hidden_size": 128, "tie_fwd_bkwd": False}, (1.0, 1.0)),
]
PANEL_IDS = ["h128", "h192-sum-relu-residual", "h256-dropout-two-tasks", "h128-untied-8-types"]


def _count_routes(pkg, monkeypatch):
    """Counters on the three places a step can go through: the native step on the panel route, the autograd route's fused GRU
    backward, and the autograd forward."""
    calls = {"native_panel": 0, "gru_bwd_fused": 0, "forward_batch": 0}
    native, fused = pkg.train_native.native_step, pkg.ops.gru_bwd_fused
    forward = pkg.SparseGGNNChemModel.forward_batch

    def native_counted(route, *a, **k):
        calls["native_panel"] += route.name == "panel"
        return native(route, *a, **k)

    def fused_counted(*a, **k):
        calls["gru_bwd_fused"] += 1
        return fused(*a, **k)

    def forward_counted(self, *a, **k):
        calls["forward_batch"] += 1
        return forward(self, *a, **k)

    monkeypatch.setattr(pkg.train_native, "native_step", native_counted)
    monkeypatch.setattr(pkg.ops, "gru_bwd_fused", fused_counted)
    monkeypatch.setattr(pkg.SparseGGNNChemModel, "forward_batch", forward_counted)
    return calls


@pytest.mark.parametrize("config,keeps", PANEL_CONFIGS, ids=PANEL_IDS)
def test_native_panel_step_gradients_match_fp64(pkg, oracle, oracle_torch, cuda, config, keeps, monkeypatch):
    """One train_batch per configuration with the key set: loss to 1e-5 relative, every variable's gradient to the project's bound
    (2e-4 of its largest entry) against the fp64 oracle, dropped weights without gradient -- and the step was ONE call of
    native_step on the panel route, with no fused-GRU-backward op call and no autograd forward."""
    calls = _count_routes(pkg, monkeypatch)
    model, layers, feed = _small(pkg, oracle, dict(config, **{KEY: True}), keeps)
    assert model.num_edge_types == (8 if config.get("tie_fwd_bkwd") is False else 4)
    assert pkg.train_native.panel_eligible(model, feed)
    assert not pkg.train_native.eligible(model, feed)            # (the whole-block native step keeps refusing the panel sizes)
    assert model.threaded_batches_default() is False
    masks = tr.dropout_masks(oracle, model, *keeps)
    want_loss, want = tr.oracle_loss_and_grads(oracle_torch, model, layers, feed, masks, device=cuda)
    with tr.capture_step_gradients(model) as steps:
        loss = float(model.train_batch(feed))
    torch.cuda.synchronize()
    assert len(steps) == 1
    got = steps[0]
    assert calls == {"native_panel": 1, "gru_bwd_fused": 0, "forward_batch": 0}, calls
    assert abs(loss - want_loss) < 1e-5 * max(1.0, abs(want_loss)), (loss, want_loss)
    tr.assert_gradients_match(got, want)
    _check_masked_entries(got, masks)
    tr.assert_comparison_has_teeth(got, want)


def _three_steps(pkg, oracle, config, keeps, key):
    model, _, feed = _small(pkg, oracle, dict(config, **({KEY: True} if key else {})), keeps)
    assert pkg.train_native.panel_eligible(model, feed) == key
    with tr.capture_step_gradients(model) as grads:
        losses = [model.train_batch(feed) for _ in range(3)]
    torch.cuda.synchronize()
    assert len(grads) == 3
    return (torch.stack(losses).cpu(), {k: v.detach().clone() for k, v in model.trainable_variables.items()},
            model.ops["final_node_representations"].detach().clone(), grads[0])


@pytest.mark.parametrize("config,keeps", PANEL_CONFIGS[:3], ids=PANEL_IDS[:3])
def test_native_panel_step_against_the_autograd_step(pkg, oracle, cuda, config, keeps):
    """Three steps from the same weights with the key on and off: the losses to rtol 2e-6, the gradients of step 1 within the project's
    native-vs-autograd bound (2e-6 of a variable's largest entry), the weights after three steps within 2e-5.  The two routes
    launch the same forward kernels except the GRU's place of the segment sum; the weight-gradient products differ in their order of
    summation (row-split partials here, returned to autograd there).
    Measured worst max|g1 - g0| / max|g0| on the MI355X: 2.2e-7 (h128), 0 (h192: bit-identical), 1.9e-7 (h256).  With the timesteps of
    a layer merged into one product (GGNN_TRAIN_MERGE_PRODUCTS=1, not the default on this route): 3.3e-7 / 2.7e-7 / 3.2e-7, and at h192
    the weights after three steps 2.17e-5 apart -- past this test's 2e-5."""
    (l1, w1, f1, g1), (l0, w0, f0, g0) = _three_steps(pkg, oracle, config, keeps, True), _three_steps(pkg, oracle, config, keeps, False)
    worst = 0.0
    for k in g0:
        err, scale = float((g1[k] - g0[k]).abs().max()), float(g0[k].abs().max())
        worst = max(worst, err / max(scale, 1e-300))
    print("native panel step vs autograd step, %s: worst max|dg| / max|g| = %.3g; losses %s vs %s" % (
        config, worst, l1.tolist(), l0.tolist()))
    np.testing.assert_allclose(l1.numpy(), l0.numpy(), rtol=2e-6)
    assert float((f1 - f0).abs().max()) < 2e-5
    assert set(g1) == set(g0)
    for k in g0:
        err, scale = float((g1[k] - g0[k]).abs().max()), float(g0[k].abs().max())
        assert err <= NATIVE_VS_AUTOGRAD_GRAD_RTOL * scale, (k, err, scale)
    for k in w0:
        assert float((w1[k] - w0[k]).abs().max()) < 2e-5, k       # three Adam steps of ~1e-3: <1 % of one step


@pytest.mark.parametrize("config,keeps", [PANEL_CONFIGS[1], PANEL_CONFIGS[2]], ids=[PANEL_IDS[1], PANEL_IDS[2]])
def test_native_panel_step_is_deterministic(pkg, oracle, cuda, config, keeps):
    """Two runs from the same weights: the same bits in every loss, every step-1 gradient and every weight after three steps (the
    side stream's products are ordered by events, every reduction has a fixed order)."""
    (l1, w1, f1, g1), (l2, w2, f2, g2) = _three_steps(pkg, oracle, config, keeps, True), _three_steps(pkg, oracle, config, keeps, True)
    assert torch.equal(l1, l2) and torch.isfinite(l1).all()
    assert torch.equal(f1, f2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for k in w1:
        assert torch.equal(w1[k], w2[k]), k


# ---- the one-launch image preparation --------------------------------------------------------------------------------------------
PREPARE_CONFIGS = [
    {"hidden_size": 128, "layer_timesteps": [1, 2], "residual_connections": {"1": [0]}},                 # nx 1 and 2
    {"hidden_size": 192, "layer_timesteps": [1, 1], "residual_connections": {"1": [0]}},
    {"hidden_size": 256, "layer_timesteps": [1, 1], "residual_connections": {"1": [0]}},
]


@pytest.mark.parametrize("keep", [1.0, 0.8])
@pytest.mark.parametrize("config", PREPARE_CONFIGS, ids=["h128", "h192", "h256"])
def test_panel_weight_preparation_equals_per_layer_packing(pkg, oracle, cuda, config, keep):
    """ggnn_sparse_train_panel_prepare_f32 (all of a step's panel images in one launch, weight-dropout mask on the fly) against the
    per-layer path: ggnn_dropout_f32 on the variable, a transpose copy, ggnn_edge_weights_pack_f32 twice, ggnn_gru_pack_weights_f32 in
    the layer's format, ggnn_gru_bwd_fused_f32(g = NULL) -- bit for bit, layers with one and with two inputs, the GRU forward exact
    and (on the split path, where the two-piece format exists) f16x2."""
    ms = pkg.synthetic_qm9(30, mean_nodes=8, seed=1)
    model = pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms, "--config": dict(config)})
    model.set_graph_weights(oracle.make_sparse_layers(np.random.default_rng(1), model.params, model.num_edge_types, random_bias=True))
    lib = pkg._lib.load()
    T, D, L = model.num_edge_types, model.params["hidden_size"], len(model.params["layer_timesteps"])
    cells = model.gnn_weights.rnn_cells
    nxs = [len(model.params["residual_connections"].get(str(l)) or []) + 1 for l in range(L)]
    assert nxs == [1, 2]
    f32 = lambda nbytes: torch.full((nbytes // 4,), float("nan"), device=cuda)
    eb = lib.ggnn_msg_transform_compact_workspace_bytes(D, T)
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    seeds = [model.dropout_seed("edge_weights", l) for l in range(L)]
    split = pkg.formats.split_path()
    for fmts in ([pkg.formats.BF16X3] * L, [pkg.formats.F16X2, pkg.formats.BF16X3], [pkg.formats.BF16X3, pkg.formats.F16X2]):
        if not split and fmts != [pkg.formats.BF16X3] * L:
            continue
        imgs = ([f32(eb) for _ in range(L)], [f32(eb) for _ in range(L)], [f32(lib.ggnn_gru_packed_bytes(D, nxs[l])) for l in range(L)],
                [f32(lib.ggnn_gru_bwd_packed_bytes(D, nxs[l])) for l in range(L)])
        pkg._lib.check(lib.ggnn_sparse_train_panel_prepare_f32(
            L, T, D, (ctypes.c_int32 * L)(*nxs), ptrs(model._edge_weight_vars), keep, (ctypes.c_uint64 * L)(*seeds),
            ptrs([c.gates_kernel for c in cells]), ptrs([c.candidate_kernel for c in cells]), (ctypes.c_int32 * L)(*fmts), ptrs(imgs[0]),
            ptrs(imgs[1]), ptrs(imgs[2]), ptrs(imgs[3]), torch.cuda.current_stream().cuda_stream))
        packed = pkg.ops.PackedWeights()
        for l in range(L):
            W = model._edge_weight_vars[l].view(T, D, D)
            if keep < 1.0:
                W = pkg.ops.dropout(W.contiguous(), keep, seeds[l])
            want = [packed.edge(W), packed.edge(W.transpose(1, 2).contiguous()),
                    packed.gru(cells[l].gates_kernel, cells[l].candidate_kernel, nxs[l], D, fmts[l]),
                    packed.gru_bwd(cells[l].gates_kernel, cells[l].candidate_kernel, nxs[l], D)]
            for k in range(4):
                n = want[k].numel() if k >= 2 else (eb - 256) // 4          # (the edge buffers end in 256 bytes of alignment slack)
                if k == 2 and fmts[l] == pkg.formats.F16X2:
                    # (the buffer is sized for the larger bf16x3 images: an f16x2 panel image is D / 32 chunks of two 4 KiB planes)
                    n = 3 * (nxs[l] + 1) * (D // 64) * (D // 32) * 8192 // 4
                assert not torch.isnan(imgs[k][l][:n]).any(), (fmts, l, k)
                assert torch.equal(imgs[k][l][:n].view(torch.int32), want[k][:n].view(torch.int32)), (fmts, l, k)


# ---- the accumulate form of the row-split product ------------------------------------------------------------------------------------
def _tn_acc(pkg, A, B, C, N, accumulate):
    lib = pkg._lib.load()
    M, K = A.shape
    wsb = lib.ggnn_gemm_tn_workspace_bytes(M, K, N)
    ws = torch.empty(wsb, dtype=torch.uint8, device=A.device)
    pkg._lib.check(lib.ggnn_gemm_tn_acc_f32(A.data_ptr(), A.stride(0) if M else K, B.data_ptr(), B.stride(0) if M else N, C.data_ptr(),
                                            C.stride(0), accumulate, M, K, N, ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


@pytest.mark.parametrize("K,N", [(128, 512), (192, 384), (256, 256)])
@pytest.mark.parametrize("M", [0, 1, 63, 65, 1000])
def test_gemm_tn_acc(pkg, cuda, M, K, N):
    """ggnn_gemm_tn_acc_f32: with accumulate = 0 and ldc = N the bits of ggnn_gemm_tn_f32; with accumulate = 1 into a non-zero
    [K, ldc] destination with ldc > N the columns beyond N untouched and the result within ggnn_gemm_tn_f32's own bound of the fp64
    sum (test_gpu_parity.test_gemm_tn: 1e-6 of the sum of the summands' magnitudes; C's old entry is one more summand of the sum).
    A is an unaligned view (row stride K + 3, column offset 1) of a wider matrix.  M == 0 with accumulate leaves C untouched."""
    rng = np.random.default_rng(M + K + N)
    Aw = rng.uniform(-1, 1, (M, K + 3)).astype(np.float32)
    Bh = rng.uniform(-1, 1, (M, N)).astype(np.float32)
    Ad, Bd = torch.from_numpy(Aw).to(cuda)[:, 1:1 + K], torch.from_numpy(Bh).to(cuda)
    A = Aw[:, 1:1 + K]
    plain = pkg.ops.gemm_tn(Ad, Bd) if M else torch.zeros((K, N), device=cuda)
    got = torch.full((K, N), float("nan"), device=cuda)
    _tn_acc(pkg, Ad, Bd, got, N, 0)
    assert torch.equal(got, plain)
    ldc = N + 8
    C0 = rng.uniform(-1, 1, (K, ldc)).astype(np.float32)
    Cd = torch.from_numpy(C0).to(cuda)
    _tn_acc(pkg, Ad, Bd, Cd, N, 1)
    C1 = Cd.cpu().numpy()
    assert np.array_equal(C1[:, N:], C0[:, N:])
    if M == 0:
        assert np.array_equal(C1, C0)
        return
    want = A.astype(np.float64).T @ Bh.astype(np.float64)
    bound = 1e-6 * (np.abs(A).astype(np.float64).T @ np.abs(Bh).astype(np.float64) + np.abs(C0[:, :N])) + 1e-30
    assert np.all(np.abs(C1[:, :N] - (C0[:, :N].astype(np.float64) + want)) <= bound)
    # deterministic, and exactly the plain product added once
    assert np.array_equal(C1[:, :N], C0[:, :N] + plain.cpu().numpy())
    Cd2 = torch.from_numpy(C0).to(cuda)
    _tn_acc(pkg, Ad, Bd, Cd2, N, 1)
    assert torch.equal(Cd2, Cd)


# ---- what keeps the old step -----------------------------------------------------------------------------------------------------
KEEPS_OLD_STEP = {
    "key-off": ({"hidden_size": 128}, {}),
    "h116-padded": ({"hidden_size": 116, KEY: True}, {}),
    "edge-bias": ({"hidden_size": 128, "use_edge_bias": True, KEY: True}, {}),
    "rnn-cell": ({"hidden_size": 128, "graph_rnn_cell": "RNN", KEY: True}, {}),
    "attention": ({"hidden_size": 128, "use_propagation_attention": True, KEY: True}, {}),
    "four-inputs": ({"hidden_size": 128, "layer_timesteps": [1, 1, 1, 1], "residual_connections": {"3": [0, 1, 2]}, KEY: True}, {}),
    "state-dropout": ({"hidden_size": 128, KEY: True}, {"graph_state_keep_prob": 0.9}),
}


@pytest.mark.parametrize("case", list(KEEPS_OLD_STEP))
def test_steps_the_panel_route_cannot_take_keep_the_old_step(pkg, cuda, monkeypatch, case):
    config, feed_extra = KEEPS_OLD_STEP[case]
    calls = _count_routes(pkg, monkeypatch)
    ms = pkg.synthetic_qm9(40, mean_nodes=8, seed=1)
    model = pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms, "--config": dict(config)})
    feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=False))), **feed_extra)
    assert not pkg.train_native.panel_eligible(model, feed), case
    assert not pkg.train_native.eligible(model, feed), case
    assert np.isfinite(float(model.train_batch(feed)))
    assert calls["native_panel"] == 0 and calls["forward_batch"] == 1, calls


def test_hidden_100_with_the_key_keeps_the_default_native_step_bit_for_bit(pkg, oracle, cuda, monkeypatch):
    calls = _count_routes(pkg, monkeypatch)
    runs = []
    for key in (True, False):
        model, _, feed = _small(pkg, oracle, {KEY: True} if key else {}, (0.8, 0.9))
        assert pkg.train_native.eligible(model, feed) and not pkg.train_native.panel_eligible(model, feed)
        with tr.capture_step_gradients(model) as grads:
            loss = model.train_batch(feed)
        torch.cuda.synchronize()
        runs.append((loss.cpu(), grads[0]))
    assert calls == {"native_panel": 0, "gru_bwd_fused": 0, "forward_batch": 0}, calls
    (l1, g1), (l0, g0) = runs
    assert torch.equal(l1, l0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


@pytest.mark.parametrize("D", [128, 192, 256])
def test_whole_block_native_step_stays_ineligible_at_the_wide_sizes_with_the_key(pkg, cuda, D):
    ms = pkg.synthetic_qm9(40, mean_nodes=8, seed=1)
    model = pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                     "--config": {"hidden_size": D, KEY: True}})
    feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=False))))
    assert not pkg.train_native.eligible(model, feed) and not pkg.train_native.model_eligible(model)
    assert pkg.train_native.panel_eligible(model, feed) and pkg.train_native.panel_model_eligible(model)
    with pkg.ops.kernel_timing():                                # per-launch timing keeps the autograd step
        assert not pkg.train_native.panel_eligible(model, feed)
