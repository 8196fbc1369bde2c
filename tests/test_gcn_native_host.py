"""The sparse GCN's native training step (params['native_training']) on the host: argument validation of the new C entry points,
the eligibility predicates on a CPU-device model, and the float64 step helper of gcn_train_reference.py against torch.autograd.
No GPU needed."""
import numpy as np
import torch

import gcn_train_reference as GR


def test_gcn_native_entry_points_validate_without_gpu(pkg):
    lib = pkg._lib.load()
    c = pkg.ops.ctypes
    fake, other = 256, 512
    assert [lib.ggnn_gcn_train_supported(d) for d in (32, 48, 64, 100, 128)] == [1, 0, 1, 1, 0]
    assert [lib.ggnn_gcn_fused_supported(d) for d in (32, 48, 64, 100, 128)] == [1, 0, 1, 1, 0]

    def bwd(dP=fake, gate=other, out=1024, V=5, D=64, keep=1.0):
        return lib.ggnn_gcn_layer_bwd_f32(dP, fake, fake, fake, 4, fake, gate, None, 0, 0, keep, out, V, D, None)
    assert bwd(gate=None) == -1                              # null gate_out
    assert bwd(gate=1024) == -1                              # gate_out aliased to out
    assert bwd(dP=1024) == -1                                # dP aliased to out
    assert bwd(gate=other + 4) == -1                         # misaligned gate_out
    assert bwd(keep=0.0) == -1 and bwd(keep=1.5) == -1       # keep_prob outside (0, 1]
    assert bwd(D=48) == -2                                   # no fused kernel for 48
    assert bwd(dP=None, gate=None, out=None, V=0) == 0       # V == 0: nothing to do
    assert bwd(V=-1) == -1

    L = 3
    W = (c.c_void_p * L)(fake, fake, fake)
    assert lib.ggnn_gcn_train_pack_f32(None, L, 64, fake, None) == -1
    assert lib.ggnn_gcn_train_pack_f32(W, L, 48, fake, None) == -2
    assert lib.ggnn_gcn_train_pack_f32(W, 0, 64, fake, None) == -1
    assert lib.ggnn_gcn_train_pack_f32(W, 65, 64, fake, None) == -1
    assert lib.ggnn_gcn_train_pack_f32((c.c_void_p * L)(fake, None, fake), L, 64, fake, None) == -1

    seeds = (c.c_uint64 * L)(1, 2, 3)
    off = c.c_int64(0)

    def fwd(h0=fake, V=5, D=64, ws_bytes=1 << 30, keep=1.0):
        return lib.ggnn_gcn_train_forward_f32(h0, V, D, L, fake, fake, fake, 4, W, None, None, seeds, keep, fake, ws_bytes,
                                              c.byref(off), None)

    def back(d=fake, V=5, D=64, ws_bytes=1 << 30, keep=1.0, g_b=None):
        return lib.ggnn_gcn_train_backward_f32(d, V, D, L, fake, fake, fake, 4, None, seeds, keep, W, g_b, fake, ws_bytes, None, None)
    for call in (fwd, back):
        assert call(None) == -1                              # null pointer
        assert call(D=48) == -2                              # no native step for 48
        assert call(V=(1 << 30) // 64) == -2                 # V*D >= 2^30: 32-bit byte offsets
        assert call(None, V=0, ws_bytes=0) == 0              # V == 0: nothing to do
        assert call(keep=0.0) == -1
        assert call(ws_bytes=16) == -3                       # workspace too small
        assert b"workspace" in lib.ggnn_last_error()
        assert call(ws_bytes=lib.ggnn_gcn_train_workspace_bytes(5, 64, L) - 1) == -3
    assert back(g_b=(c.c_void_p * L)(fake, None, fake)) == -1

    for V, D, layers in ((1000, 100, 4), (17, 32, 1), (5, 64, 3)):
        images = (2 * layers - 1) * lib.ggnn_gcn_image_bytes(D)
        assert lib.ggnn_gcn_train_workspace_bytes(V, D, layers) >= images + 3 * layers * V * D * 4
    assert lib.ggnn_gcn_train_workspace_bytes(1000, 48, 4) == 0


def _model(pkg, ms, **config):
    params = {"hidden_size": 32, "num_timesteps": 3, "random_seed": 7}
    params.update(config)
    return pkg.SparseGCNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": params})


def test_gcn_eligibility_on_a_cpu_device(pkg):
    ms = pkg.synthetic_qm9(10, seed=1)
    tn = pkg.train_native
    for config in ({}, {"native_training": True}):
        m = _model(pkg, ms, **config)
        assert tn.gcn_model_eligible(m) is False
        assert tn.model_eligible(m) is False and tn.dense_model_eligible(m) is False
        feed = next(iter(m.make_minibatch_iterator(m.valid_data, is_training=False)))
        assert tn.gcn_eligible(m, feed) is False and tn.gcn_eligible(m, {}) is False
        assert m.threaded_batches_default() is True         # (the autograd step: batches packed on the producer thread)
    assert "native_training" not in pkg.SparseGCNChemModel.default_params()
    # the predicates take any model
    sparse = pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms,
                                      "--config": {"hidden_size": 32, "native_training": True}})
    assert tn.gcn_model_eligible(sparse) is False


def test_fp64_step_helper_against_autograd(oracle_torch):
    """gcn_train_reference.fp64_step (gcn_reference_math's layers, the oracle's readout and loss) against plain torch.autograd on a
    dense float64 A_hat: asymmetric, with duplicate entries, negative weights and an empty row; bias; masks on the hidden layers;
    two tasks, one with a sample ratio (looked up by its int id, chem_tensorflow.py:168)."""
    rng = np.random.default_rng(5)
    V, D, L, G = 23, 8, 3, 4
    adj = rng.integers(0, V - 1, (70, 2))                 # (node V-1 has no entries: an empty row and column)
    adj = np.concatenate([adj, adj[:5]])                  # duplicate (i, j) entries
    w = rng.standard_normal(len(adj))
    h0 = rng.standard_normal((V, D))
    Ws = [rng.standard_normal((D, D)) * 0.5 for _ in range(L)]
    bs = [rng.standard_normal(D) * 0.1 for _ in range(L)]
    masks = [(rng.random((V, D)) < 0.7) / 0.7 for _ in range(L - 1)] + [None]
    gnl = np.sort(rng.integers(0, G, V))
    params = {"task_ids": [0, 2], "task_sample_ratios": {2: 0.5, "0": 0.25}}
    readouts = {t: (rng.standard_normal((2 * D, 1)) * 0.3, rng.standard_normal(1), rng.standard_normal((D, 1)) * 0.3,
                    rng.standard_normal(1)) for t in params["task_ids"]}
    targets = rng.standard_normal((2, G))
    tmask = np.array([[1.0, 1.0, 0.0, 1.0], [1.0, 0.0, 1.0, 1.0]])

    for biases in (bs, None):
        loss, got = GR.fp64_step(oracle_torch, params, h0, adj, w, Ws, biases, masks, readouts, gnl, G, targets, tmask)

        A = torch.zeros((V, V), dtype=torch.float64)
        A.index_put_((torch.from_numpy(adj[:, 0]), torch.from_numpy(adj[:, 1])), torch.from_numpy(w), accumulate=True)
        leaves = {}
        h = torch.from_numpy(h0)
        for l in range(L):
            W = leaves["graph_model/gcn_scope/gcn_weights_%i:0" % l] = torch.tensor(Ws[l], requires_grad=True)
            h = A @ h @ W
            if biases is not None:
                b = leaves["graph_model/gcn_scope/gcn_bias_%i:0" % l] = torch.tensor(biases[l], requires_grad=True)
                h = h + b
            if l < L - 1:
                h = torch.relu(h) * torch.from_numpy(masks[l])
        want_loss = 0.0
        for i, t in enumerate(params["task_ids"]):
            gW, gb, tW, tb = (torch.tensor(a, requires_grad=True) for a in readouts[t])
            for name, leaf in zip(GR.READOUT_NAMES, (gW, gb, tW, tb)):
                leaves["out_layer_task%i/%s:0" % (t, name)] = leaf
            gate = torch.sigmoid(torch.cat([h, torch.from_numpy(h0)], dim=1) @ gW + gb)
            pred = torch.zeros(G, 1, dtype=torch.float64).index_add_(0, torch.from_numpy(gnl), gate * (h @ tW + tb))[:, 0]
            diff = (pred - torch.from_numpy(targets[i])) * torch.from_numpy(tmask[i])
            task = (0.5 * diff * diff).sum() / (torch.from_numpy(tmask[i]).sum() + 1e-7)
            want_loss = want_loss + task * (2.0 if t == 2 else 1.0)
        want_loss.backward()
        assert set(got) == set(leaves)
        np.testing.assert_allclose(loss, float(want_loss), rtol=1e-10, atol=1e-10)
        for name, leaf in leaves.items():
            np.testing.assert_allclose(got[name].numpy(), leaf.grad.numpy(), rtol=1e-10, atol=1e-10, err_msg=name)
