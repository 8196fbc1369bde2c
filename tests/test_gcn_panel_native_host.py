"""The sparse GCN's native training step at hidden sizes 128 / 192 / 256 (params['native_training'] with params['gcn_panel_layers'])
on the host: argument validation of the six ggnn_gcn_panel_* training entry points before any launch, and the eligibility predicates
on a CPU-device model with both keys.  No GPU needed."""


def test_gcn_panel_native_entry_points_validate_without_gpu(pkg):
    lib = pkg._lib.load()
    c = pkg.ops.ctypes
    fake, other = 256, 512
    assert [lib.ggnn_gcn_panel_train_supported(d) for d in (100, 128, 160, 192, 256)] == [0, 1, 0, 1, 1]
    # the D <= 100 family keeps its contract at the wide sizes
    assert [lib.ggnn_gcn_train_supported(d) for d in (100, 128, 192, 256)] == [1, 0, 0, 0]
    assert [lib.ggnn_gcn_fused_supported(d) for d in (100, 128, 192, 256)] == [1, 0, 0, 0]

    def bwd(dP=fake, gate=other, out=1024, V=5, D=128, keep=1.0):
        return lib.ggnn_gcn_panel_layer_bwd_f32(dP, fake, fake, fake, 4, fake, gate, None, 0, 0, keep, out, V, D, None)
    assert bwd(gate=None) == -1 and bwd(dP=None) == -1 and bwd(out=None) == -1      # null pointers
    assert bwd(gate=1024) == -1                              # gate_out aliased to out
    assert bwd(dP=1024) == -1                                # dP aliased to out
    assert bwd(gate=other + 4) == -1 and bwd(dP=fake + 4) == -1 and bwd(out=1024 + 4) == -1     # misaligned
    assert bwd(keep=0.0) == -1 and bwd(keep=1.5) == -1       # keep_prob outside (0, 1]
    assert bwd(D=100) == -2 and bwd(D=48) == -2              # no panel kernel
    assert bwd(dP=None, gate=None, out=None, V=0) == 0       # V == 0: nothing to do
    assert bwd(V=-1) == -1
    for D in (128, 192, 256):
        assert bwd(V=-(-(1 << 30) // D), D=D) == -2          # V*D >= 2^30: 32-bit byte offsets

    L = 3
    W = (c.c_void_p * L)(fake, fake, fake)
    assert lib.ggnn_gcn_panel_train_pack_f32(None, L, 128, fake, None) == -1
    assert lib.ggnn_gcn_panel_train_pack_f32(W, L, 128, None, None) == -1
    assert lib.ggnn_gcn_panel_train_pack_f32(W, L, 100, fake, None) == -2
    assert lib.ggnn_gcn_panel_train_pack_f32(W, L, 48, fake, None) == -2
    assert lib.ggnn_gcn_panel_train_pack_f32(W, 0, 128, fake, None) == -1
    assert lib.ggnn_gcn_panel_train_pack_f32(W, 65, 128, fake, None) == -1
    assert lib.ggnn_gcn_panel_train_pack_f32((c.c_void_p * L)(fake, None, fake), L, 128, fake, None) == -1

    seeds = (c.c_uint64 * L)(1, 2, 3)
    off = c.c_int64(0)

    def fwd(h0=fake, V=5, D=128, ws_bytes=1 << 30, keep=1.0, layers=L, weights=W):
        return lib.ggnn_gcn_panel_train_forward_f32(h0, V, D, layers, fake, fake, fake, 4, weights, None, None, seeds, keep, fake,
                                                    ws_bytes, c.byref(off), None)

    def back(d=fake, V=5, D=128, ws_bytes=1 << 30, keep=1.0, layers=L, weights=W, g_b=None):
        return lib.ggnn_gcn_panel_train_backward_f32(d, V, D, layers, fake, fake, fake, 4, None, seeds, keep, weights, g_b, fake,
                                                     ws_bytes, None, None)
    for call in (fwd, back):
        assert call(None) == -1                              # null pointer
        assert call(D=100) == -2 and call(D=48) == -2        # no native panel step
        assert call(V=(1 << 30) // 128) == -2                # V*D >= 2^30
        assert call(None, V=0, ws_bytes=0) == 0              # V == 0: nothing to do
        assert call(keep=0.0) == -1 and call(keep=1.5) == -1
        assert call(layers=0) == -1 and call(layers=65) == -1
        assert call(weights=(c.c_void_p * L)(fake, None, fake)) == -1       # null entry in W / g_W
        assert call(ws_bytes=16) == -3                       # workspace too small
        assert b"workspace" in lib.ggnn_last_error()
        for D in (128, 192, 256):
            assert call(D=D, ws_bytes=lib.ggnn_gcn_panel_train_workspace_bytes(5, D, L) - 1) == -3      # one byte short
    assert back(g_b=(c.c_void_p * L)(fake, None, fake)) == -1
    # the D <= 100 calls still refuse the wide sizes
    assert lib.ggnn_gcn_train_forward_f32(fake, 5, 128, L, fake, fake, fake, 4, W, None, None, seeds, 1.0, fake, 1 << 30,
                                          c.byref(off), None) == -2
    assert lib.ggnn_gcn_train_backward_f32(fake, 5, 128, L, fake, fake, fake, 4, None, seeds, 1.0, W, None, fake, 1 << 30, None,
                                           None) == -2

    for V, D, layers in ((1000, 128, 4), (17, 192, 1), (5, 256, 3)):
        images = (2 * layers - 1) * lib.ggnn_gcn_panel_image_bytes(D)
        assert lib.ggnn_gcn_panel_image_bytes(D) > 0
        assert lib.ggnn_gcn_panel_train_workspace_bytes(V, D, layers) >= images + 3 * layers * V * D * 4
    assert lib.ggnn_gcn_panel_train_workspace_bytes(1000, 100, 4) == 0
    assert lib.ggnn_gcn_panel_train_workspace_bytes(1000, 160, 4) == 0


def test_gcn_panel_eligibility_on_a_cpu_device(pkg):
    ms = pkg.synthetic_qm9(10, seed=1)
    tn = pkg.train_native
    m = pkg.SparseGCNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms,
                                "--config": {"hidden_size": 128, "num_timesteps": 2, "random_seed": 7, "native_training": True,
                                             "gcn_panel_layers": True}})
    assert m.gcn_panel_route() is False
    assert tn.gcn_model_eligible(m) is False
    feed = next(iter(m.make_minibatch_iterator(m.valid_data, is_training=False)))
    assert tn.gcn_eligible(m, feed) is False
    assert m.threaded_batches_default() is True              # (the autograd step: batches packed on the producer thread)
    defaults = pkg.SparseGCNChemModel.default_params()
    assert "native_training" not in defaults and "gcn_panel_layers" not in defaults
    assert callable(pkg.ops.gcn_panel_layer_bwd) and callable(pkg.ops.gcn_panel_train_pack)
