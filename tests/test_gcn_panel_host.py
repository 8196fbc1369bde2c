"""The column-panel GCN layer (csrc/ggnn_gcn_panel.hip, hidden sizes 128 / 192 / 256) on the host: the predicates, the image and
workspace sizes, argument validation of its C entry points, and the model's opt-in key on a CPU device.  No GPU needed."""
import pytest

SIZES = (32, 48, 64, 100, 128, 192, 256, 320)


def test_predicates(pkg):
    lib = pkg._lib.load()
    assert [lib.ggnn_gcn_panel_supported(d) for d in SIZES] == [0, 0, 0, 0, 1, 1, 1, 0]
    assert [pkg.ops.gcn_panel_supported(d) for d in SIZES] == [False, False, False, False, True, True, True, False]
    # the existing predicates keep their values: the panel kernel is a route of its own
    assert [lib.ggnn_gcn_fused_supported(d) for d in SIZES] == [1, 0, 1, 1, 0, 0, 0, 0]
    assert [lib.ggnn_gcn_train_supported(d) for d in SIZES] == [1, 0, 1, 1, 0, 0, 0, 0]
    assert [lib.ggnn_gcn_image_bytes(d) > 0 for d in SIZES] == [True, False, True, True, False, False, False, False]


def test_image_and_workspace_bytes(pkg):
    lib = pkg._lib.load()
    assert [lib.ggnn_gcn_panel_image_bytes(d) > 0 for d in SIZES] == [False, False, False, False, True, True, True, False]
    for D in (128, 192, 256):
        # three bf16 planes of the D x D matrix: 6 bytes per weight, in D / 64 panel images
        assert lib.ggnn_gcn_panel_image_bytes(D) == 6 * D * D
        for V, L in ((0, 1), (1000, 4), (12345, 7)):
            assert lib.ggnn_gcn_panel_workspace_bytes(V, D, L) >= L * lib.ggnn_gcn_panel_image_bytes(D) + 2 * V * D * 4
    rows, cap = pkg.ops.gcn_panel_launch_geometry()
    assert rows == 128 and cap > 0


def test_entry_points_validate_without_gpu(pkg):
    lib = pkg._lib.load()
    fake = 16

    def layer(x, V, D, keep=1.0, out=32, s_out=None):
        return lib.ggnn_gcn_panel_layer_f32(x, fake, fake, fake, 4, fake, None, 1, None, 0, 0, keep, out, s_out, V, D, None)

    assert layer(None, 5, 128) == -1                      # null pointer
    assert layer(fake, 5, 100) == -2                      # the panel kernel has no D = 100 ...
    assert layer(fake, 5, 48) == -2                       # ... and no 48
    assert layer(None, 0, 256) == 0                       # V == 0: nothing to do
    assert layer(fake, 5, 192, keep=0.0) == -1            # keep_prob outside (0, 1]
    assert layer(fake, 5, 192, keep=1.5) == -1
    assert layer(fake, -1, 128) == -1
    assert layer(fake, 5, 128, out=fake) == -1            # out aliases x
    assert layer(fake, 5, 128, s_out=fake) == -1          # s_out aliases x
    assert layer(fake, 5, 128, s_out=32) == -1            # s_out aliases out
    assert layer(fake, 5, 128, out=36) == -1              # misaligned
    assert layer(fake, 1 << 22, 256) == -2                # V * D >= 2^30
    assert layer(fake, 1 << 23, 128) == -2
    assert lib.ggnn_gcn_panel_pack_weights_f32(None, 128, 0, fake, None) == -1
    assert lib.ggnn_gcn_panel_pack_weights_f32(fake, 128, 1, None, None) == -1
    assert lib.ggnn_gcn_panel_pack_weights_f32(fake, 100, 0, fake, None) == -2
    assert lib.ggnn_gcn_panel_pack_weights_f32(fake, 48, 0, fake, None) == -2
    W = (pkg.ops.ctypes.c_void_p * 2)(fake, fake)

    def prop(h0, V, D, ws_bytes, out=32):
        return lib.ggnn_gcn_panel_propagate_f32(h0, V, D, 2, fake, fake, fake, 4, W, None, out, fake, ws_bytes, None)

    assert prop(None, 5, 128, 1 << 30) == -1
    assert prop(fake, 5, 100, 1 << 30) == -2
    assert prop(fake, 5, 48, 1 << 30) == -2
    assert prop(None, 0, 256, 0) == 0
    assert prop(fake, 5, 192, 1 << 30, out=fake) == -1    # out aliases h0
    assert prop(fake, 1 << 22, 256, 1 << 40) == -2        # V * D >= 2^30
    assert prop(fake, 5, 128, 16) == -3                   # workspace too small
    assert b"GCN" in lib.ggnn_last_error() or b"workspace" in lib.ggnn_last_error()


@pytest.mark.parametrize("hidden", [128, 100])
def test_cpu_model_with_the_key_constructs(pkg, hidden):
    ms = pkg.synthetic_qm9(10, seed=1)
    params = {"hidden_size": hidden, "num_timesteps": 2, "random_seed": 7, "gcn_panel_layers": True}
    m = pkg.SparseGCNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": params})
    assert m.params["gcn_panel_layers"] is True
    assert "gcn_panel_layers" not in type(m).default_params()
    assert m.gcn_panel_route() is False                   # no CUDA/HIP device: the key changes nothing
