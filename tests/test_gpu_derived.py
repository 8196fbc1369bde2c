"""The version-keyed cache (derived.py) under the stage images, the transposed and the dropped-out weights, on the GPU: every kind of
image equals what the C packer writes, a new weight version repacks, a strided view is refused, and the per-layer fallback of the
native training step -- the route that uses PACKED.edge_t and backward.masked -- trains the same weights as the fused preparation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, T = 32, 2


def _rand(cuda, seed, *shape):
    return ((torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) - 0.5) * 0.4).to(cuda)


def _kinds(pkg, cuda):
    """name -> (source tensors, cached call on a PackedWeights P, direct C pack into `out`, image floats)."""
    lib, st = pkg._lib.load(), lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    W = _rand(cuda, 1, T, D, D)
    Wg1, Wc1 = _rand(cuda, 2, 2 * D, 2 * D), _rand(cuda, 3, 2 * D, D)           # nx = 1
    Wg2, Wc2 = _rand(cuda, 4, 3 * D, 2 * D), _rand(cuda, 5, 3 * D, D)           # nx = 2
    Wr = _rand(cuda, 6, 2 * D, D)
    edge_n = lib.ggnn_msg_transform_compact_workspace_bytes(D, T) // 4
    kinds = {}
    for fmt in (pkg.formats.F16X2, pkg.formats.BF16X3):
        kinds["gru/%d" % fmt] = ((Wg2, Wc2), lambda P, fmt=fmt: P.gru(Wg2, Wc2, 2, D, fmt),
                                 lambda out, fmt=fmt: lib.ggnn_gru_pack_weights_f32(p(Wg2), p(Wc2), 2, D, fmt, p(out), st()),
                                 lib.ggnn_gru_packed_bytes(D, 2) // 4)
        kinds["edge/%d" % fmt] = ((W,), lambda P, fmt=fmt: P.edge(W, fmt),
                                  lambda out, fmt=fmt: lib.ggnn_edge_weights_pack_f32(p(W), T, D, fmt, p(out), st()), edge_n)

    def pack_edge_t(out):
        Wt = W.transpose(1, 2).contiguous()
        return lib.ggnn_edge_weights_pack_f32(p(Wt), T, D, pkg.formats.BF16X3, p(out), st())
    kinds["edge_t"] = ((W,), lambda P: P.edge_t(W), pack_edge_t, edge_n)
    kinds["dense_edge"] = ((W,), lambda P: P.dense_edge(W), lambda out: lib.ggnn_dense_edge_pack_f32(p(W), T, D, p(out), st()),
                           lib.ggnn_dense_edge_packed_bytes(D, T) // 4)
    kinds["dense_gru"] = ((Wg1, Wc1), lambda P: P.dense_gru(Wg1, Wc1, D),
                          lambda out: lib.ggnn_dense_gru_pack_f32(p(Wg1), p(Wc1), D, p(out), st()), lib.ggnn_dense_gru_packed_bytes(D) // 4)
    kinds["gru_bwd"] = ((Wg1, Wc1), lambda P: P.gru_bwd(Wg1, Wc1, 1, D),
                        lambda out: lib.ggnn_gru_bwd_fused_f32(None, None, None, None, None, p(Wg1), p(Wc1), p(out), None, None, None,
                                                               None, None, None, 0, 0, 1, 0, D, 0, st()),
                        lib.ggnn_gru_bwd_packed_bytes(D, 1) // 4)
    kinds["rnn"] = ((Wr,), lambda P: P.rnn(Wr, 1, D), lambda out: lib.ggnn_rnn_pack_weights_f32(p(Wr), 1, D, p(out), st()),
                    max(lib.ggnn_rnn_packed_bytes(D, 1) // 4, 4))
    kinds["dense_bwd"] = ((W, Wg1, Wc1), lambda P: P.dense_bwd(W, Wg1, Wc1),
                          lambda out: lib.ggnn_dense_bwd_pack_f32(p(W), p(Wg1), p(Wc1), T, D, p(out), st()),
                          lib.ggnn_dense_bwd_packed_bytes(D, T) // 4)
    return kinds


def _direct(pkg, cuda, pack, n):
    """What the C packer writes, as int32 bits, and WHERE it writes: an image buffer may end in alignment slack that no packer
    touches, so the pack runs into two buffers of different fill and the words that agree are the written ones."""
    a, b = torch.full((n,), 1.0, device=cuda), torch.full((n,), 2.0, device=cuda)
    pkg._lib.check(pack(a))
    pkg._lib.check(pack(b))
    a, b = a.view(torch.int32), b.view(torch.int32)
    written = a == b
    assert bool(written.any())
    return a[written], written


KINDS = ["gru/2", "gru/3", "edge/2", "edge/3", "edge_t", "dense_edge", "dense_gru", "gru_bwd", "rnn", "dense_bwd"]


@pytest.mark.parametrize("kind", KINDS)
def test_cached_image_equals_the_c_packer_and_follows_the_version(pkg, cuda, kind):
    sources, cached, pack, n = _kinds(pkg, cuda)[kind]
    assert n > 0
    P = pkg.ops.PACKED
    want, written = _direct(pkg, cuda, pack, n)
    img = cached(P)
    assert img.numel() == n and torch.equal(img.view(torch.int32)[written], want)
    assert cached(P).data_ptr() == img.data_ptr()                               # a hit: the same image
    if kind == "dense_bwd":
        assert torch.equal(pkg.ops.dense_bwd_pack(*sources).view(torch.int32)[written], want)
    for s in sources:
        s.mul_(2)                                                               # a new version: a stale hit fails below
    want2, written2 = _direct(pkg, cuda, pack, n)
    assert torch.equal(written2, written) and not torch.equal(want2, want)
    img2 = cached(P)
    assert torch.equal(img2.view(torch.int32)[written], want2)
    assert cached(P).data_ptr() == img2.data_ptr()


def test_edge_t_is_the_image_of_the_transposed_copy(pkg, cuda):
    W = _rand(cuda, 7, T, D, D)
    a = pkg.ops.PACKED.edge_t(W)
    b = pkg.ops.PackedWeights().edge(W.transpose(1, 2).contiguous())
    n = a.numel() - 256 // 4                                                    # (the edge buffers end in 256 bytes of alignment slack)
    assert a.numel() == b.numel() and torch.equal(a[:n], b[:n])


def test_strided_view_is_refused_even_after_its_sibling_was_cached(pkg, cuda, monkeypatch):
    W = _rand(cuda, 8, T, D, D)
    pkg.ops.PACKED.edge(W)
    launched = []
    monkeypatch.setattr(pkg._lib.load(), "ggnn_edge_weights_pack_f32", lambda *a: launched.append(a) or 0)
    with pytest.raises(ValueError, match="must be contiguous"):
        pkg.ops.PACKED.edge(W.transpose(1, 2))
    with pytest.raises(ValueError, match="must be contiguous"):
        pkg.ops.PACKED.edge_t(W.transpose(1, 2))
    assert not launched                                                         # refused before the packer: no kernel launch


def test_masked_weights(pkg, cuda):
    b, ops = pkg.backward, pkg.ops
    var = _rand(cuda, 9, T * D, D)
    m = b.masked(var.view(T, D, D), 0.8, 123)
    assert torch.equal(m, ops.dropout(var.view(T, D, D).contiguous(), 0.8, 123))
    assert b.masked(var.view(T, D, D), 0.8, 123) is m                           # shared by the views of the variable
    m2 = b.masked(var.view(T, D, D), 0.8, 124)
    assert m2 is not m and torch.equal(m2, ops.dropout(var.view(T, D, D).contiguous(), 0.8, 124)) and not torch.equal(m2, m)
    var.add_(1)
    m3 = b.masked(var.view(T, D, D), 0.8, 124)
    assert m3 is not m2 and torch.equal(m3, ops.dropout(var.view(T, D, D).contiguous(), 0.8, 124))


@pytest.mark.parametrize("keep", [1.0, 0.8])
def test_per_layer_fallback_of_the_native_step_trains_the_same_weights(pkg, oracle, cuda, monkeypatch, keep):
    """Three native training steps with the step's images from the per-layer path (backward.masked, PACKED.edge / edge_t / gru /
    gru_bwd) against three with ggnn_sparse_train_prepare_f32: test_fused_weight_preparation_equals_per_layer_packing holds the two
    image sets equal bit for bit, so every trained variable is too.  Afterwards no image of a dead source is left behind."""
    trained, asked = [], []
    edge_t = pkg.ops.PACKED.edge_t
    monkeypatch.setattr(pkg.ops.PACKED, "edge_t", lambda W, *a: asked.append(fused) or edge_t(W, *a))
    for fused in (True, False):
        monkeypatch.setattr(pkg.train_native, "USE_FUSED_PREPARE", fused)
        ms = pkg.synthetic_qm9(30, mean_nodes=8, seed=1)
        model = pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms})
        model.set_graph_weights(oracle.make_sparse_layers(np.random.default_rng(1), model.params, model.num_edge_types, random_bias=True))
        feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=False))))
        feed["edge_weight_dropout_keep_prob"] = keep
        assert pkg.train_native.eligible(model, feed)
        losses = [float(model.train_batch(feed)) for _ in range(3)]
        assert np.all(np.isfinite(losses))
        trained.append((losses, {k: v.detach().clone() for k, v in model.trainable_variables.items()}))
    (l1, w1), (l0, w0) = trained
    assert set(w1) == set(w0)
    for k in w0:
        assert torch.equal(w1[k], w0[k]), k
    L = len(model.params["layer_timesteps"])
    assert asked == [False] * (3 * L)                                           # (the fallback ran: one transposed image per layer and step)
    assert all(ref() is not None for entry in pkg.ops.PACKED._images._t.values() for ref in entry[0])
