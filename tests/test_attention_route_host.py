"""CPU tests of the compacted propagation-attention route (params['compact_attention']): the library exports its three entry
points, their launchers refuse bad arguments with an error code and a message before anything is launched, the slot -> compact
row addressing (active (source node, type) pairs, type-major / node-ascending) reproduces dense-row addressing bit for bit in a
NumPy restatement, and SparseGGNNChemModel.attention_route() says no wherever the route does not apply."""
import ctypes

import numpy as np
import pytest
import torch

import variant_kernel_ref as ref

NEW_SYMBOLS = ("ggnn_gather_segment_sum_attn_compact_f32", "ggnn_attn_bwd_target_compact_f32", "ggnn_sparse_propagate_attn_f32")


def test_library_exports_the_new_symbols(pkg):
    lib = pkg._lib.load()
    for s in NEW_SYMBOLS:
        assert s in pkg._lib.SYMBOLS and hasattr(lib, s), s
    assert lib.ggnn_abi_version() == pkg._lib.ABI_VERSION == 3


def _aligned(buf):
    p = ctypes.cast(buf, ctypes.c_void_p)
    return ctypes.c_void_p((p.value + 15) // 16 * 16)


def test_launchers_refuse_bad_arguments_without_gpu(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 64)()
    a = _aligned(buf)
    fwd, bwd = lib.ggnn_gather_segment_sum_attn_compact_f32, lib.ggnn_attn_bwd_target_compact_f32
    # null pointers
    assert fwd(None, None, None, None, None, None, None, None, 0, None, 10, 100, 4, None) == -1
    assert b"null" in lib.ggnn_last_error()
    assert bwd(None, None, None, None, None, None, None, None, None, None, None, None, 1, 10, 100, 4, None) == -1
    assert b"null" in lib.ggnn_last_error()
    # D % 4
    assert fwd(a, a, a, a, a, a, a, None, 1, a, 10, 6, 4, None) == -1
    assert b"bad sizes" in lib.ggnn_last_error()
    assert bwd(a, a, a, a, a, a, a, a, a, a, a, a, 1, 10, 6, 4, None) == -1
    # D = 260: beyond the widest sub-wave
    assert fwd(a, a, a, a, a, a, a, None, 1, a, 10, 260, 4, None) == -2
    assert b"up to 256" in lib.ggnn_last_error()
    assert bwd(a, a, a, a, a, a, a, a, a, a, a, a, 1, 10, 260, 4, None) == -2
    assert b"up to 256" in lib.ggnn_last_error()
    # mean aggregation without the in-degree table
    assert fwd(a, a, a, a, a, a, None, None, 1, a, 10, 100, 4, None) == -1
    assert b"nin" in lib.ggnn_last_error()
    # V == 0 is a no-op
    assert fwd(None, None, None, None, None, None, None, None, 0, None, 0, 100, 4, None) == 0
    assert bwd(None, None, None, None, None, None, None, None, None, None, None, None, 1, 0, 100, 4, None) == 0
    # the driver: no attention factors, no compacted form, D = 260
    i32 = (ctypes.c_int32 * 2)(1, 1)
    ptrs = (ctypes.c_void_p * 1)(a)
    off = (ctypes.c_int64 * 5)(0, 0, 0, 0, 0)
    drv = lib.ggnn_sparse_propagate_attn_f32

    def call(D, pair_node, type_off, attn):
        return drv(a, 10, D, 4, a, a, pair_node, type_off, a, 1, 1, i32, i32, i32, ptrs, None, None, ptrs, ptrs, ptrs, ptrs, None,
                   None, None, 0, 0, ptrs, a, 0, a, attn, None)
    assert call(100, a, off, None) == -1 and b"attn_factors" in lib.ggnn_last_error()
    assert call(260, a, off, ptrs) == -2 and b"up to 256" in lib.ggnn_last_error()
    assert call(100, None, None, ptrs) == -1 and b"compacted" in lib.ggnn_last_error()


def _compact_rows(adj, V, T):
    """NumPy restatement of ops.build_compact_sources: the active (source node, type) pairs, type-major / node-ascending ->
    (pair_node [R], type_of_row [R], compact row of every message, by message id)."""
    src, dst, typ = ref.messages(adj)
    active = np.zeros((T, V), bool)
    active[typ, src] = True
    row_of_pair = np.full((T, V), -1, np.int64)
    t_idx, v_idx = np.nonzero(active)                      # row-major over [T, V]: type-major, node ascending
    row_of_pair[t_idx, v_idx] = np.arange(len(t_idx))
    return v_idx, t_idx, row_of_pair[typ, src]


@pytest.mark.parametrize("V,T", [(1, 1), (17, 3), (33, 4)])
def test_compact_row_addressing_equals_dense_row_addressing(V, T):
    D = 100
    c = ref.attn_inputs(D, V, T, ref.seed_of("attn", D, V, T))
    Hrows = ref.transform_rows(c["h"], c["W"], np.float32)
    pair_node, type_of_row, row_of_msg = _compact_rows(c["adj"], V, T)
    src, dst, typ = ref.messages(c["adj"])
    R = len(pair_node)
    assert (row_of_msg >= 0).all() and R <= min(len(src), V * T) and R < len(src)      # (the tripled pair, the hub: shared rows)
    assert (np.diff(type_of_row) >= 0).all() and all((np.diff(pair_node[type_of_row == t]) > 0).all() for t in range(T))
    Hc = Hrows[pair_node * T + type_of_row].copy()
    np.testing.assert_array_equal(Hc[row_of_msg], Hrows[src * T + typ])
    if c["info"]["empty_type"] is not None:
        assert not (type_of_row == c["info"]["empty_type"]).any()
    for bias_on, use_avg in ref.ATTN_SWITCHES:
        bias = c["bias"] if bias_on else None
        want = ref.attn_forward(c["h"], Hrows, c["adj"], c["factors"], c["nin"], bias, use_avg, dt=np.float32)
        # the same float32 formula reading the messages through the compact rows; every dense row outside them is poisoned
        *_, a = ref._softmax(c["h"], c["adj"], c["factors"], np.float32)
        got = np.zeros((V, D), np.float32)
        np.add.at(got, dst, a[:, None] * Hc[row_of_msg])
        if bias_on:
            got = got + c["nin"] @ c["bias"]
        if use_avg:
            got = got / (c["nin"].sum(-1, keepdims=True, dtype=np.float32) + np.float32(ref.SMALL))
        assert got.dtype == want.dtype == np.float32
        np.testing.assert_array_equal(got, want)
        poisoned = np.full_like(Hrows, np.nan)
        poisoned[pair_node * T + type_of_row] = Hc
        np.testing.assert_array_equal(ref.attn_forward(c["h"], poisoned, c["adj"], c["factors"], c["nin"], bias, use_avg, dt=np.float32), want)


def _cpu_model(pkg, **config):
    ms = pkg.synthetic_qm9(10, mean_nodes=6, seed=3)
    return pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": config})


def test_attention_route_predicate(pkg):
    on = dict(use_propagation_attention=True, compact_attention=True)
    for config in (dict(use_propagation_attention=True),                           # without the key
                   dict(on, graph_rnn_cell="RNN"), dict(on, graph_rnn_cell="CudnnCompatibleGRUCell"),
                   dict(on, hidden_size=96), dict(on, hidden_size=160), dict(on, hidden_size=200), dict(on, hidden_size=300),
                   dict(compact_attention=True)):                                  # the key without attention
        model = _cpu_model(pkg, **config)
        assert not model.attention_route(), config
        model.device = torch.device("cuda:0")               # (the predicate's device condition alone; nothing runs)
        assert not model.attention_route(), config
    assert "compact_attention" not in pkg.SparseGGNNChemModel.default_params()
    for hidden in (32, 64, 84, 100, 128, 192, 256):
        model = _cpu_model(pkg, hidden_size=hidden, **on)
        assert not model.attention_route(), "a CPU model has no HIP route"
        model.device = torch.device("cuda:0")
        assert model.attention_route(), hidden


def test_cpu_model_keeps_todays_behaviour(pkg):
    """A CPU-device model can be built; the hot path has no CPU implementation with or without the key, and says so the same way."""
    errors = []
    for key in (True, False):
        config = dict(use_propagation_attention=True, pack_on_device=False)
        if key:
            config["compact_attention"] = True
        model = _cpu_model(pkg, **config)
        assert not model.attention_route()
        with pytest.raises(TypeError) as e:
            feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
            with torch.no_grad():
                model.forward_batch(feed)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "no CPU implementation" in errors[0]
