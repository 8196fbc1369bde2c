"""CPU tests of the compacted BasicRNNCell route (params['compact_rnn'], the R-GCN configuration of the sparse GGNN): the header
and the ctypes table agree on the new entry points, ggnn_rnn_fused_supported names the supported set and every other entry point
agrees with it, the launchers refuse bad arguments with an error code before anything is launched, and
SparseGGNNChemModel.rnn_route() says no wherever the route does not apply."""
import ctypes
import os
import re

import pytest
import torch

NEW_SYMBOLS = ("ggnn_rnn_fused_supported", "ggnn_rnn_packed_bytes", "ggnn_rnn_pack_weights_f32", "ggnn_rnn_fused_launch_geometry",
               "ggnn_rnn_packed_gather_f32", "ggnn_sparse_propagate_rnn_f32")
REQUIRED = [(32, 1), (32, 2), (32, 3), (64, 1), (64, 2), (64, 3), (100, 1)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_args(name):
    """Number of parameters the header declares for `name`."""
    with open(os.path.join(ROOT, "include", "ggnn_hip.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % re.escape(name), text, flags=re.S)
    assert m, "%s is not declared in include/ggnn_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])


def test_header_and_symbol_table_agree(pkg):
    lib = pkg._lib.load()
    for s in NEW_SYMBOLS:
        assert s in pkg._lib.SYMBOLS and hasattr(lib, s), s
        assert _header_args(s) == len(pkg._lib.SYMBOLS[s][1]), s
    assert lib.ggnn_abi_version() == pkg._lib.ABI_VERSION == 3


def _aligned(buf):
    p = ctypes.cast(buf, ctypes.c_void_p)
    return ctypes.c_void_p((p.value + 15) // 16 * 16)


def _launch(lib, D, nx, a, b, V=16, act=1, h=None, h_out=None, save=None, packed=None):
    """ggnn_rnn_packed_gather_f32 with distinct, aligned fake pointers (nothing may be launched: every call here must fail or be a
    no-op before the first HIP call)."""
    x = (ctypes.c_void_p * 2)(ctypes.c_void_p(a.value + 64), ctypes.c_void_p(a.value + 128))
    h = a if h is None else h
    h_out = b if h_out is None else h_out
    packed = ctypes.c_void_p(a.value + 192) if packed is None else packed
    return lib.ggnn_rnn_packed_gather_f32(x, nx, h, packed, ctypes.c_void_p(a.value + 256), h_out, ctypes.c_void_p(a.value + 320), 8,
                                          ctypes.c_void_p(a.value + 384), ctypes.c_void_p(a.value + 448), 8,
                                          ctypes.c_void_p(a.value + 512), 4, 1, save, V, D, act, None)


def test_supported_set(pkg):
    lib = pkg._lib.load()
    for D, nx in REQUIRED:
        assert lib.ggnn_rnn_fused_supported(D, nx) == 1, (D, nx)
    for D, nx in ((48, 1), (128, 1), (64, 0), (64, 4), (32, 0), (32, 4), (100, 0), (100, 4)):
        assert lib.ggnn_rnn_fused_supported(D, nx) == 0, (D, nx)


def test_every_entry_point_agrees_with_the_predicate(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 1024)()
    a = _aligned(buf)
    b = ctypes.c_void_p(a.value + 2048)
    for D in (32, 48, 64, 100, 128):
        for nx in range(5):
            ok = lib.ggnn_rnn_fused_supported(D, nx)
            assert ok in (0, 1)
            rows, wgs = ctypes.c_int(-1), ctypes.c_int(-1)
            lib.ggnn_rnn_fused_launch_geometry(D, nx, ctypes.byref(rows), ctypes.byref(wgs))
            if ok:
                # (the weight blocks as exact bf16x3 images: at least 3 x 2 bytes per weight, at most what a CU's LDS holds)
                assert (nx + 1) * D * D * 6 <= lib.ggnn_rnn_packed_bytes(D, nx) <= 160 * 1024, (D, nx)
                assert rows.value > 0 and rows.value % 16 == 0 and wgs.value > 0, (D, nx)
                assert pkg.ops.rnn_fused_supported(D, nx)
            else:
                assert lib.ggnn_rnn_packed_bytes(D, nx) == 0, (D, nx)
                assert (rows.value, wgs.value) == (0, 0), (D, nx)
                assert lib.ggnn_rnn_pack_weights_f32(a, nx, D, b, None) == -2, (D, nx)
                assert b"fused RNN cell supports" in lib.ggnn_last_error()
                assert _launch(lib, D, nx, a, b) == -2, (D, nx)
                assert not pkg.ops.rnn_fused_supported(D, nx)


def test_launchers_refuse_bad_arguments_without_gpu(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 1024)()
    a = _aligned(buf)
    b = ctypes.c_void_p(a.value + 2048)
    # null pointers
    assert lib.ggnn_rnn_packed_gather_f32(None, 1, None, None, None, None, None, 8, None, None, 8, None, 4, 1, None, 16, 64, 1, None) == -1
    assert b"null" in lib.ggnn_last_error()
    assert lib.ggnn_rnn_pack_weights_f32(None, 1, 64, None, None) == -1
    # misalignment
    assert _launch(lib, 64, 1, a, b, h_out=ctypes.c_void_p(b.value + 4)) == -1 and b"aligned" in lib.ggnn_last_error()
    # aliasing: h_out on h, on a residual segment, on save_incoming; save_incoming on an input
    assert _launch(lib, 64, 1, a, b, h_out=a) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 64, 2, a, b, h_out=ctypes.c_void_p(a.value + 64)) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 64, 1, a, b, save=b) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 64, 1, a, b, save=a) == -1 and b"alias" in lib.ggnn_last_error()
    # unknown activation
    assert _launch(lib, 64, 1, a, b, act=2) == -1 and b"activation" in lib.ggnn_last_error()
    assert _launch(lib, 64, 1, a, b, act=-1) == -1
    # 32-bit byte offsets: V * D >= 2^30
    assert _launch(lib, 64, 1, a, b, V=(1 << 30) // 64) == -2 and b"2^30" in lib.ggnn_last_error()
    assert _launch(lib, 100, 1, a, b, V=(1 << 30) // 100 + 1) == -2
    # V == 0 is a no-op
    assert _launch(lib, 64, 1, a, b, V=0) == 0
    assert lib.ggnn_rnn_packed_gather_f32(None, 1, None, None, None, None, None, 0, None, None, 0, None, 4, 0, None, 0, 100, 0, None) == 0


def test_driver_refuses_bad_arguments_without_gpu(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 64)()
    a = _aligned(buf)
    i32 = (ctypes.c_int32 * 2)(1, 1)
    res = (ctypes.c_int32 * 2)(0, 0)
    ptrs = (ctypes.c_void_p * 1)(a)
    off = (ctypes.c_int64 * 5)(0, 2, 2, 3, 5)
    drv = lib.ggnn_sparse_propagate_rnn_f32

    def call(pair_node, type_off, ws_bytes, act=1, rnn_b=ptrs):
        return drv(a, 10, 100, 4, a, a, 12, pair_node, type_off, a, 1, 1, i32, res, res, ptrs, None, None, ptrs, rnn_b, None, None,
                   act, 3, ptrs, a, ws_bytes, None)
    assert call(None, None, 1 << 30) == -1 and b"compacted" in lib.ggnn_last_error()
    assert call(a, None, 1 << 30) == -1 and b"compacted" in lib.ggnn_last_error()
    assert call(a, off, 1 << 30, act=5) == -1 and b"activation" in lib.ggnn_last_error()
    assert call(a, off, 1 << 30, rnn_b=None) == -1 and b"RNN weights" in lib.ggnn_last_error()
    need = lib.ggnn_sparse_propagate_workspace_bytes(10, 100, 4, 5)
    assert need > 0
    assert call(a, off, need - 1) == -3 and b"workspace too small" in lib.ggnn_last_error()
    assert call(a, off, 0) == -3


def _cpu_model(pkg, **config):
    ms = pkg.synthetic_qm9(10, mean_nodes=6, seed=3)
    return pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": config})


def test_rnn_route_predicate(pkg):
    assert "compact_rnn" not in pkg.SparseGGNNChemModel.default_params()
    on = dict(graph_rnn_cell="RNN", compact_rnn=True)
    for config in (dict(graph_rnn_cell="RNN"),                                         # without the key
                   dict(compact_rnn=True),                                             # the key on the GRU
                   dict(on, use_propagation_attention=True),                           # attention + RNN keeps its route
                   dict(compact_rnn=True, graph_rnn_cell="CudnnCompatibleGRUCell"),
                   dict(on, hidden_size=96), dict(on, hidden_size=300)):               # no compacted transform at these widths
        model = _cpu_model(pkg, **config)
        assert not model.rnn_route(), config
        model.device = torch.device("cuda:0")               # (the predicate's device condition alone; nothing runs)
        assert not model.rnn_route(), config
    for hidden in (32, 64, 84, 100, 128, 192, 256):
        for extra in (dict(), dict(graph_rnn_activation="ReLU", use_edge_bias=False)):
            model = _cpu_model(pkg, hidden_size=hidden, **on, **extra)
            assert not model.rnn_route(), "a CPU model has no HIP route"
            model.device = torch.device("cuda:0")
            assert model.rnn_route(), hidden
            assert not model.attention_route()


def test_cpu_model_keeps_todays_behaviour(pkg):
    """The hot path has no CPU implementation with or without the key, and says so the same way."""
    errors = []
    for key in (True, False):
        config = dict(graph_rnn_cell="RNN", pack_on_device=False)
        if key:
            config["compact_rnn"] = True
        model = _cpu_model(pkg, **config)
        assert not model.rnn_route()
        with pytest.raises(TypeError) as e:
            feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
            with torch.no_grad():
                model.forward_batch(feed)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "no CPU implementation" in errors[0]
