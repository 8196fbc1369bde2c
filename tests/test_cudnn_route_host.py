"""CPU tests of the compacted CudnnCompatibleGRUCell route (params['compact_cudnn_gru']): the header and the ctypes table agree on
the new entry points, ggnn_cudnn_gru_fused_supported names the supported set and every other entry point agrees with it, the launcher
and the driver refuse bad arguments with an error code before anything is launched, and SparseGGNNChemModel.cudnn_route() says no
wherever the route does not apply."""
import ctypes
import os
import re

import pytest
import torch

NEW_SYMBOLS = ("ggnn_cudnn_gru_fused_supported", "ggnn_cudnn_gru_packed_bytes", "ggnn_cudnn_gru_pack_weights_f32",
               "ggnn_cudnn_gru_fused_launch_geometry", "ggnn_cudnn_gru_packed_f32", "ggnn_sparse_propagate_cudnn_f32",
               "ggnn_sparse_propagate_cudnn_workspace_bytes")
REQUIRED = [(D, nx) for D in (32, 64, 100) for nx in (1, 2, 3)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_text():
    with open(os.path.join(ROOT, "include", "ggnn_hip.h"), encoding="utf-8") as f:
        return f.read()


def _header_args(name):
    """Number of parameters the header declares for `name`."""
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % re.escape(name), text, flags=re.S)
    assert m, "%s is not declared in include/ggnn_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])


def test_header_and_symbol_table_agree(pkg):
    lib = pkg._lib.load()
    for s in NEW_SYMBOLS:
        assert s in pkg._lib.SYMBOLS and hasattr(lib, s), s
        assert _header_args(s) == len(pkg._lib.SYMBOLS[s][1]), s
    assert lib.ggnn_abi_version() == pkg._lib.ABI_VERSION == 3
    # every symbol's comment cites the reference lines it replaces
    comment = re.search(r"/\* ---- CudnnCompatibleGRUCell in one launch.*?\*/.*?/\* ggnn_sparse_propagate_f32 for graph_rnn_cell = Cudnn.*?\*/",
                        _header_text(), flags=re.S).group(0)
    assert comment.count(":105-108") >= 5 and "131-218" in comment


def _aligned(buf):
    p = ctypes.cast(buf, ctypes.c_void_p)
    return ctypes.c_void_p((p.value + 15) // 16 * 16)


def _at(a, off):
    return ctypes.c_void_p(a.value + off)


def _launch(lib, D, nx, a, b, V=16, h=None, h_out=None, saves=None, packed=None, x1=None):
    """ggnn_cudnn_gru_packed_f32 with distinct, aligned fake pointers (nothing may be launched: every call here must fail or be a
    no-op before the first HIP call)."""
    x = (ctypes.c_void_p * 3)(_at(a, 64), _at(a, 128) if x1 is None else x1, _at(a, 192))
    h = a if h is None else h
    h_out = b if h_out is None else h_out
    packed = _at(a, 256) if packed is None else packed
    sr, su, sc, shc = (None, None, None, None) if saves is None else saves
    return lib.ggnn_cudnn_gru_packed_f32(x, nx, h, packed, _at(a, 320), _at(a, 384), _at(a, 448), h_out, sr, su, sc, shc, V, D, None)


def test_supported_set(pkg):
    lib = pkg._lib.load()
    for D, nx in REQUIRED:
        assert lib.ggnn_cudnn_gru_fused_supported(D, nx) == 1, (D, nx)
    for D, nx in ((48, 1), (128, 1), (64, 0), (64, 4), (32, 0), (32, 4), (100, 0), (100, 4)):
        assert lib.ggnn_cudnn_gru_fused_supported(D, nx) == 0, (D, nx)


def test_every_entry_point_agrees_with_the_predicate(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 1024)()
    a = _aligned(buf)
    b = _at(a, 2048)
    for D in (32, 48, 64, 100, 128):
        for nx in range(5):
            ok = lib.ggnn_cudnn_gru_fused_supported(D, nx)
            assert ok in (0, 1)
            rows, wgs = ctypes.c_int(-1), ctypes.c_int(-1)
            lib.ggnn_cudnn_gru_fused_launch_geometry(D, nx, ctypes.byref(rows), ctypes.byref(wgs))
            if ok:
                # 3 (nx + 1) blocks as exact bf16x3 images: at least 3 x 2 bytes per weight; and two of them (the ring) fit a CU's LDS
                nimg = 3 * (nx + 1)
                nbytes = lib.ggnn_cudnn_gru_packed_bytes(D, nx)
                assert nimg * D * D * 6 <= nbytes and nbytes % nimg == 0 and 2 * (nbytes // nimg) <= 160 * 1024, (D, nx)
                assert rows.value > 0 and rows.value % 16 == 0 and wgs.value > 0, (D, nx)
                assert pkg.ops.cudnn_gru_fused_supported(D, nx)
                assert pkg.ops.cudnn_gru_fused_launch_geometry(D, nx) == (rows.value, wgs.value)
            else:
                assert lib.ggnn_cudnn_gru_packed_bytes(D, nx) == 0, (D, nx)
                assert (rows.value, wgs.value) == (0, 0), (D, nx)
                assert lib.ggnn_cudnn_gru_pack_weights_f32(a, a, a, nx, D, b, None) == -2, (D, nx)
                assert b"supports D = 32, 64, 100 with nx = 1..3" in lib.ggnn_last_error()
                assert _launch(lib, D, nx, a, b) == -2, (D, nx)
                assert b"supports D = 32, 64, 100 with nx = 1..3" in lib.ggnn_last_error()
                assert not pkg.ops.cudnn_gru_fused_supported(D, nx)
                assert pkg.ops.cudnn_gru_fused_launch_geometry(D, nx) == (0, 0)


def test_launcher_refuses_bad_arguments_without_gpu(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 2048)()
    a = _aligned(buf)
    b = _at(a, 2048)
    saves = (_at(b, 64), _at(b, 128), _at(b, 192), _at(b, 256))
    # null pointers
    assert lib.ggnn_cudnn_gru_packed_f32(None, 1, None, None, None, None, None, None, None, None, None, None, 16, 64, None) == -1
    assert b"null" in lib.ggnn_last_error()
    assert _launch(lib, 64, 2, a, b, x1=ctypes.c_void_p(None)) == -1 and b"null" in lib.ggnn_last_error()
    assert lib.ggnn_cudnn_gru_pack_weights_f32(None, None, None, 1, 64, None, None) == -1
    # misalignment: an input, the output, a segment, a save buffer
    assert _launch(lib, 64, 1, a, b, h=_at(a, 4)) == -1 and b"aligned" in lib.ggnn_last_error()
    assert _launch(lib, 64, 1, a, b, h_out=_at(b, 4)) == -1 and b"aligned" in lib.ggnn_last_error()
    assert _launch(lib, 64, 2, a, b, x1=_at(a, 132)) == -1 and b"misaligned" in lib.ggnn_last_error()
    assert _launch(lib, 64, 1, a, b, saves=(saves[0], _at(b, 132), saves[2], saves[3])) == -1 and b"aligned" in lib.ggnn_last_error()
    # aliasing: h_out on h, on a segment; a save buffer on an input, on h_out, on another save buffer
    assert _launch(lib, 64, 1, a, b, h_out=a) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 64, 2, a, b, h_out=_at(a, 128)) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 64, 3, a, b, h_out=_at(a, 192)) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 64, 1, a, b, saves=(a, saves[1], saves[2], saves[3])) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 64, 1, a, b, saves=(saves[0], saves[1], _at(a, 64), saves[3])) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 64, 1, a, b, saves=(saves[0], saves[1], saves[2], b)) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 64, 1, a, b, saves=(saves[0], saves[0], saves[2], saves[3])) == -1 and b"alias" in lib.ggnn_last_error()
    # the save pointers are all null or all given
    for k in range(4):
        part = tuple(None if i == k else s for i, s in enumerate(saves))
        assert _launch(lib, 64, 1, a, b, saves=part) == -1 and b"all null or all given" in lib.ggnn_last_error()
        one = tuple(s if i == k else None for i, s in enumerate(saves))
        assert _launch(lib, 64, 1, a, b, saves=one) == -1 and b"all null or all given" in lib.ggnn_last_error()
    # 32-bit byte offsets: V * D >= 2^30
    assert _launch(lib, 64, 1, a, b, V=(1 << 30) // 64) == -2 and b"2^30" in lib.ggnn_last_error()
    assert _launch(lib, 100, 1, a, b, V=(1 << 30) // 100 + 1) == -2
    assert _launch(lib, 64, 1, a, b, V=-1) == -1
    # V == 0 is a no-op
    assert _launch(lib, 64, 1, a, b, V=0) == 0
    assert lib.ggnn_cudnn_gru_packed_f32(None, 3, None, None, None, None, None, None, None, None, None, None, 0, 100, None) == 0


def test_driver_refuses_bad_arguments_without_gpu(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 64)()
    a = _aligned(buf)
    i32 = (ctypes.c_int32 * 2)(1, 1)
    res = (ctypes.c_int32 * 2)(0, 0)
    ptrs = (ctypes.c_void_p * 1)(a)
    off = (ctypes.c_int64 * 5)(0, 2, 2, 3, 5)
    drv = lib.ggnn_sparse_propagate_cudnn_f32

    def call(pair_node, type_off, ws_bytes, bch=ptrs, V=10):
        return drv(a, V, 100, 4, a, a, pair_node, type_off, a, 1, 1, i32, res, res, ptrs, None, None, ptrs, ptrs, ptrs, ptrs, ptrs,
                   bch, None, None, ptrs, a, ws_bytes, None)
    assert call(None, None, 1 << 30) == -1 and b"compacted" in lib.ggnn_last_error()
    assert call(a, None, 1 << 30) == -1 and b"compacted" in lib.ggnn_last_error()
    assert call(a, off, 1 << 30, bch=None) == -1 and b"Cudnn GRU weights" in lib.ggnn_last_error()
    need = lib.ggnn_sparse_propagate_cudnn_workspace_bytes(10, 100, 4, 5)
    # the composed cell's workspace (layers without packed images) comes on top of the GRU / RNN drivers'
    assert need >= lib.ggnn_sparse_propagate_workspace_bytes(10, 100, 4, 5) + lib.ggnn_cudnn_gru_workspace_bytes(10, 100) > 0
    assert call(a, off, need - 1) == -3 and b"workspace too small" in lib.ggnn_last_error()
    assert call(a, off, 0) == -3
    assert call(a, off, 0, V=0) == 0
    assert lib.ggnn_sparse_propagate_cudnn_workspace_bytes(-1, 100, 4, 5) == 0


def _cpu_model(pkg, **config):
    ms = pkg.synthetic_qm9(10, mean_nodes=6, seed=3)
    return pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": config})


def test_cudnn_route_predicate(pkg):
    assert "compact_cudnn_gru" not in pkg.SparseGGNNChemModel.default_params()
    on = dict(graph_rnn_cell="CudnnCompatibleGRUCell", compact_cudnn_gru=True)
    for config in (dict(graph_rnn_cell="CudnnCompatibleGRUCell"),                      # without the key
                   dict(compact_cudnn_gru=True),                                       # the key on the GRU
                   dict(compact_cudnn_gru=True, graph_rnn_cell="RNN"),                 # the key on the RNN cell
                   dict(on, use_propagation_attention=True),                           # attention + Cudnn cell keeps its route
                   dict(graph_rnn_cell="CudnnCompatibleGRUCell", compact_rnn=True, compact_attention=True),   # the other cells' keys
                   dict(on, hidden_size=96), dict(on, hidden_size=300)):               # no compacted transform at these widths
        model = _cpu_model(pkg, **config)
        assert not model.cudnn_route(), config
        model.device = torch.device("cuda:0")               # (the predicate's device condition alone; nothing runs)
        assert not model.cudnn_route(), config
    for hidden in (32, 64, 84, 100, 128, 192, 256):
        for extra in (dict(), dict(use_edge_bias=True, use_edge_msg_avg_aggregation=False)):
            model = _cpu_model(pkg, hidden_size=hidden, **on, **extra)
            assert not model.cudnn_route(), "a CPU model has no HIP route"
            model.device = torch.device("cuda:0")
            assert model.cudnn_route(), hidden
            assert not model.attention_route() and not model.rnn_route()


def test_cpu_model_keeps_todays_behaviour(pkg):
    """The hot path has no CPU implementation with or without the key, and says so the same way."""
    errors = []
    for key in (True, False):
        config = dict(graph_rnn_cell="CudnnCompatibleGRUCell", pack_on_device=False)
        if key:
            config["compact_cudnn_gru"] = True
        model = _cpu_model(pkg, **config)
        assert not model.cudnn_route()
        with pytest.raises(TypeError) as e:
            feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
            with torch.no_grad():
                model.forward_batch(feed)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "no CPU implementation" in errors[0]
