"""Host side of the column-panel GRU backward (hidden sizes 128 / 192 / 256 behind the fused-backward entry points): which sizes
report a single-launch backward, how large their packed weight images are, and the argument checks of the two launch calls that
return before anything touches a device.  No GPU needed."""
import ctypes

INVALID, UNSUPPORTED = -1, -2


def _aligned(n_floats=64):
    buf = (ctypes.c_float * (n_floats + 4))()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    return buf, ctypes.c_void_p((p + 15) // 16 * 16)


def test_fused_backward_sizes(pkg):
    lib = pkg._lib.load()
    assert [lib.ggnn_gru_bwd_is_fused(D) for D in (32, 64, 100, 128, 192, 256, 200, 96)] == [1, 1, 1, 1, 1, 1, 0, 0]
    # the two-call native step keeps its own width test: no gather-fused forward GRU at the panel sizes
    assert [lib.ggnn_gru_is_fused(D) for D in (128, 192, 256)] == [2, 2, 2]


def test_product_library_reads_no_experiment_switches_of_the_training_kernels(pkg):
    """The fused GRU backward launches one kernel per matrix path, and its clock stamps and the weight-gradient product's are
    compiled in only in variant libraries (tools/variant_lib.sh): the product library holds none of the variables' names.
    (GGNN_DG_TPTR / GGNN_DGB_TPTR are not in the list: the graph-resident dense kernels keep their run-time stamps, because
    compiling them out moved two of those kernels across an occupancy step, profiles/README.md.)"""
    pkg._lib.load()
    assert pkg._lib.LIB_PATH.endswith("libggnn_hip.so"), pkg._lib.LIB_PATH
    with open(pkg._lib.LIB_PATH, "rb") as f:
        blob = f.read()
    names = (b"GGNN_BWD_FORM", b"GGNN_BWD_ALIAS", b"GGNN_BWD_TPTR", b"GGNN_XTY_TPTR")
    assert [n for n in names if n in blob] == []
    assert b"GGNN_MATRIX" in blob                                              # (a variable the library does read: the search finds names)


def test_packed_bytes_of_the_panel_sizes(pkg):
    """3 (nx + 1) transposed D x D blocks, each as D / 64 panel images: three bf16 planes (6 bytes per weight) under the split matrix
    path, f32 (4 bytes) otherwise."""
    lib = pkg._lib.load()
    per_weight = 6 if lib.ggnn_matrix_path_is_split() else 4
    for D in (128, 192, 256):
        for nx in (1, 2, 3):
            n = lib.ggnn_gru_bwd_packed_bytes(D, nx)
            assert n > 0 and n % 16 == 0
            assert n == 3 * (nx + 1) * D * D * per_weight, (D, nx, n)
    assert lib.ggnn_gru_bwd_packed_bytes(200, 1) == 0 and lib.ggnn_gru_bwd_packed_bytes(96, 2) == 0
    assert lib.ggnn_gru_bwd_packed_bytes(100, 1) > 0                          # (the whole-block sizes keep theirs)


def test_launch_argument_checks_without_device(pkg):
    lib = pkg._lib.load()
    keep, p = _aligned()
    D, T = 256, 4
    dx = (ctypes.c_void_p * 3)(p, p, p)

    def plain(g=p, h=p, packed=p, dxs=dx, nx=1, V=16, D=D, act=0, nin=p):
        return lib.ggnn_gru_bwd_fused_f32(g, h, p, p, p, None, None, packed, p, p, p, p, dxs, nin, T, 1, nx, V, D, act, None)

    def gather(g=p, gz=p, heads=p, packed=p, nx=1, V=16, D=D):
        return lib.ggnn_gru_bwd_fused_gather_f32(g, gz, heads, p, p, p, p, packed, p, p, p, p, dx, p, T, 1, nx, V, D, 0, None)

    # null pointers
    assert plain(packed=None) == INVALID and b"packed" in lib.ggnn_last_error()
    assert plain(h=None) == INVALID and b"null" in lib.ggnn_last_error()
    assert plain(nin=None) == INVALID                                          # mean aggregation needs the in-degrees
    assert plain(dxs=(ctypes.c_void_p * 3)(p, None, p), nx=2) == INVALID and b"dx[1]" in lib.ggnn_last_error()
    assert gather(gz=None) == INVALID and gather(heads=None) == INVALID and gather(g=None) == INVALID
    # nx outside 1..3, unknown activation, negative V
    for nx in (0, 4):
        assert plain(nx=nx) == INVALID and gather(nx=nx) == INVALID
    assert plain(act=7) == INVALID and plain(V=-1) == INVALID
    # 32-bit byte offsets: V * 2D must stay below 2^30
    V_big = (1 << 30) // (2 * D)
    assert plain(V=V_big) == UNSUPPORTED and b"2^30" in lib.ggnn_last_error()
    assert gather(V=V_big) == UNSUPPORTED and b"2^30" in lib.ggnn_last_error()
    assert plain(V=(1 << 30) // (2 * 128), D=128) == UNSUPPORTED
    # sizes outside both kernels' sets: unsupported, and the message says which sizes are
    assert plain(D=200) == UNSUPPORTED
    msg = lib.ggnn_last_error()
    assert all(s in msg for s in (b"200", b"100", b"128", b"192", b"256")), msg
    assert gather(D=96) == UNSUPPORTED
    # V == 0 with packed images in place: a no-op
    assert plain(V=0) == 0 and gather(V=0) == 0
    del keep
