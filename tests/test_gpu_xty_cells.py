"""Every instantiation of the three weight-gradient product kernels behind ggnn_xty_f32 / ggnn_xty_acc_f32 (xty_kernel,
xty_split_kernel, xty_planes_kernel: csrc/ggnn_bwd_gemm.hip) against X^T dY in float64.

Which instantiation runs depends on the shape and on switches the library reads once per process, so the cases are FOUND, not
listed: ggnn_xty_describe (the launcher's own selection function) is swept on the host and each cell gets the smallest shape that
selects it (tests/xty_cases.py); every test first asserts, through the same query, that its shape selects the cell it is named
after IN THIS PROCESS.  The legs -- default, GGNN_MATRIX=f32, GGNN_XTY_PLANES=0, GGNN_XTY_ROWS=32 -- are this process plus one
child pytest process over this file per other leg (test_other_legs_...); between them they run every instantiation of the table.

Bound, per element: |got - want| <= 4e-7 * (|X|^T |dY|) + 1e-6, the ones row (the bias gradient: an X column of ones) included:
4e-7 * sum |dY| + 1e-6.  tests/test_xty_dispatch_host.py shows that a plain float32 product passes it and that wrong results of
seven kinds fail it.  Every product is also computed twice and must be bit-identical."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import xty_cases as xc
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

LEG = os.environ.get("GGNN_XTY_CELLS_LEG")                 # set for the child processes of test_other_legs_...: the leg's name
REPORT = os.environ.get("GGNN_XTY_CELLS_REPORT")           # a file that receives what ran: {cells: {id: ratio}, families: {name: ratio}}
_leg = xc.LEGS[LEG] if LEG else xc.PROCESS
_ran = {"cells": {}, "families": {}}
LARGE_M = 50001


def _cell_id(cell):
    return "%s-%dr-%dx%d" % (xc.family_name(cell), cell[2], cell[3], cell[4])


_cache = []


def _found():
    """({cell: smallest shape}, {family: (cell, smallest shape with the ones row)}) of this process's leg, swept once."""
    if not _cache:
        import importlib
        lib = importlib.import_module(PKG)._lib.load()
        _cache.append((xc.sweep(lib, _leg)[0], xc.family_shapes(xc.sweep_with_ones(lib, _leg))))
    return _cache[0]


def pytest_generate_tests(metafunc):
    want = [n for n in ("cell_case", "family_case", "gathered_case") if n in metafunc.fixturenames]
    if not want:
        return
    try:
        cells, families = _found()
    except Exception as e:                                  # (no library: the tests fail with the reason, the collection goes on)
        for n in want:
            metafunc.parametrize(n, [e], ids=["library-not-loaded"])
        return
    if "cell_case" in want:
        items = sorted(cells.items())
        metafunc.parametrize("cell_case", items, ids=[_cell_id(c) for c, _ in items])
    if "family_case" in want:
        items = sorted(families.items())
        metafunc.parametrize("family_case", [v for _, v in items], ids=[n for n, _ in items])
    if "gathered_case" in want:
        metafunc.parametrize("gathered_case", [families.get("f32-gathered")], ids=["f32-gathered"])


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        with open(REPORT, "w") as f:
            json.dump(_ran, f, indent=1, sort_keys=True)


def _selects(lib, cell, shape):
    """The process's own selection (all switches at 'this process') is the cell the case was found for."""
    if isinstance(cell, Exception):
        raise cell
    rc, got, geom = xc.describe(lib, *shape)
    assert rc == 0 and got == cell, (shape, cell, got, lib.ggnn_last_error())
    return geom


def _device(c, cuda):
    xw, yw = torch.from_numpy(c.xwide).to(cuda), torch.from_numpy(c.ywide).to(cuda)
    segs = [xw[:, 4 + s * c.Dseg:4 + (s + 1) * c.Dseg] for s in range(c.nseg)]
    rows = None if c.x_rows is None else torch.from_numpy(c.x_rows).to(cuda)
    return segs, yw[:, 4:4 + c.N], rows


def _product(pkg, cuda, c):
    """The product, computed twice (bit-identical), on the host.  A missed bound lets the session go on; an ERROR of the library
    or the runtime ends it here (pytest.exit), so that nothing more is started on a GPU that may have faulted -- the leg's parent
    sees the exit status and starts no further leg."""
    try:
        segs, dy, rows = _device(c, cuda)
        got = pkg.ops.xty(segs, dy, x_rows=rows, row_off=c.row_off, ones_row=bool(c.ones))
        again = pkg.ops.xty(segs, dy, x_rows=rows, row_off=c.row_off, ones_row=bool(c.ones))
        same = torch.equal(got, again)
        host = (got if c.row_off is not None else got[None]).cpu()
    except RuntimeError as e:
        pytest.exit("library or runtime error, nothing more is run: %s" % e, returncode=3)
    assert same, "two runs differ"
    return host


def _check(pkg, cuda, c, cell, what):
    want, bound = xc.reference(c)
    got = _product(pkg, cuda, c).numpy()
    ratio = xc.worst_ratio(got, want, bound) if got.shape == want.shape else float("nan")
    print("%s: worst error / bound %.3f" % (what, ratio))                       # (the figure first, then the assertion)
    for key, name in (("families", xc.family_name(cell)), ("cells", _cell_id(cell))):
        if key == "families" or name in _ran[key]:
            _ran[key][name] = max(_ran[key].get(name, 0.0), ratio)
    xc.assert_within(got, want, bound, what)
    return ratio


def test_cell_matches_float64_at_the_row_edges(pkg, cuda, lib, cell_case):
    """One instantiation at M = 1, 3, ROWS-1, ROWS, ROWS+1, 2 ROWS+1, 4 ROWS+1, 8 ROWS+5 (ROWS: the cell's slab height; the planes
    kernel's 32-row step): less than one MFMA step, the slab edges, the third slab reusing a buffer, a second workgroup row owning
    one row, zero-padded rows past a workgroup's range, waves with an empty tile group (the smallest shape of a cell with one tile
    per group leaves most groups empty)."""
    cell, shape = cell_case
    _selects(lib, cell, shape)
    _ran["cells"][_cell_id(cell)] = 0.0                                          # (_check keeps the cell's worst ratio here)
    for M in xc.row_counts(cell[2]):
        c = xc.make_case(M, M, *shape)
        _check(pkg, cuda, c, cell, "%s K=%d N=%d ones=%d M=%d" % (_cell_id(cell), shape[0], shape[1], shape[2], M))


def test_large_row_count(pkg, cuda, lib, family_case):
    """M = 50 001: every workgroup row of a 256-CU part walks at least 3 slabs, at the family's smallest shape."""
    cell, shape = family_case
    _selects(lib, cell, shape)
    _check(pkg, cuda, xc.make_case(17, LARGE_M, *shape), cell, "%s M=%d" % (_cell_id(cell), LARGE_M))


def test_batches(pkg, cuda, lib, family_case):
    """Five batches over one row set -- one empty, one of a single row, neighbours scaled by 2^10 against each other so that a row
    leaked from the larger neighbour is far outside the smaller batch's bound -- and nbatch = 64 (the most the ABI takes), with
    empty batches among them.

    This test found the split forms' truncating operand split too coarse for few-row batches: with pieces cut by truncation the
    six-product form drops up to 2^-21 |x y| per product, all of one sign, and xty_split_kernel<false, 32, 3, 4> missed the bound
    on a batch of ONE row scaled by 2^10 (64 batches, batch 52, element (60, 202): got 278.044006, want 278.044122, error /
    bound 1.033; five batches 0.897, planes 0.786 / 0.915).  The two kernels now cut their pieces by rounding (xty_split_pair,
    csrc/ggnn_bwd_gemm.hip: dropped part < 2^-23 |x y|, mixed signs); the figures since are in DESIGN.md, Tolerances."""
    cell, shape = family_case
    _selects(lib, cell, shape)
    r = cell[2]
    off = [0, 2 * r + 3, 2 * r + 3, 2 * r + 4, 7 * r + 1, 12 * r + 5]
    c = xc.scale_batches(xc.make_case(23, off[-1], *shape, row_off=off))
    want, _ = xc.reference(c)
    assert not want[1].any() and np.abs(want[4]).max() > 100 * np.abs(want[3]).max()
    _check(pkg, cuda, c, cell, "%s five batches" % _cell_id(cell))
    rng = np.random.default_rng(64)
    sizes = rng.integers(0, 9, 64)
    sizes[[5, 40]] = 0
    sizes[[0, 17, 63]] = (r + 1, 2 * r + 1, 1)
    off = [0] + [int(v) for v in np.cumsum(sizes)]
    c = xc.scale_batches(xc.make_case(29, off[-1], *shape, row_off=off))
    assert len(xc.batches(c)) == 64
    _check(pkg, cuda, c, cell, "%s 64 batches" % _cell_id(cell))


def test_accumulate_is_prefill_plus_product(pkg, cuda, lib, family_case):
    """add_to / add_bias_to: the reduction adds the product (and the ones row) into what the buffers hold -- bit-identical to
    prefill + plain product; one product and three batches."""
    cell, shape = family_case
    _selects(lib, cell, shape)
    K, N, r = shape[0], shape[1], cell[2]
    for off in (None, [0, r + 1, r + 1, 4 * r + 1]):
        c = xc.make_case(31, 4 * r + 1, *shape, row_off=off)
        B = 1 if off is None else len(off) - 1
        plain = _product(pkg, cuda, c).to(cuda)                                     # [B, K + 1, N]
        g = torch.Generator(device="cpu").manual_seed(5)
        w0 = (torch.rand(B, K, N, generator=g) * 2 - 1).to(cuda)
        b0 = (torch.rand(B, N, generator=g) * 2 - 1).to(cuda)
        w, b = w0.clone(), b0.clone()
        segs, dy, rows = _device(c, cuda)
        assert pkg.ops.xty(segs, dy, x_rows=rows, row_off=off, ones_row=True, add_to=w, add_bias_to=b) is None
        assert torch.equal(w, w0 + plain[:, :K]) and torch.equal(b, b0 + plain[:, K]), (_cell_id(cell), off)


def test_gathered_index_patterns(pkg, cuda, lib, gathered_case):
    """x_rows with repeats (every per-cell case of a gathered cell has them), with ALL rows equal -- X's last row, and row 0 -- and
    an X with more rows than M.  A leg without row-gathered kernels (GGNN_XTY_ROWS=32) refuses the product instead."""
    if isinstance(gathered_case, Exception):
        raise gathered_case
    if gathered_case is None:
        assert xc.describe(lib, 64, 64, 0, 1)[0] == xc.E_UNSUPPORTED and xc.describe(lib, 4, 4, 1, 1)[0] == xc.E_UNSUPPORTED
        return
    cell, shape = gathered_case
    _selects(lib, cell, shape)
    M = 4 * cell[2] + 1
    for row in (M + 6, 0):
        c = xc.make_case(37, M, *shape, x_rows=np.full(M, row, np.int32))
        assert c.xwide.shape[0] == M + 7
        _check(pkg, cuda, c, cell, "%s all rows = %d" % (_cell_id(cell), row))
    c = xc.make_case(41, M, *shape, x_rows=(np.arange(M)[::-1] // 3 + (M + 6 - (M - 1) // 3)).astype(np.int32))
    assert c.x_rows.max() == M + 6 and c.x_rows.min() >= 0
    _check(pkg, cuda, c, cell, "%s descending triples" % _cell_id(cell))


@pytest.mark.parametrize("K,ones,N,kblocks,default_cell", [
    (4 * 132, 1, 64, 3, None), (4 * 256, 0, 64, 4, None),
    (4 * 132, 1, 128, 3, (2, 0, 32, 3, 2)), (4 * 256, 0, 256, 4, (1, 0, 32, 4, 4))],
    ids=["528-1-3", "1024-0-4", "528-1-N128-3", "1024-0-N256-4"])              # (the N = 64 cases keep the ids they had)
def test_three_and_four_k_blocks(pkg, cuda, lib, K, ones, N, kblocks, default_cell):
    """512 < K <= 1024, ungathered: the product is cut into 3 / 4 K blocks (blockIdx.x), the last one short of whole tile groups
    (K = 528 + ones row: 34 tiles in blocks of 12, the last one 10) or exactly full (K = 1024: 4 x 16).  N = 64 runs on the f32
    kernel in every leg; N = 128 / 256 take the workgroups that are not the first K block through the split families too: in the
    default leg xty_planes_kernel<3, 2> (12 + 8 tiles) and xty_split_kernel<false, 32, 4, 4> (16 + 16 tiles do not fit the planes'
    LDS)."""
    rc, cell, geom = xc.describe(lib, K, N, ones, 0)
    assert rc == 0 and geom[0] == kblocks and geom[2] == (N + 15) // 16, (cell, geom)
    if default_cell is not None and (LEG == "default" or not (LEG or any(v in os.environ for v in xc.LEG_VARS))):
        assert cell == default_cell, (cell, default_cell)
    for M in (cell[2] + 1, 4 * cell[2] + 1):
        _check(pkg, cuda, xc.make_case(M, M, K, N, ones, 0), cell, "K=%d N=%d (%d K blocks, %s) M=%d" % (K, N, kblocks, _cell_id(cell), M))


def test_other_legs_run_every_remaining_instantiation(pkg, cuda, lib, tmp_path):
    """The legs this process is not: one child pytest process over this file each, one at a time, each under its own time limit.
    A child that ends by signal, abort, time limit or a library / runtime error fails the test at once and no further leg is
    started; a child in which only bounds were missed is reported at the end, after the other legs.  Each child runs the cells its
    leg selects and reports them; between them and this process every instantiation of the table has run."""
    if LEG:
        pytest.skip("a leg's own process does not start legs")
    table = set(xc.table(lib))
    mine = set(xc.sweep(lib, xc.PROCESS)[0])
    plain = not any(v in os.environ for v in xc.LEG_VARS)
    if plain:
        assert mine == set(xc.sweep(lib, xc.LEGS["default"])[0])
    legs = [n for n in xc.LEGS if not (plain and n == "default")]
    expect = {n: {_cell_id(c) for c in xc.sweep(lib, xc.LEGS[n])[0]} for n in legs}
    assert set().union({_cell_id(c) for c in mine}, *expect.values()) == {_cell_id(c) for c in table} and len(table) == 41
    me = os.path.abspath(__file__)
    missed = []
    for n in legs:
        env = {k: v for k, v in os.environ.items() if k not in xc.LEG_VARS}
        env.update(xc.LEGS[n].env)
        report = str(tmp_path / ("%s.json" % n))
        env.update(GGNN_XTY_CELLS_LEG=n, GGNN_XTY_CELLS_REPORT=report)
        r = subprocess.run([sys.executable, "-m", "pytest", me, "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rfP",
                            "--deselect", "%s::test_other_legs_run_every_remaining_instantiation" % os.path.relpath(me, ROOT)],
                           env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        # 0: all passed; 1: cases outside their bound, the GPU is fine and the other legs still run; anything else (a signal, an
        # abort, the exit of _product, no tests) ends the test here
        assert r.returncode in (0, 1), (n, r.returncode, r.stdout[-3000:], r.stderr[-2000:])
        assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], (n, r.stdout[-800:])
        ran = json.load(open(report))
        assert set(ran["cells"]) == expect[n], (n, sorted(set(ran["cells"]) ^ expect[n]))
        print("leg %s: %d instantiations, worst error / bound per family %s" % (n, len(ran["cells"]), json.dumps(ran["families"], sort_keys=True)))
        print("\n".join(l for l in r.stdout.splitlines() if "error / bound" in l or l.startswith(("FAILED", "E  "))))
        if r.returncode:
            missed.append((n, [l for l in r.stdout.splitlines() if l.startswith("FAILED")]))
    assert not missed, missed
