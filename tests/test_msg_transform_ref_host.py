"""tests/msg_transform_ref.py on the CPU, on the very inputs tests/test_gpu_msg_transform_cells.py feeds the kernels:

  *  a plain float32 numpy evaluation and the two operand formats of csrc/ggnn_split.hpp emulated in numpy (bf16x3: six products of
     truncated pieces; f16x2: three products of rounded pieces, weights x 2^8) stay inside the a-priori bound at FACTOR 1, at every
     hidden size -- the condition that the reference alone stays inside the bound;
  *  the comparison has teeth at the factor the GPU test uses (msg_transform_ref.CAP[D]): the eight wrong results of
     msg_transform_ref.corruptions each fail, on the small cases, the backward's case and the multi-pass case;
  *  ggnn_msg_transform_compact_describe (loads the library; needs no GPU) is exported and declared, refuses what the launch
     refuses, reports a consistent schedule, and over the legs of the GPU test selects exactly the 21 instantiations."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import msg_transform_ref as mr
from conftest import PKG, ROOT

SMALL = [(name, D) for D in mr.SIZES for name in mr.SMALL_CASES]
SMALL_IDS = ["%s-D%d" % p for p in SMALL]


@pytest.fixture(scope="module")
def pkg_lib():
    pkg = importlib.import_module(PKG)
    return pkg, pkg._lib.load()


def _multipass(pkg, D):
    """The multi-pass case of the GPU test at the schedule this machine's library reports (without a GPU: its 256-CU default)."""
    desc = lambda off: pkg.ops.msg_transform_compact_describe(D, off, mr.BF16X3)
    big, small = mr.multipass_rows(desc, 234 if D < 128 else 300, 160000 if D < 128 else 80000)
    d = desc((0, big, big + small))
    return mr.make_case("multipass", D, (big, small)), mr.strides(d, D), d


def _cases(D, pkg):
    for name in mr.SMALL_CASES:
        yield mr.small_case(name, D), None
    yield mr.backward_case(D)[0], None
    c, strides, _ = _multipass(pkg, D)
    yield c, strides


@pytest.mark.parametrize("D", mr.SIZES)
def test_float32_and_both_formats_stay_within_factor_1(D, pkg_lib):
    worst = {}
    for c, _ in _cases(D, pkg_lib[0]):
        ref, bnd = mr.reference(c), mr.bound(c)
        for fmt, mm in mr.FORMATS.items():
            if c.name == "backward" and fmt == "f16x2":
                continue                                             # (the backward always multiplies in the exact format)
            r = mr.check(mr.with_guard(mr.evaluate(c, mm).astype(np.float32)), ref, bnd, 1.0, "%s %s D=%d" % (fmt, c.name, D))
            worst[fmt] = max(worst.get(fmt, 0.0), r)
    print("D=%d, numpy evaluations, worst error / bound: %s" % (D, json.dumps(worst, sort_keys=True)))
    assert set(worst) == set(mr.FORMATS)


@pytest.mark.parametrize("D", mr.SIZES)
def test_wrong_results_fail_at_the_cap(D, pkg_lib):
    """Every corruption a case has room for fails on it; over the cases of a hidden size all eight kinds occur (the two that need
    a K remainder at D = 100 only)."""
    seen = set()
    for c, strides in _cases(D, pkg_lib[0]):
        ref, bnd = mr.reference(c), mr.bound(c)
        mr.check(mr.with_guard(ref.astype(np.float32)), ref, bnd, mr.CAP[D], "uncorrupted")
        for what, buf in mr.corruptions(c, ref, strides).items():
            with pytest.raises(AssertionError, match="outside|guard row"):
                mr.check(buf, ref, bnd, mr.CAP[D], "%s %s D=%d" % (what, c.name, D))
            seen.add(what.split(" (")[0])
    want = {"stale prefetch", "neighbour's weights", "W transposed", "low piece dropped", "acc_scale missing",
            "clamped row stored past the last type", "clamped row stored into the next type"}
    if D % 16:
        want |= {"K remainder dropped", "last column tile dropped"}
    assert seen == want, sorted(seen ^ want)


def test_the_stale_tile_of_the_multipass_case_is_a_third_pass(pkg_lib):
    """The multi-pass case carries the stale-prefetch corruption where only the in-loop prefetch reaches: a tile two strides in."""
    for D in (100, 256):
        c, strides, d = _multipass(pkg_lib[0], D)
        assert all(mr.walks(d["types"])), d
        t = [t for t, (_, mx, _) in enumerate(d["types"]) if mx >= 3][0]
        n_wt = (int(c.row_off[t + 1] - c.row_off[t]) + 15) // 16
        assert (n_wt - 1) // strides[t] >= 2
        assert "stale prefetch (type %d)" % t in mr.corruptions(c, mr.reference(c), strides)


# ---- the describe query (needs the library, no GPU) -----------------------------------------------------------------------------
def _describe(lib, D, off, fmt):
    import ctypes
    T = len(off) - 1
    out = (ctypes.c_int32 * (4 + 3 * max(T, 1)))()
    rc = lib.ggnn_msg_transform_compact_describe(D, T, (ctypes.c_int64 * (T + 1))(*off), fmt, out)
    return rc, list(out)


def test_describe_is_exported_and_declared(pkg_lib):
    pkg, lib = pkg_lib
    header = open(os.path.join(ROOT, "include", "ggnn_hip.h")).read()
    assert hasattr(lib, "ggnn_msg_transform_compact_describe") and "ggnn_msg_transform_compact_describe(" in header
    assert "ggnn_msg_transform_compact_describe" in pkg._lib.SYMBOLS
    for i, fam in enumerate(pkg.ops.MSG_TRANSFORM_FAMILIES):
        assert "#define GGNN_MSG_TRANSFORM_%s %d" % (fam.upper().replace("-", "_"), i) in header


def test_describe_refuses_what_the_launch_refuses(pkg_lib):
    pkg, lib = pkg_lib
    assert _describe(lib, 100, (0, 5), 3)[0] == 0
    assert lib.ggnn_msg_transform_compact_describe(100, 1, None, 3, None) == -1
    assert _describe(lib, 100, (0, 5), 1)[0] == -1 and b"fmt" in lib.ggnn_last_error()
    assert _describe(lib, 100, (1, 5), 3)[0] == -1
    assert _describe(lib, 100, (0, 5, 4), 3)[0] == -1 and b"monotone" in lib.ggnn_last_error()
    assert _describe(lib, 100, tuple(range(66)), 3)[0] == -1                     # T = 65
    assert _describe(lib, 200, (0, 5), 3)[0] == -2 and _describe(lib, 36, (0, 5), 3)[0] == -2
    assert _describe(lib, 256, (0, 1 << 22), 3)[0] == -2 and b"2^30" in lib.ggnn_last_error()
    with pytest.raises(pkg._lib.GGNNError):
        pkg.ops.msg_transform_compact_describe(200, (0, 5))


@pytest.mark.parametrize("D", mr.SIZES)
def test_described_schedule_is_consistent(D, pkg_lib):
    """Workgroups add up, a type has workgroups exactly where it has rows, its waves' walks differ by at most a tile and cover its
    tiles; no rows, no launch.  fmt = 0 means the exact format."""
    pkg, lib = pkg_lib
    desc = pkg.ops.msg_transform_compact_describe
    assert desc(D, (0, 0, 0), mr.F16X2)["workgroups"] == 0
    assert desc(D, (0, 40), 0) == desc(D, (0, 40), mr.BF16X3)
    for rows in list(mr.SMALL_CASES.values()) + [(9000, 1, 70000, 300), (50001,), mr.BACKWARD_ROWS]:
        off = [0] + [int(x) for x in np.cumsum(rows)]
        d = desc(D, off, mr.F16X2)
        assert d["family"] == ("whole-block" if D < 128 else d["family"]) and d["family"] in pkg.ops.MSG_TRANSFORM_FAMILIES
        assert d["workgroups"] == sum(wg for wg, _, _ in d["types"]) and d["waves"] == 8
        for n, (wg, mx, mn), stride in zip(rows, d["types"], mr.strides(d, D)):
            n_wt = (n + 15) // 16
            assert (wg > 0) == (n > 0) and 0 <= mx - mn <= 1
            if n:
                assert mx == -(-n_wt // stride) and mn == n_wt // stride and stride * mn <= n_wt <= stride * mx


_SWEEP = "import importlib, json, sys; sys.path[:0] = [%r, %r]; import msg_transform_ref as mr; " \
         "ops = importlib.import_module(%r).ops; ds = [(D, ops.msg_transform_compact_describe(D, (0, 40), f)) for D in mr.SIZES " \
         "for f in (mr.BF16X3, mr.F16X2)]; print(json.dumps(sorted({mr.instantiation(d['family'], D, d['fmt']) for D, d in ds})))"


def test_the_legs_select_exactly_the_21_instantiations():
    """One process per leg of the GPU test (GGNN_MATRIX and GGNN_PANEL_TRANSFORM are read once per process)."""
    assert len(set(mr.INSTANTIATIONS)) == 21
    union, per_leg = set(), {}
    for name, (env_add, only) in mr.LEGS.items():
        env = {k: v for k, v in os.environ.items() if k not in mr.LEG_VARS}
        env.update(env_add)
        r = subprocess.run([sys.executable, "-c", _SWEEP % (ROOT, os.path.join(ROOT, "tests"), PKG)], env=env, capture_output=True,
                           text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        per_leg[name] = {n for n in json.loads(r.stdout.splitlines()[-1]) if only is None or n.startswith(only)}
        union |= per_leg[name]
    assert union == set(mr.INSTANTIATIONS), sorted(union ^ set(mr.INSTANTIATIONS))
    assert len(per_leg["split"]) == 12 and len(per_leg["f32"]) == 6 and len(per_leg["split-stationary"]) == 3
    assert not (per_leg["split"] & per_leg["f32"]) and not (per_leg["split-stationary"] & (per_leg["split"] | per_leg["f32"]))
