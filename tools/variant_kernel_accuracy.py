#!/usr/bin/env python3
"""Record profiles/variant_kernel_accuracy.json: per operation and shape class, the largest error / a-priori-bound ratio that
tests/variant_kernel_ref.assert_within saw (1 = the bound; the GPU tests allow 2).

    python tools/variant_kernel_accuracy.py [--out profiles/variant_kernel_accuracy.json]

Runs tests/test_variant_kernel_ref_host.py in this process (section `cpu_float32`: the float32 CPU evaluation of the formulas)
and, where a GPU is present, tests/test_gpu_variant_kernels.py (section `gpu_mi355x`); a section that cannot be measured here
is kept from the existing file.  Both test files must pass."""
import argparse
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(path, extra):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import variant_kernel_ref as ref
    ref.RATIOS.clear()
    rc = pytest.main([os.path.join(ROOT, path), "-q", "-p", "no:cacheprovider"] + extra)
    if rc != 0:
        raise SystemExit("%s failed (exit %d): nothing recorded" % (path, rc))
    return {k: float("%.4g" % v) for k, v in sorted(ref.RATIOS.items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variant_kernel_accuracy.json"))
    args = ap.parse_args()
    import torch
    old = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out = {"_meta": {
        "what": "largest |got - float64 reference| / a-priori bound per operation and shape class (tests/variant_kernel_ref.py; "
                "1 = the bound, the GPU tests allow 2); written by tools/variant_kernel_accuracy.py",
        "gpu_mi355x": "one run of tests/test_gpu_variant_kernels.py on one MI355X (gfx950)",
        "cpu_float32": "float32 CPU evaluation of the same formulas on the same inputs (tests/test_variant_kernel_ref_host.py)"}}
    out["cpu_float32"] = _run("tests/test_variant_kernel_ref_host.py", [])
    out["gpu_mi355x"] = _run("tests/test_gpu_variant_kernels.py", ["-m", "gpu"]) if torch.cuda.is_available() else old.get("gpu_mi355x")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote %s: %d cpu_float32 keys, %s gpu_mi355x keys" % (args.out, len(out["cpu_float32"]),
                                                               len(out["gpu_mi355x"]) if out["gpu_mi355x"] else "no"))


if __name__ == "__main__":
    main()
