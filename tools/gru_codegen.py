#!/usr/bin/env python3
"""What the compiler made of the hot forward kernels (no GPU needed): cross-compiles the split-form fused GRU and the compacted message
transform for gfx950 with build.py's flags, and records per kernel the registers, scratch, occupancy and the static instruction mix --
whole kernel and inside the pass loop (the widest backward branch that encloses matrix instructions).

    python tools/gru_codegen.py --out mix.json                       # every fused-GRU / compact-transform kernel of this tree
    python tools/gru_codegen.py --asm a.s b.s --out mix.json         # ... of listings made elsewhere (e.g. from the parent commit)
    python tools/gru_codegen.py --pair parent.json this.json --out profiles/gru_issue_diet_codegen.json
    # any other kernel family: its translation units and a regex on the demangled kernel names; with them --pair compares every kernel
    python tools/gru_codegen.py --sources ggnn_panel.hip,ggnn_rnn_panel.hip --kernels 'panel_kernel<|ring_kernel<' --out this.json
    python tools/gru_codegen.py --kernels . --pair parent.json this.json --out profiles/panel_shared_layer_codegen.json
    # (kernels whose template list changed are paired through the RENAMED table below)
"""
import argparse, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gated-graph-neural-network-samples_amd")
SOURCES = ["ggnn_gru_fused_split.hip", "ggnn_msg_compact.hip"]
KERNELS = re.compile(r"ggnn_gru_fused_kernel<|msg_transform_compact_kernel<")
COUNTS = {
    "v_mfma": r"v_mfma_", "v_mfma_f16": r"v_mfma_f32_16x16x32_f16", "v_mfma_bf16": r"v_mfma_f32_16x16x\d+_bf16", "v_mfma_f32": r"v_mfma_f32_16x16x4_f32",
    "ds_read_b128": r"ds_read_b128", "cond_branch": r"s_cbranch_(scc|vcc|exec)", "s_waitcnt": r"s_waitcnt",
    "scalar_mask": r"s_(and|or|andn2|orn2|xor|cselect)_b64|s_(and|or|andn2)_saveexec_b64",
    "v_readlane": r"v_readlane_b32", "v_writelane": r"v_writelane_b32", "v_mov": r"v_mov_|v_accvgpr_mov|v_pk_mov",
    "global_load_lds": r"global_load_lds_", "ds_read": r"ds_read_",
    "ds_bpermute_b32": r"ds_bpermute_b32", "v_permlane_swap": r"v_permlane(16|32)_swap", "v_exp_f32": r"v_exp_f32", "v_rcp_f32": r"v_rcp_f32",
    "v_div": r"v_div_(scale|fmas|fixup)_f32",
}
COUNTS = {k: re.compile(r"(%s)" % v) for k, v in COUNTS.items()}
# hot instantiations: label -> (parent's kernel, this tree's kernel), template argument lists as c++filt prints them
HOT = {
    "gru nx=1 f16x2 form 1": ("ggnn_gru_fused_kernel<100, 1, 4, false, true, true, false, 1, 2, 1, true>",) * 2,
    "gru nx=2 f16x2 form 1": ("ggnn_gru_fused_kernel<100, 2, 4, false, true, true, false, 1, 2, 1, true>",) * 2,
    "gru nx=3 f16x2 form 1": ("ggnn_gru_fused_kernel<100, 3, 4, false, true, true, false, 1, 2, 1, true>",) * 2,
    "gru nx=1 bf16x3 form 0": ("ggnn_gru_fused_kernel<100, 1, 8, false, true, true, false, 0, 3, 1, true>",) * 2,
    "gru nx=2 bf16x3 form 1": ("ggnn_gru_fused_kernel<100, 2, 4, false, true, true, false, 1, 3, 1, true>",) * 2,
    "gru nx=3 bf16x3 form 1": ("ggnn_gru_fused_kernel<100, 3, 4, false, true, true, false, 1, 3, 1, true>",) * 2,
    "compact transform f16x2": ("msg_transform_compact_kernel<100, 8, true, 2>",) * 2,
    "compact transform bf16x3": ("msg_transform_compact_kernel<100, 8, true, 3>",) * 2,
}

# kernels whose template list changed: parent's name -> this tree's (--pair with --kernels compares them as one kernel).  The fused GRU
# backward kept one form per matrix path: <D, NX, NW = 8, PREFETCH = 3 | 0, RING = 2, SPLIT> became <D, NX, SPLIT>
RENAMED = {"ggnn_gru_bwd_fused_kernel<%d, %d, 8, %d, 2, %s>" % (D, nx, 3 if split else 0, "true" if split else "false"):
           "ggnn_gru_bwd_fused_kernel<%d, %d, %s>" % (D, nx, "true" if split else "false")
           for D in (32, 64, 100) for nx in (1, 2, 3) for split in (False, True)}


def compile_asm(src, out, extra):
    sys.path.insert(0, PKG)
    import build
    cmd = ["hipcc", "--offload-arch=" + build.ARCH, "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-I", os.path.join(ROOT, "include")]
    cmd += build.PER_SOURCE_FLAGS.get(src, []) + extra + ["--cuda-device-only", "-S", os.path.join(PKG, "csrc", src), "-o", out]
    subprocess.run(cmd, check=True)


def mix(lines):
    c = {k: 0 for k in COUNTS}
    n = 0
    for ln in lines:
        t = ln.strip()
        if not t or t[0] in ".;" or t.endswith(":"):
            continue
        n += 1
        for k, rx in COUNTS.items():
            if rx.match(t):
                c[k] += 1
    c["instructions"] = n
    return c


def pass_loop(body):
    """Line range of the widest loop (backward branch -> its label) that encloses a matrix instruction."""
    label_at = {}
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label_at[m.group(1)] = i
    mf = [i for i, ln in enumerate(body) if ln.strip().startswith("v_mfma_")]
    best = None
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            lo = label_at[m.group(1)]
            if any(lo < k < i for k in mf) and (best is None or i - lo > best[1] - best[0]):
                best = (lo, i)
    return best


def parse(path, kernels=KERNELS):
    txt = open(path, encoding="utf-8", errors="replace").read().split("\n")
    out = {}
    i = 0
    while i < len(txt):
        m = re.match(r"^(_Z\w+):", txt[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        j = i + 1
        while j < len(txt) and not txt[j].startswith(".Lfunc_end"):
            j += 1
        body = txt[i + 1:j]
        meta = {}
        k = j
        while k < len(txt) and k < j + 80 and not re.match(r"^_Z\w+:", txt[k]):
            for key, rx in (("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"), ("sgprs", r"; TotalNumSgprs: (\d+)"),
                            ("scratch_bytes", r"; ScratchSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)"),
                            ("sgpr_spills", r"; SGPRSpillCount: (\d+)"), ("vgpr_spills", r"; VGPRSpillCount: (\d+)")):
                mm = re.match(rx, txt[k].strip())
                if mm and key not in meta:
                    meta[key] = int(mm.group(1))
            k += 1
        out[name] = (meta, body)
        i = j
    names = list(out)
    dem = subprocess.run(["c++filt"] + names, check=True, capture_output=True, text=True).stdout.strip().split("\n")
    res = {}
    for n, d in zip(names, dem):
        if not kernels.search(d):
            continue
        d = re.sub(r"^void ggnn::(\(anonymous namespace\)::)?", "", d)
        d = re.sub(r"\(.*$", "", d).replace("(ggnn::SplitFormat)", "").replace("(bool)", "")
        meta, body = out[n]
        e = dict(meta)
        e["kernel"] = mix(body)
        lp = pass_loop(body)
        e["pass_loop"] = mix(body[lp[0]:lp[1] + 1]) if lp else None
        res[d] = e
    return res


def pair_all(par, cur):
    """Every kernel of two listings' records side by side (the form of profiles/xty_shared_layer_codegen.json)."""
    keys = ("vgprs", "sgprs", "scratch_bytes", "occupancy")
    row = lambda e: dict({k: e.get(k) for k in keys}, **{k: e["kernel"][k] for k in ("instructions", "v_mfma", "global_load_lds", "ds_read")})
    doc = {"note": "static code generation of every kernel of the listed translation units, parent commit vs this change (tools/gru_codegen.py: "
                   "hipcc --offload-arch=gfx950, build.py's per-source flags, --cuda-device-only -S). instructions: lines of the kernel's "
                   "assembly that are instructions; v_mfma / global_load_lds / ds_read: those that start with the word; scratch_bytes: per lane.",
           "kernels": {k: {"parent": row(par[k]), "branch": row(cur[k])} for k in sorted(cur) if k in par},
           "only_parent": sorted(set(par) - set(cur)), "only_branch": sorted(set(cur) - set(par))}
    rows = doc["kernels"].values()
    doc["summary"] = {
        "kernels": len(doc["kernels"]),
        "identical_rows": sum(r["parent"] == r["branch"] for r in rows),
        "scratch_nonzero": sorted(k for k, r in doc["kernels"].items() if r["branch"]["scratch_bytes"] or r["parent"]["scratch_bytes"]),
        "mfma_or_lds_dma_count_differs": sorted(k for k, r in doc["kernels"].items()
                                                if any(r["parent"][f] != r["branch"][f] for f in ("v_mfma", "global_load_lds"))),
        "occupancy_below_2_where_parent_has_2": sorted(k for k, r in doc["kernels"].items()
                                                       if r["parent"]["occupancy"] >= 2 and r["branch"]["occupancy"] < 2),
        "vgprs_differ": {k: [r["parent"]["vgprs"], r["branch"]["vgprs"]] for k, r in doc["kernels"].items() if r["parent"]["vgprs"] != r["branch"]["vgprs"]},
        "instructions_grew": {k: [r["parent"]["instructions"], r["branch"]["instructions"]] for k, r in doc["kernels"].items()
                              if r["branch"]["instructions"] > r["parent"]["instructions"]},
    }
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", nargs="*")
    ap.add_argument("--pair", nargs=2)
    ap.add_argument("--out", required=True)
    ap.add_argument("--flags", default="")
    ap.add_argument("--sources", help="comma-separated csrc/*.hip translation units instead of the fused GRU and compact transform")
    ap.add_argument("--kernels", help="regex on the demangled kernel names to keep; with --pair: compare every kernel of the two records")
    a = ap.parse_args()
    kernels = re.compile(a.kernels) if a.kernels else KERNELS
    if a.pair:
        par, cur = (json.load(open(p)) for p in a.pair)
        if a.kernels:
            par, cur = ({k: v for k, v in d.items() if kernels.search(k)} for d in (par, cur))
            par = {RENAMED.get(k, k): v for k, v in par.items()}
            doc = pair_all(par, cur)
            json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)
            print(json.dumps({k: (v if not isinstance(v, dict) else len(v)) for k, v in doc["summary"].items()}, indent=1))
            return
        doc = {"note": "static code generation of the hot forward kernels, parent commit vs this change (tools/gru_codegen.py: hipcc "
                       "--offload-arch=gfx950, build.py's per-source flags, --cuda-device-only -S; pass_loop = the widest loop that "
                       "encloses matrix instructions)", "kernels": {}}
        for label, (pk, ck) in HOT.items():
            doc["kernels"][label] = {"parent": dict(par[pk], name=pk), "branch": dict(cur[ck], name=ck)}
        # the generic inference instantiations behind the GGNN_GRU_FORM override (forms 0 and 2): registers and scratch only
        doc["other_inference"] = {}
        keys = ("vgprs", "sgprs", "scratch_bytes", "occupancy")
        for form in (0, 2):
            for fmt in (2, 3):
                for nx in (1, 2, 3):
                    pk = ck = "ggnn_gru_fused_kernel<100, %d, 8, false, true, true, false, %d, %d, -1, false>" % (nx, form, fmt)
                    doc["other_inference"]["gru nx=%d %s form %d" % (nx, {2: "f16x2", 3: "bf16x3"}[fmt], form)] = {
                        "parent": dict({k: par[pk].get(k) for k in keys}, name=pk), "branch": dict({k: cur[ck].get(k) for k in keys}, name=ck)}
        json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)
        return
    res = {}
    if a.asm:
        for p in a.asm:
            res.update(parse(p, kernels))
    else:
        with tempfile.TemporaryDirectory() as td:
            for src in (a.sources.split(",") if a.sources else SOURCES):
                out = os.path.join(td, src[:-4] + ".s")
                compile_asm(src, out, a.flags.split())
                res.update(parse(out, kernels))
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    for k in sorted(res):
        e = res[k]
        lp = e["pass_loop"] or {}
        print("%-90s vgpr %3s sgpr %3s scratch %3s occ %s | mfma %s ds128 %s br %s mask %s wait %s rdlane %s/%s (loop %s/%s) mov %s" % (
            k, e.get("vgprs"), e.get("sgprs"), e.get("scratch_bytes"), e.get("occupancy"), e["kernel"]["v_mfma"], e["kernel"]["ds_read_b128"],
            e["kernel"]["cond_branch"], e["kernel"]["scalar_mask"], e["kernel"]["s_waitcnt"], e["kernel"]["v_readlane"], e["kernel"]["v_writelane"],
            lp.get("v_readlane"), lp.get("v_writelane"), e["kernel"]["v_mov"]))


if __name__ == "__main__":
    main()
