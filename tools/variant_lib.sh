#!/bin/bash
# Kernel experiments: build libggnn_hip_<tag>.so = the current objects with some sources recompiled under extra flags.
#   tools/variant_lib.sh <tag> <source.hip[,source2.hip,...]> [-DFLAG=...]      then run with GGNN_LIB_VARIANT=<tag>
# e.g. the fused GRU with its s_memtime stamps for tools/gru_timeline.py:
#   tools/variant_lib.sh tl ggnn_gru_fused.hip,ggnn_gru_fused_split.hip -DGGNN_GRU_STAMPS=1
# the fused GRU with the GGNN_GRU_DBG ablation bits (tools/gru_ablate.py, tools/exp_ablate_f16.sh; the product library has none):
#   tools/variant_lib.sh abl ggnn_gru_fused.hip,ggnn_gru_fused_split.hip -DGGNN_GRU_ABLATE=1
# the compacted message transform with the stamps behind GGNN_K1C_TPTR (tools/k1c_timeline.py):
#   tools/variant_lib.sh k1t ggnn_msg_compact.hip -DGGNN_K1C_STAMPS=1
# the fused GRU backward with the stamps behind GGNN_BWD_TPTR (tools/gru_bwd_timeline.py):
#   tools/variant_lib.sh btl ggnn_gru_bwd_fused.hip,ggnn_gru_bwd_fused_split.hip -DGGNN_BWD_STAMPS=1
# the weight-gradient product with the stamps behind GGNN_XTY_TPTR (tools/xty_timeline.py):
#   tools/variant_lib.sh xtl ggnn_bwd_gemm.hip -DGGNN_XTY_STAMPS=1
# (tools/dense_graph_timeline.py needs none: the stamps of the graph-resident dense kernels are run-time, GGNN_DG_TPTR / GGNN_DGB_TPTR)
set -e
tag=$1; srcs=$2; shift; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd); P=$ROOT/gated-graph-neural-network-samples_amd
objs=$(ls "$P"/build/*.o)
new=""
for src in ${srcs//,/ }; do
    base=$(basename "$src" .hip)
    # the per-source flags of build.py (the translation units it compiles without packed-f32 vector instructions)
    extra=$(cd "$P" && python3 -c "import sys, build; print(' '.join(build.PER_SOURCE_FLAGS.get(sys.argv[1], [])))" "$base.hip")
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -I "$ROOT/include" $extra "$@" -c "$P/csrc/$base.hip" -o "/tmp/${base}_$tag.o"
    objs=$(echo "$objs" | grep -v "/$base.o")
    new="$new /tmp/${base}_$tag.o"
done
hipcc --offload-arch=gfx950 -shared -fPIC $objs $new -o "$P/libggnn_hip_$tag.so"
echo "built $P/libggnn_hip_$tag.so"
