// A training step's weight images at the column-panel hidden sizes (128 / 192 / 256) in ONE launch: what train_prepare_kernel
// (ggnn_train.hip) does for the whole-block sizes.  Every optimisation step changes every weight, so every step rebuilds every image:
// per layer the T * NP panel images of the edge weights and the T * NP of their transposes (both of the weight-dropout-MASKED weights,
// the mask applied on the fly: ggnn_philox.hpp), the 3 (nx + 1) NP images of the panel GRU forward in the layer's operand format and
// the 3 (nx + 1) NP of its backward -- 80 images of 64-96 KiB for one layer at D = 256, T = 4.  Driven layer by layer from the host that
// is a mask launch, a transpose copy and four pack launches per layer at the head of the step.
//
// A pure streaming kernel: no LDS, each thread writes whole 4-byte image words.  The image layouts and the order of the images are
// those of the per-layer pack kernels (ggnn_panel.hip, ggnn_gru_bwd_panel.hip) because they are the same device functions
// (ggnn_panel.hpp): pack_panel_*_image_fn write an image from a value(k, n) functor, panel_gru_{fwd,bwd}_image_src name the weight
// panel behind image i.  Only the masked edge-weight functor is new here.
#include "ggnn_panel.hpp"
#include "ggnn_philox.hpp"

namespace ggnn {

// ggnn_panel.hip
int gru_panel_supported(int D);
int transform_panel_image_floats(int D);
bool transform_panel_ring();

namespace {

constexpr int kPanelPrepMaxLayers = 16;
struct PanelPrepArgs {
    const float* edge_w[kPanelPrepMaxLayers]; const float* Wg[kPanelPrepMaxLayers]; const float* Wc[kPanelPrepMaxLayers];
    float* edge_img[kPanelPrepMaxLayers]; float* edge_img_t[kPanelPrepMaxLayers]; float* gru_img[kPanelPrepMaxLayers]; float* gru_bwd_img[kPanelPrepMaxLayers];
    unsigned long long seed[kPanelPrepMaxLayers];
    int nx[kPanelPrepMaxLayers];
    int gru_fmt[kPanelPrepMaxLayers];       // operand format of layer l's GRU FORWARD images (kSplitF16x2 / kSplitBf16x3)
    int T; float keep;
};

// panel (type t, columns c0 .. c0+63) of the masked edge weights, or of their transposes (the backward's Z = dHc W_t^T): masked like
// ggnn_dropout_f32 masks the [T*D, D] variable: row key = t*D + (row of W_t), column = column of W_t
template <int D, bool TRANS>
struct MaskedEdgeSrc {
    const float* W; int t, c0; float keep; unsigned long long seed;
    __device__ __forceinline__ float operator()(int k, int n) const {
        const int r = TRANS ? c0 + n : k, c = TRANS ? k : c0 + n;
        float v = W[(size_t)r * D + c];
        if (keep < 1.0f) v = dropout_apply(v, keep, seed, (unsigned long long)(t * D + r), c);
        return v;
    }
};

// SPLIT: every image in split form; RING: the edge-weight images in the ring transform's chunk-major format (else the
// stationary-image kernel's plane-major one).  The edge-weight images and the GRU backward's are always exact bf16 x 3.
template <int D, bool SPLIT, bool RING>
__global__ __launch_bounds__(256) void train_panel_prepare_kernel(PanelPrepArgs a) {
    using C = PanelCfg<D>;
    constexpr int NP = C::NP;
    constexpr int EDGE_IMG = SPLIT ? PanelGruSplitCfg<D>::IMG : C::IMG;      // (both split formats of the transform have one size)
    static_assert(PanelGruSplitCfg<D>::IMG == PanelSplitCfg<D>::IMG, "both split image formats of the transform have one size");
    const int l = blockIdx.z, i = blockIdx.y;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    const int ne = a.T * NP, ng = panel_gru_images(D, a.nx[l]);
    if (i < 2 * ne) {
        const bool tr = i >= ne;                                          // (block-uniform)
        const int j = tr ? i - ne : i, t = j / NP, p = j % NP;
        const float* W = a.edge_w[l] + (size_t)t * D * D;
        float* img = (tr ? a.edge_img_t[l] : a.edge_img[l]) + (size_t)j * EDGE_IMG;
        auto write = [&](auto src) {
            if constexpr (!SPLIT) pack_panel_image_fn<D>(src, img, first, stride);
            else if constexpr (RING) pack_panel_gru_split_image_fn<D, kSplitBf16x3>(src, img, first, stride);
            else pack_panel_split_image_fn<D>(src, img, first, stride);
        };
        if (tr) write(MaskedEdgeSrc<D, true>{W, t, p * C::BN, a.keep, a.seed[l]});
        else write(MaskedEdgeSrc<D, false>{W, t, p * C::BN, a.keep, a.seed[l]});
    } else if (i < 2 * ne + ng) {
        const int ci = i - 2 * ne;
        const PanelSrc<false> src = panel_gru_fwd_image_src<D>(a.Wg[l], a.Wc[l], a.nx[l], ci);
        if constexpr (SPLIT) {
            if (a.gru_fmt[l] == kSplitF16x2)         // (block-uniform)
                pack_panel_gru_split_image_fn<D, kSplitF16x2>(src, a.gru_img[l] + (size_t)ci * PanelGruSplitCfg<D, kSplitF16x2>::IMG, first, stride);
            else
                pack_panel_gru_split_image_fn<D, kSplitBf16x3>(src, a.gru_img[l] + (size_t)ci * PanelGruSplitCfg<D>::IMG, first, stride);
        } else pack_panel_image_fn<D>(src, a.gru_img[l] + (size_t)ci * C::IMG, first, stride);
    } else if (i < 2 * ne + 2 * ng) {
        const int bi = i - 2 * ne - ng;
        const PanelSrc<true> src = panel_gru_bwd_image_src<D>(a.Wg[l], a.Wc[l], a.nx[l], bi);
        if constexpr (SPLIT) pack_panel_gru_split_image_fn<D, kSplitBf16x3>(src, a.gru_bwd_img[l] + (size_t)bi * PanelGruSplitCfg<D>::IMG, first, stride);
        else pack_panel_image_fn<D>(src, a.gru_bwd_img[l] + (size_t)bi * C::IMG, first, stride);
    }
}

template <int D>
void launch_panel_prepare(const PanelPrepArgs& a, dim3 grid, hipStream_t st) {
    if (!split_matrix_path()) hipLaunchKernelGGL((train_panel_prepare_kernel<D, false, false>), grid, dim3(256), 0, st, a);
    else if (transform_panel_ring()) hipLaunchKernelGGL((train_panel_prepare_kernel<D, true, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((train_panel_prepare_kernel<D, true, false>), grid, dim3(256), 0, st, a);
}

}  // namespace
}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_sparse_train_panel_supported(int D) { return panel_hidden_ok(D); }

extern "C" int ggnn_sparse_train_panel_prepare_f32(int num_layers, int T, int D, const int32_t* nx, const float* const* edge_w,
                                                   float keep_prob, const uint64_t* seeds, const float* const* Wg, const float* const* Wc,
                                                   const int32_t* gru_fmt, float* const* edge_packed, float* const* edge_packed_t,
                                                   float* const* gru_packed, float* const* gru_bwd_packed, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(num_layers > 0 && num_layers <= kPanelPrepMaxLayers, "num_layers %d outside 1..%d", num_layers, kPanelPrepMaxLayers);
    GGNN_CHECK_ARG(T > 0 && T <= 64 && nx && edge_w && Wg && Wc && edge_packed && edge_packed_t && gru_packed && gru_bwd_packed, "bad arguments");
    GGNN_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f && (keep_prob >= 1.0f || seeds), "keep_prob %g outside (0, 1] or seeds missing", (double)keep_prob);
    if (!ggnn_sparse_train_panel_supported(D) || !gru_panel_supported(D))
        return fail(GGNN_E_UNSUPPORTED, "no column-panel stage images for hidden size %d", D);
    PanelPrepArgs a{};
    a.T = T; a.keep = keep_prob;
    int max_images = 0;
    for (int l = 0; l < num_layers; ++l) {
        GGNN_CHECK_ARG(nx[l] >= 1 && nx[l] <= 3, "layer %d: nx %d outside 1..3", l, nx[l]);
        GGNN_CHECK_ARG(edge_w[l] && Wg[l] && Wc[l] && edge_packed[l] && edge_packed_t[l] && gru_packed[l] && gru_bwd_packed[l], "layer %d: null pointer", l);
        GGNN_CHECK_ARG(aligned16(edge_packed[l]) && aligned16(edge_packed_t[l]) && aligned16(gru_packed[l]) && aligned16(gru_bwd_packed[l]),
                       "layer %d: misaligned image buffer", l);
        GGNN_CHECK_ARG(!gru_fmt || gru_fmt[l] == 0 || gru_fmt[l] == GGNN_GRU_FMT_F16X2 || gru_fmt[l] == GGNN_GRU_FMT_BF16X3,
                       "layer %d: gru_fmt %d is not a GGNN_GRU_FMT_* value", l, gru_fmt[l]);
        a.edge_w[l] = edge_w[l]; a.Wg[l] = Wg[l]; a.Wc[l] = Wc[l];
        a.edge_img[l] = edge_packed[l]; a.edge_img_t[l] = edge_packed_t[l]; a.gru_img[l] = gru_packed[l]; a.gru_bwd_img[l] = gru_bwd_packed[l];
        a.seed[l] = seeds ? seeds[l] : 0ULL; a.nx[l] = nx[l];
        a.gru_fmt[l] = gru_launch_fmt(gru_fmt ? gru_fmt[l] : kSplitBf16x3);
        const int images = 2 * T * (D / 64) + 2 * panel_gru_images(D, nx[l]);
        if (images > max_images) max_images = images;
    }
    const dim3 grid(8, max_images, num_layers);
    hipStream_t st = (hipStream_t)stream;
    panel_for_D(D, [&](auto d) { launch_panel_prepare<decltype(d)::value>(a, grid, st); });
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}
