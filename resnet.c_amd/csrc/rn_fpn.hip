// Feature pyramid: the top-down step of torchvision's FeaturePyramidNetwork as one launch
// (rn_upsample_nearest_add_forward_dt: dst = lat + nearest_upsample(top), or the plain nearest upsample), and the
// neck itself as an object over the library's own contractions, max-pool and export (rn_fpn_*).  The reference
// classifies whole images only; nothing here has a counterpart in it.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "rn_conv_params.h"
#include "rn_internal.h"
#include "rn_private.h"

using rn_gemm::bf16_t;
using rn_gemm::u32x4;

namespace {

// ---- the top-down kernel ----------------------------------------------------------------------------------
// Bound by HBM: dst and lat stream once, top is read H / h times, the repeats from cache (at 2x the two output
// rows of a source row are adjacent in the grid's walk, the two columns adjacent lanes' runs).  A "chunk" is 16
// bytes along C; a pixel is cpp chunks.  A block takes `span` consecutive pixels of one output row (span * cpp is
// about kNaChunks, so short pixels are grouped and a long pixel is one block's loop): consecutive lanes hold
// consecutive chunks, a wave stores 1 KiB in a row and loads runs of cpp chunks of top.  The source row is computed
// once per output row (a scalar), the source column per chunk: one fp32 multiply, no table.  Four chunks per thread
// are loaded before the first is stored.  Both grid dimensions stride: rows of all images in y, spans of a row in
// x.  256 threads, no LDS.  Every chunk is read (lat, top) and written (dst) by the same thread, the reads of a trip
// before its writes: dst == lat is safe by construction.  Offsets are 64-bit from the image on; inside a block's
// span they are 32-bit (span * cpp < 2^31 by the host's choice of span).
constexpr uint32_t kNaBlock = 256, kNaUnroll = 4, kNaChunks = kNaBlock * kNaUnroll;

struct nearest_args {
    const uint4 *top, *lat;
    uint4 *dst;
    uint32_t h, w, H, W, rows;  // rows = B * H
    uint32_t cpp, span, spans;  // chunks of a pixel; pixels of a block's run; runs of a row
    uint32_t mul_cpp, shr_cpp;
    float scale_h, scale_w;
};

// the contract's source index of output o
__device__ __forceinline__ uint32_t nearest_index(uint32_t o, float scale, uint32_t n_in)
{
    const uint32_t i = (uint32_t)floorf(__fmul_rn((float)o, scale));  // the product rounded on its own; never negative
    return i < n_in - 1 ? i : n_in - 1;
}

template <typename T>
__device__ __forceinline__ uint4 add_chunk(const uint4 a, const uint4 b)
{
    constexpr int EPT = rn_gemm::OutVec<T>::EPT;
    const u32x4 ua{a.x, a.y, a.z, a.w}, ub{b.x, b.y, b.z, b.w};
    float va[EPT], vb[EPT];
    rn_gemm::OutVec<T>::unpack(ua, va);
    rn_gemm::OutVec<T>::unpack(ub, vb);
#pragma unroll
    for (int j = 0; j < EPT; ++j) va[j] = va[j] + vb[j];  // fp32, then one rounding to the storage type
    const u32x4 r = rn_gemm::OutVec<T>::pack(va);
    return make_uint4(r[0], r[1], r[2], r[3]);
}

template <typename T, bool ADD>
__global__ __launch_bounds__(kNaBlock) void upsample_nearest_add_kernel(const nearest_args p)
{
    for (uint32_t row = blockIdx.y; row < p.rows; row += gridDim.y) {
        const uint32_t b = row / p.H, y = row - b * p.H;  // uniform: once per row
        const uint32_t iy = nearest_index(y, p.scale_h, p.h);
        const uint4 *top_row = p.top + ((uint64_t)b * p.h + iy) * p.w * p.cpp;
        const uint64_t out_row = (uint64_t)row * p.W * p.cpp;
        for (uint32_t s = blockIdx.x; s < p.spans; s += gridDim.x) {
            const uint32_t x0 = s * p.span;
            const uint32_t px = p.W - x0 < p.span ? p.W - x0 : p.span, n = px * p.cpp;
            const uint64_t base = out_row + (uint64_t)x0 * p.cpp;
            for (uint32_t j0 = threadIdx.x; j0 < n; j0 += kNaChunks) {
                uint4 t[kNaUnroll], l[kNaUnroll];
#pragma unroll
                for (uint32_t u = 0; u < kNaUnroll; ++u) {
                    const uint32_t j = j0 + u * kNaBlock;
                    if (j < n) {
                        const uint32_t dx = rn_gemm::fast_div(j, (int)p.cpp, p.mul_cpp, p.shr_cpp), k = j - dx * p.cpp;
                        const uint32_t ix = nearest_index(x0 + dx, p.scale_w, p.w);
                        t[u] = top_row[(uint64_t)ix * p.cpp + k];
                        if (ADD) l[u] = p.lat[base + j];
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < kNaUnroll; ++u) {
                    const uint32_t j = j0 + u * kNaBlock;
                    if (j < n) p.dst[base + j] = ADD ? add_chunk<T>(l[u], t[u]) : t[u];
                }
            }
        }
    }
}

constexpr int kFpnMaxLevels = 4, kFpnPool = kFpnMaxLevels, kFpnScratch = 2 * kFpnMaxLevels + 1;

}  // namespace

// torchvision's FeaturePyramidNetwork(in_channels_list, a, extra_blocks=LastLevelMaxPool() or None), norm_layer=None
struct rn_fpn {
    rn_ctx *ctx;
    int n, extra, dtype, finalized;
    uint64_t cin[kFpnMaxLevels], a;
    // entries 4 l .. 4 l + 3, level l: the lateral's weight [a,in,1,1] and bias [a], the 3x3's weight [a,a,3,3] and bias [a]
    rn_params params;
    rn_stage_unit lateral[kFpnMaxLevels], layer[kFpnMaxLevels];  // the biases are the epilogues' shifts
    // scratch, per level: the lateral / merged tensor [cap, h, w, a] of the storage type and the 3x3's output
    // [cap, h, w, a] fp32; the pooled coarsest output [cap, hp, wp, a] fp32
    void *inner[kFpnMaxLevels];
    float *outb[kFpnMaxLevels], *poolb;
    uint64_t cap_pix[kFpnMaxLevels + 1];  // pixels a level's tensors hold; the last: the pooled output's (kFpnPool)
};

namespace {

// the scratch tensors for pix[l] pixels of level l and pix[kFpnPool] of the pooled output; returns how many
int fpn_scratch(rn_fpn *f, const uint64_t *pix, rn_scratch_item *list)
{
    int n = 0;
    for (int i = 0; i < f->n; ++i) {
        list[n++] = {&f->inner[i], pix[i] * f->a * rn_elem_size(f->dtype)};
        list[n++] = {(void **)&f->outb[i], pix[i] * f->a * sizeof(float)};
    }
    list[n++] = {(void **)&f->poolb, pix[kFpnPool] * f->a * sizeof(float)};
    return n;
}

}  // namespace

extern "C" {

int rn_upsample_nearest_add_forward_dt(rn_ctx *ctx, int dtype, const void *top_nhwc, uint64_t B, uint64_t h, uint64_t w,
                                       uint64_t C, const void *lat_nhwc, void *dst_nhwc, uint64_t H, uint64_t W)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, dtype == RN_DTYPE_F32 || dtype == RN_DTYPE_BF16, "unknown dtype");
    RN_REQUIRE(ctx, top_nhwc, "top_nhwc is NULL");
    RN_REQUIRE(ctx, dst_nhwc, "dst_nhwc is NULL");
    RN_REQUIRE(ctx, h >= 1 && w >= 1 && H >= 1 && W >= 1, "h, w, H, W must be >= 1");
    const uint64_t es = rn_elem_size(dtype), per = 16 / es;  // elements of a 16-byte chunk
    RN_REQUIRE(ctx, C >= 1 && C < (1ull << 31) && C % per == 0, "C must be a multiple of 16 bytes (and below 2^31)");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(top_nhwc) & 15) == 0, "top_nhwc is off a 16-byte boundary");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(lat_nhwc) & 15) == 0, "lat_nhwc is off a 16-byte boundary");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(dst_nhwc) & 15) == 0, "dst_nhwc is off a 16-byte boundary");
    RN_REQUIRE(ctx, h < (1ull << 31) && w < (1ull << 31) && H < (1ull << 31) && W < (1ull << 31) && B < (1ull << 31) &&
                        h * w < (1ull << 31) && H * W < (1ull << 31) && B * h * w < (1ull << 31) &&
                        B * H * W < (1ull << 31),
               "B * h * w and B * H * W must be below 2^31");
    if (B == 0) return RN_OK;
    const uint64_t top_bytes = B * h * w * C * es, dst_bytes = B * H * W * C * es;
    RN_REQUIRE(ctx, !rn_overlap(dst_nhwc, dst_bytes, top_nhwc, top_bytes), "dst_nhwc overlaps top_nhwc");
    RN_REQUIRE(ctx, !lat_nhwc || lat_nhwc == dst_nhwc || !rn_overlap(dst_nhwc, dst_bytes, lat_nhwc, dst_bytes),
               "dst_nhwc overlaps lat_nhwc partly (it may be lat_nhwc itself)");
    nearest_args p;
    p.top = (const uint4 *)top_nhwc, p.lat = (const uint4 *)lat_nhwc, p.dst = (uint4 *)dst_nhwc;
    p.h = (uint32_t)h, p.w = (uint32_t)w, p.H = (uint32_t)H, p.W = (uint32_t)W, p.rows = (uint32_t)(B * H);
    p.cpp = (uint32_t)(C / per);
    p.span = p.cpp >= kNaChunks ? 1 : kNaChunks / p.cpp;
    p.spans = (uint32_t)rn_ceil_div(W, p.span);
    rn_fast_div(p.cpp, &p.mul_cpp, &p.shr_cpp);
    p.scale_h = (float)h / (float)H, p.scale_w = (float)w / (float)W;
    // at most about 4096 blocks, eight a CU and some to balance; the rest is the kernel's two strides
    const uint32_t gx = p.spans < 2048 ? p.spans : 2048, per_x = 4096 / gx;
    const dim3 grid(gx, p.rows < per_x ? p.rows : per_x);
    if (dtype == RN_DTYPE_BF16) {
        if (lat_nhwc) upsample_nearest_add_kernel<bf16_t, true><<<grid, kNaBlock, 0, ctx->stream>>>(p);
        else upsample_nearest_add_kernel<bf16_t, false><<<grid, kNaBlock, 0, ctx->stream>>>(p);
    } else {
        if (lat_nhwc) upsample_nearest_add_kernel<float, true><<<grid, kNaBlock, 0, ctx->stream>>>(p);
        else upsample_nearest_add_kernel<float, false><<<grid, kNaBlock, 0, ctx->stream>>>(p);
    }
    return rn_after_launch(ctx, "rn_upsample_nearest_add_forward_dt");
}

// ---- the neck -----------------------------------------------------------------------------------------------

int rn_fpn_create(rn_ctx *ctx, rn_fpn **out, uint64_t n_levels, const uint64_t *in_channels, uint64_t out_channels,
                  int extra)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    RN_REQUIRE(ctx, n_levels >= 1 && n_levels <= (uint64_t)kFpnMaxLevels && in_channels,
               "n_levels must be 1..4 (and in_channels not NULL)");
    for (uint64_t i = 0; i < n_levels; ++i)
        RN_REQUIRE(ctx, in_channels[i] >= 64 && in_channels[i] % 64 == 0 && in_channels[i] <= 8192,
                   "every in_channels must be a multiple of 64 (at most 8192)");
    RN_REQUIRE(ctx, out_channels >= 64 && out_channels % 64 == 0 && out_channels <= 1024,
               "out_channels must be a multiple of 64 (at most 1024)");
    RN_REQUIRE(ctx, extra == 0 || extra == 1, "extra must be 0 (none) or 1 (LastLevelMaxPool)");
    rn_fpn *f = (rn_fpn *)calloc(1, sizeof(*f));
    if (!f) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_fpn_create: out of host memory");
    f->ctx = ctx, f->n = (int)n_levels, f->extra = extra, f->a = out_channels, f->dtype = RN_DTYPE_F32;
    for (uint64_t i = 0; i < n_levels; ++i) {  // "inner_blocks.2.0.weight", or "inner_blocks.2.weight": the older spelling
        static const char *const block[2] = {"inner_blocks", "layer_blocks"}, *const part[2] = {"weight", "bias"};
        f->cin[i] = in_channels[i];
        for (int t = 0; t < 4; ++t) {
            char key[RN_PARAM_KEY], alt[RN_PARAM_KEY];
            snprintf(key, sizeof(key), "%s.%d.0.%s", block[t / 2], (int)i, part[t % 2]);
            snprintf(alt, sizeof(alt), "%s.%d.%s", block[t / 2], (int)i, part[t % 2]);
            const uint64_t rows = t % 2 ? 1 : f->a, len = t == 0 ? f->cin[i] : t == 2 ? f->a * 9 : f->a;
            rn_params_add(&f->params, key, alt, rows, len, rows, len, 0.0f);
        }
    }
    *out = f;
    return RN_OK;
}

int rn_fpn_set_dtype(rn_fpn *f, int dtype)
{
    if (!f) return RN_ERR_INVALID;
    RN_REQUIRE(f->ctx, !f->finalized, "the neck is finalized");
    RN_REQUIRE(f->ctx, dtype == RN_DTYPE_F32 || dtype == RN_DTYPE_BF16, "unknown dtype");
    f->dtype = dtype;
    return RN_OK;
}

int rn_fpn_set_tensor(rn_fpn *f, const char *key, const float *host_data, uint64_t numel)
{
    if (!f) return RN_ERR_INVALID;
    return rn_stage_set_tensor(f->ctx, __func__, "the neck", f->finalized, &f->params, key, host_data, numel);
}

int rn_fpn_finalize(rn_fpn *f)
{
    if (!f) return RN_ERR_INVALID;
    rn_ctx *ctx = f->ctx;
    RN_ENTER(ctx);
    if (f->finalized) return RN_OK;
    RN_TRY(rn_stage_all_set(ctx, __func__, &f->params));
    for (int i = 0; i < f->n; ++i) {
        const rn_params_entry *p = &f->params.p[4 * i];
        RN_TRY(rn_stage_pack(ctx, f->dtype, p[0].host, f->cin[i], f->a, 1, p[1].host, NULL, &f->lateral[i]));
        RN_TRY(rn_stage_pack(ctx, f->dtype, p[2].host, f->a, f->a, 3, p[3].host, NULL, &f->layer[i]));
    }
    rn_params_free(&f->params);
    f->finalized = 1;
    return RN_OK;
}

int rn_fpn_destroy(rn_fpn *f)
{
    if (!f) return RN_OK;
    rn_ctx *ctx = f->ctx;
    RN_ENTER(ctx);
    RN_TRY(rn_sync(ctx));
    rn_scratch_item list[kFpnScratch];
    rn_stage_free_list(ctx, list, fpn_scratch(f, f->cap_pix, list));
    rn_params_free(&f->params);
    for (int i = 0; i < f->n; ++i) rn_stage_unit_free(ctx, &f->lateral[i]), rn_stage_unit_free(ctx, &f->layer[i]);
    free(f);
    return RN_OK;
}

int rn_fpn_level_shape(const rn_fpn *f, int level, uint64_t h_in, uint64_t w_in, uint64_t *C, uint64_t *H, uint64_t *W)
{
    if (!f) return RN_ERR_INVALID;
    if (level < 0 || level > f->n || (level == f->n && !f->extra) || h_in == 0 || w_in == 0) return RN_ERR_INVALID;
    const int pool = level == f->n;  // LastLevelMaxPool: kernel 1, stride 2, no padding, on the coarsest output
    if (C) *C = f->a;
    if (H) *H = pool ? (h_in - 1) / 2 + 1 : h_in;
    if (W) *W = pool ? (w_in - 1) / 2 + 1 : w_in;
    return RN_OK;
}

// ---- library-internal (rn_private.h): what the model driver asks of a neck and queues of it ----

int rn_fpn_matches(const rn_fpn *f, const rn_ctx *ctx, int dtype, const char **why)
{
    const char *w = NULL;
    if (!f) w = "the neck is NULL";
    else if (!f->finalized) w = "the neck is not finalized";
    else if (f->ctx->device != ctx->device) w = "the neck's context is on another device than the model's";
    else if (f->dtype != dtype) w = "the neck's storage type (dtype) is not the model's";
    if (why) *why = w;
    return w == NULL;
}

void rn_fpn_dims(const rn_fpn *f, int *n_levels, int *extra, uint64_t *out_channels, uint64_t in_channels[4])
{
    if (n_levels) *n_levels = f->n;
    if (extra) *extra = f->extra;
    if (out_channels) *out_channels = f->a;
    if (in_channels)
        for (int i = 0; i < f->n; ++i) in_channels[i] = f->cin[i];
}

int rn_fpn_reserve(rn_fpn *f, uint64_t images, const uint64_t *h, const uint64_t *w)
{
    const int last = f->n - 1;
    uint64_t want[kFpnMaxLevels + 1] = {};
    want[kFpnPool] = f->extra ? images * ((h[last] - 1) / 2 + 1) * ((w[last] - 1) / 2 + 1) : 0;
    for (int i = 0; i < f->n; ++i) want[i] = images * h[i] * w[i];
    bool fits = true;
    for (int i = 0; i <= kFpnPool; ++i) {
        fits = fits && want[i] <= f->cap_pix[i];
        if (want[i] < f->cap_pix[i]) want[i] = f->cap_pix[i];
    }
    if (fits) return RN_OK;
    rn_scratch_item list[kFpnScratch];
    return rn_stage_grow(f->ctx, "rn_fpn", list, fpn_scratch(f, want, list), f->cap_pix, want, kFpnMaxLevels + 1);
}

void rn_fpn_cost(const rn_fpn *f, int kind, int level, uint64_t B, const uint64_t *h, const uint64_t *w, double *flops,
                 double *bytes)
{
    const double es = (double)rn_elem_size(f->dtype), a = (double)f->a;
    const int l = level < f->n ? level : f->n - 1;
    const double P = (double)(B * h[l] * w[l]), cin = (double)f->cin[l];
    const double Pp = (double)(B * ((h[l] - 1) / 2 + 1) * ((w[l] - 1) / 2 + 1));
    double fl = 0.0, by = 0.0;
    switch (kind) {
    case RN_FPN_INNER: fl = 2.0 * P * cin * a, by = es * (P * (cin + a) + cin * a); break;
    case RN_FPN_TOPDOWN:  // level: the coarser one; the finer one is read and written
        by = es * a * (P + 2.0 * (double)(B * h[l - 1] * w[l - 1]));
        break;
    case RN_FPN_LAYER: fl = 2.0 * P * 9.0 * a * a, by = P * a * (es + 4.0) + es * 9.0 * a * a; break;
    case RN_FPN_POOL: by = 4.0 * a * (P + Pp); break;
    default: by = 8.0 * a * (level == f->n ? Pp : P); break;  // the export
    }
    if (flops) *flops = fl;
    if (bytes) *bytes = by;
}

int rn_fpn_step(rn_fpn *f, rn_ctx *ctx, int kind, int level, const void *x_nhwc, uint64_t img0, uint64_t B,
                const uint64_t *h, const uint64_t *w, float *dst_nchw)
{
    const int dt = f->dtype, last = f->n - 1;
    const uint64_t es = rn_elem_size(f->dtype), a = f->a;
    const uint64_t hp = (h[last] - 1) / 2 + 1, wp = (w[last] - 1) / 2 + 1;
    for (int i = 0; i < f->n; ++i)
        if ((img0 + B) * h[i] * w[i] > f->cap_pix[i]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_fpn: scratch not reserved");
    if (f->extra && (img0 + B) * hp * wp > f->cap_pix[kFpnPool]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_fpn: scratch not reserved");
    const int l = level < f->n ? level : last;
    void *inner = (char *)f->inner[l] + img0 * h[l] * w[l] * a * es;
    float *outb = f->outb[l] + img0 * h[l] * w[l] * a;
    float *poolb = f->extra ? f->poolb + img0 * hp * wp * a : NULL;
    rn_epilogue ep;
    ep.scale = NULL, ep.residual = NULL, ep.relu = 0;
    switch (kind) {
    case RN_FPN_INNER:
        ep.shift = f->lateral[l].shift;
        return rn_conv2d_nhwc_forward_dt(ctx, dt, dt, x_nhwc, inner, f->lateral[l].packed, 1, 1, 0, h[l], w[l], B, f->cin[l], a,
                                         h[l], w[l], &ep);
    case RN_FPN_TOPDOWN: {  // level (the coarser) -> level - 1, in place on the finer lateral
        void *fine = (char *)f->inner[l - 1] + img0 * h[l - 1] * w[l - 1] * a * es;
        return rn_upsample_nearest_add_forward_dt(ctx, dt, inner, B, h[l], w[l], a, fine, fine, h[l - 1], w[l - 1]);
    }
    case RN_FPN_LAYER:
        ep.shift = f->layer[l].shift;
        return rn_conv2d_nhwc_forward_dt(ctx, dt, RN_DTYPE_F32, inner, outb, f->layer[l].packed, 3, 1, 1, h[l], w[l], B, a, a,
                                         h[l], w[l], &ep);
    case RN_FPN_POOL:
        return rn_maxpool2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, outb, poolb, 1, 2, 0, hp, wp, B, a, h[l], w[l]);
    default:
        if (level == f->n) return rn_nhwc_to_nchw_dt(ctx, RN_DTYPE_F32, poolb, dst_nchw, B, a, hp, wp);
        return rn_nhwc_to_nchw_dt(ctx, RN_DTYPE_F32, outb, dst_nchw, B, a, h[l], w[l]);
    }
}

// ---- the pooler behind the neck (rn_roi.hip's kernel on the 3x3 outputs, in place) ----

// ---- one forward of the neck and what runs behind it (rn_private.h: rn_neck_call) ----

namespace {

// what follows the exports, after the kinds of rn_fpn_step.  The RoI heads' kinds are NECK_MASK + the head's slot in
// rn_neck_call (rn_private.h: RN_NECK_*_SLOT): a further head adds its kind here and its slot there, in the same order
enum { NECK_RPN = RN_FPN_EXPORT + 1, NECK_ROI, NECK_BOX, NECK_MASK, NECK_KEYPOINT };
static_assert(NECK_MASK + RN_NECK_KEYPOINT_SLOT == NECK_KEYPOINT, "a RoI head's step kind is NECK_MASK + its slot");

constexpr int kRoiOperands = 3;

// the pooler's buffers as operands: pooled and levels_out are written, rois_dev is read
void roi_operands(const rn_neck_call *c, operand ops[kRoiOperands])
{
    const rn_roi_pool *rp = c->roi;
    ops[0] = {rp->pooled, rp->K * c->a * rp->PH * rp->PW * sizeof(float), "pooled", true, false};
    ops[1] = {rp->levels_out, rp->K * 4, "levels_out", true, false};
    ops[2] = {rp->rois_dev, rp->K * 5 * sizeof(float), "rois_dev", false, false};
}

// the pooler's request against the neck whose level i is an h[i] x w[i] map: every refusal that concerns the pooler
// alone; fills the levels' scales (torchvision's infer_scale) and the thresholds between them
int rn_fpn_roi_check(rn_neck_call *c, rn_ctx *ctx)
{
    const rn_fpn *f = c->fpn;
    const rn_roi_pool *rp = c->roi;
    RN_REQUIRE(ctx, rp->n_levels >= 1 && rp->n_levels <= f->n, "the pooler reads 1 .. n_levels of the neck's levels");
    for (int i = 0; i < rp->n_levels; ++i)
        RN_REQUIRE(ctx, rp->level[i] >= 0 && rp->level[i] < f->n && (i == 0 || rp->level[i] > rp->level[i - 1]),
                   "the pooler's levels must be the neck's (0 .. n_levels - 1, the pool is none), ascending");
    RN_REQUIRE(ctx, rp->image_h >= 1 && rp->image_w >= 1, "image_h and image_w must be >= 1");
    RN_REQUIRE(ctx, rp->PH >= 1 && rp->PH <= 32 && rp->PW >= 1 && rp->PW <= 32, "PH and PW must be 1..32");
    if (rp->sampling_ratio <= 0)
        return rn_set_error(ctx, RN_ERR_UNSUPPORTED, "%s: sampling_ratio <= 0 (adaptive grids) is not carried", __func__);
    RN_REQUIRE(ctx, rp->sampling_ratio <= 4, "sampling_ratio must be 1..4");
    RN_REQUIRE(ctx, rp->aligned == 0 || rp->aligned == 1, "aligned must be 0 or 1");
    RN_REQUIRE(ctx, rp->canonical_scale > 0.0, "canonical_scale must be positive");
    RN_REQUIRE(ctx, rp->K < (1ull << 31), "K must be below 2^31");
    RN_REQUIRE(ctx, rp->K == 0 || rp->rois_dev, "rois_dev is NULL (K > 0)");
    RN_REQUIRE(ctx, rp->K == 0 || rp->pooled, "pooled is NULL (K > 0)");
    operand ops[kRoiOperands];
    roi_operands(c, ops);
    RN_TRY(check_operands(ctx, __func__, ops, kRoiOperands));
    // the power of two nearest the level's height over the image's (infer_scale returns the first of the two axes' scales)
    for (int i = 0; i < rp->n_levels; ++i)
        c->scales[i] = (float)exp2(rint(log2((double)c->h[rp->level[i]] / (double)rp->image_h)));
    if (rn_roi_level_thresholds((uint64_t)rp->n_levels, c->scales, rp->canonical_scale, rp->canonical_level, c->thr) != RN_OK)
        return rn_set_error(ctx, RN_ERR_INVALID, "%s: the level thresholds cannot be formed", __func__);
    return RN_OK;
}

// the pooler of a RoI head's request against the neck: every refusal that concerns it alone; fills the slot's scales (formed
// as rn_fpn_roi_check forms the pooler's) and thresholds
int neck_head_pool_check(const rn_neck_call *c, rn_ctx *ctx, const char *fn, rn_roi_head *s)
{
    const rn_fpn *f = c->fpn;
    const rn_roi_pool_view *v = &s->pool;
    const char *why = NULL;
    if (v->n_levels < 1 || v->n_levels > f->n) why = "pooler reads 1 .. n_levels of the neck's levels";
    for (int i = 0; i < v->n_levels && !why; ++i)
        if (v->level[i] < 0 || v->level[i] >= f->n || (i > 0 && v->level[i] <= v->level[i - 1]))
            why = "pooler's levels must be the neck's (0 .. n_levels - 1, the pool is none), ascending";
    if (!why && v->sampling_ratio <= 0)
        return rn_set_error(ctx, RN_ERR_UNSUPPORTED, "%s: the %s pooler's sampling_ratio <= 0 (adaptive grids) is not carried", fn, s->who);
    if (!why && v->sampling_ratio > 4) why = "pooler's sampling_ratio must be 1..4";
    if (!why && v->aligned != 0 && v->aligned != 1) why = "pooler's aligned must be 0 or 1";
    if (!why && !(v->canonical_scale > 0.0)) why = "pooler's canonical_scale must be positive";
    if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: the %s %s", fn, s->who, why);
    if ((reinterpret_cast<uintptr_t>(v->pooled) & 15) != 0)
        return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s.pooled is off a 16-byte boundary", fn, s->who);
    for (int i = 0; i < v->n_levels; ++i) s->scales[i] = (float)exp2(rint(log2((double)c->h[v->level[i]] / (double)c->image_h)));
    if (rn_roi_level_thresholds((uint64_t)v->n_levels, s->scales, v->canonical_scale, v->canonical_level, s->thr) != RN_OK)
        return rn_set_error(ctx, RN_ERR_INVALID, "%s: the %s pooler's level thresholds cannot be formed", fn, s->who);
    return RN_OK;
}

// a RoI head's stage on the 3x3 outputs of B images, read in place sub0 images into the neck's scratch (level i of the
// head's pooler), on these images' own detection rows
int neck_head_step(const rn_neck_call *c, rn_ctx *ctx, const rn_roi_head *s, uint64_t sub0, uint64_t img0, uint64_t B)
{
    const rn_fpn *f = c->fpn;
    const void *maps[kFpnMaxLevels];
    uint64_t hs[kFpnMaxLevels], ws[kFpnMaxLevels];
    for (int i = 0; i < s->pool.n_levels; ++i) {
        const int l = s->pool.level[i];
        if ((sub0 + B) * c->h[l] * c->w[l] > f->cap_pix[l]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_fpn: scratch not reserved");
        maps[i] = f->outb[l] + sub0 * c->h[l] * c->w[l] * f->a, hs[i] = c->h[l], ws[i] = c->w[l];
    }
    return rn_roi_head_stage(s, ctx, maps, hs, ws, c->images, sub0, img0, B, c->det_req->detections_per_img, c->det_req->out.boxes,
                             c->det_req->out.labels, c->image_h, c->image_w);
}

// The pooler's launch on ctx for the B images from the caller's image img0 on, whose 3x3 outputs start sub0 images
// into the neck's scratch, on rows row0 .. row0 + rows of rois_dev, pooled and levels_out.  A window of the whole
// call's rows leaves the rows of other images to their parts' launches and writes the invalid rows (zeros, level -1)
// where write_invalid; the chain gives a part its own rows, every one of which it writes.
int neck_roi_step(const rn_neck_call *c, rn_ctx *ctx, uint64_t sub0, uint64_t img0, uint64_t B, uint64_t row0, uint64_t rows,
                  int write_invalid)
{
    const rn_fpn *f = c->fpn;
    const rn_roi_pool *rp = c->roi;
    const void *maps[kFpnMaxLevels];
    uint64_t hs[kFpnMaxLevels], ws[kFpnMaxLevels];
    if (rows == 0) return RN_OK;
    for (int i = 0; i < rp->n_levels; ++i) {
        const int l = rp->level[i];
        if ((sub0 + B) * c->h[l] * c->w[l] > f->cap_pix[l]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_fpn: scratch not reserved");
        maps[i] = f->outb[l] + sub0 * c->h[l] * c->w[l] * f->a, hs[i] = c->h[l], ws[i] = c->w[l];
    }
    return rn_roi_align_window(ctx, RN_DTYPE_F32, (uint64_t)rp->n_levels, maps, hs, ws, c->scales, c->thr, c->images, img0, B,
                               write_invalid, f->a, rp->rois_dev + row0 * 5, rows, rp->PH, rp->PW, rp->sampling_ratio,
                               rp->aligned, rp->pooled + row0 * f->a * rp->PH * rp->PW,
                               rp->levels_out ? rp->levels_out + row0 : NULL);
}

// the rpn's stage on the neck's 3x3 outputs and pooled level of B images, read in place sub0 images into the scratch
int neck_rpn_step(const rn_neck_call *c, rn_ctx *ctx, uint64_t sub0, uint64_t img0, uint64_t B)
{
    const rn_fpn *f = c->fpn;
    const float *lv[kFpnMaxLevels + 1];
    for (int i = 0; i < c->n + c->extra; ++i) {
        if ((sub0 + B) * c->hl[i] * c->wl[i] > (i < c->n ? f->cap_pix[i] : f->cap_pix[kFpnPool]))
            return rn_set_error(ctx, RN_ERR_INVALID, "rn_fpn: scratch not reserved");
        lv[i] = (i < c->n ? f->outb[i] : f->poolb) + sub0 * c->hl[i] * c->wl[i] * f->a;
    }
    return rn_rpn_step(c->rpn, ctx, lv, sub0, img0, B, c->hl, c->wl, c->image_h, c->image_w, c->rpn_req);
}

// step `step` of what follows the laterals: its kind and level (untouched when there is no such step); returns how
// many steps there are.  The order of a forward is this function and nothing else.
int neck_step_at(const rn_neck_call *c, int step, int *kind, int *level)
{
    int at = 0;
    const auto put = [&](int k, int l) {
        if (at++ == step) *kind = k, *level = l;
    };
    for (int j = c->n - 1; j >= 1; --j) put(RN_FPN_TOPDOWN, j);
    for (int j = 0; j < c->n; ++j)
        if (c->layer_runs[j]) put(RN_FPN_LAYER, j);
    if (c->pool) put(RN_FPN_POOL, c->n - 1);
    for (int j = 0; j < c->n + c->extra; ++j)
        if (c->out[j]) put(RN_FPN_EXPORT, j);
    if (c->rpn) put(NECK_RPN, 0);
    if (c->roi && c->roi->K > 0) put(NECK_ROI, 0);
    if (c->box_head) put(NECK_BOX, 0);
    for (int i = 0; i < RN_NECK_HEADS; ++i)
        if (c->head[i].tower) put(NECK_MASK + i, 0);
    return at;
}

}  // namespace

const char *rn_fpn_op_name(const rn_fpn *f, int kind, int level)
{
    static const char *const names[4][kFpnMaxLevels] = {{"fpn_inner0", "fpn_inner1", "fpn_inner2", "fpn_inner3"},
                                                        {NULL, "fpn_topdown1", "fpn_topdown2", "fpn_topdown3"},
                                                        {"fpn_layer0", "fpn_layer1", "fpn_layer2", "fpn_layer3"},
                                                        {"fpn_export0", "fpn_export1", "fpn_export2", "fpn_export3"}};
    if (kind == RN_FPN_POOL) return "fpn_pool";
    if (kind == RN_FPN_EXPORT) return level == f->n ? "fpn_export_pool" : names[3][level];
    return names[kind][level];
}

int rn_neck_check(rn_neck_call *c, rn_ctx *ctx, const char *fn, const rn_operand *others, int n_others)
{
    static const char *const level_names[kFpnMaxLevels + 1] = {"level[0]", "level[1]", "level[2]", "level[3]", "level[4]"};
    const rn_fpn *f = c->fpn;
    const rn_roi_pool *rp = c->roi;
    const uint64_t B = c->images;
    const char *why = NULL;
    if (!rn_fpn_matches(f, ctx, f ? f->dtype : 0, &why)) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
    c->n = f->n, c->extra = f->extra, c->a = f->a;
    const int n = f->n, n_out = n + f->extra;
    bool wanted = rp != NULL || c->rpn != NULL;
    for (int i = 0; i < n_out; ++i) {
        const int l = i < n ? i : n - 1;
        RN_TRY(rn_fpn_level_shape(f, i, c->h[l], c->w[l], NULL, &c->hl[i], &c->wl[i]));
        if ((reinterpret_cast<uintptr_t>(c->out[i]) & 3) != 0)
            return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s of the outputs must be 4-byte aligned (it is off a 4-byte boundary)",
                                fn, level_names[i]);
        wanted = wanted || c->out[i];
    }
    if (!wanted) return rn_set_error(ctx, RN_ERR_INVALID, "%s: nothing wanted (every output level is NULL)", fn);
    if (rp) RN_TRY(rn_fpn_roi_check(c, ctx));
    if (c->rpn) {  // the rpn behind the neck reads every level's 3x3 output and the pooled level in place
        if (!rn_rpn_matches(c->rpn, ctx, f->a, (uint64_t)n_out, &why)) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
        RN_TRY(rn_rpn_check(c->rpn, ctx, c->rpn_req, B, c->hl, c->wl, c->image_h, c->image_w));
    }
    // the chain: the pooler may read the RoIs this call writes, and only those
    c->chain = c->rpn && rp && rp->K > 0 && rp->rois_dev == c->rpn_req->out.rois && rp->K == B * c->rpn_req->post_nms_top_n;
    if (c->box_head) {  // behind the chained pooler, on its rows
        if (!c->rpn || !c->rpn_req) why = "the box head needs the rpn and its request";
        else if (!rp || rp->K == 0) why = "the box head needs the pooler";
        else if (!c->chain) why = "the box head needs the chained pooler (rois_dev == req->out.rois, K == B * post_nms_top_n)";
        else if ((reinterpret_cast<uintptr_t>(rp->pooled) & 15) != 0) why = "pooled is off a 16-byte boundary";
        else rn_box_head_matches(c->box_head, ctx, f->a * rp->PH * rp->PW, &why);
        if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
        RN_TRY(rn_box_head_check(c->box_head, ctx, c->det_req, B, c->rpn_req->post_nms_top_n, c->image_h, c->image_w));
    }
    for (int i = 0; i < RN_NECK_HEADS; ++i) {  // behind the box head, on the detections it writes
        rn_roi_head *s = &c->head[i];
        if (!s->tower) continue;
        if (!c->box_head || !c->det_req) why = "head needs the box head and its request";
        else if (!c->det_req->out.boxes || !c->det_req->out.labels) why = "head needs boxes and labels of the detect request";
        else if (!s->req) why = "request is NULL";
        else rn_roi_tower_matches(s->tower, ctx, f->a, &why);
        if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: the %s %s", fn, s->who, why);
        RN_TRY(s->check(s, ctx, fn, B * c->det_req->detections_per_img, 1, c->image_h, c->image_w));
        RN_TRY(neck_head_pool_check(c, ctx, fn, s));
    }
    c->pool = f->extra && (c->out[n] || c->rpn);
    for (int i = 0; i < n; ++i) c->layer_runs[i] = c->out[i] || (c->pool && i == n - 1) || c->rpn;
    if (rp && rp->K > 0)
        for (int i = 0; i < rp->n_levels; ++i) c->layer_runs[rp->level[i]] = 1;
    // the operand matrix: every group against every group before it
    operand levels[kFpnMaxLevels + 1], roi[kRoiOperands], rpn[RN_RPN_OPERANDS], box[RN_BOX_HEAD_OPERANDS];
    operand head[RN_NECK_HEADS][RN_ROI_HEAD_OPERANDS];
    for (int i = 0; i < n_out; ++i) levels[i] = {c->out[i], B * f->a * c->hl[i] * c->wl[i] * sizeof(float), level_names[i], true, false};
    if (rp) roi_operands(c, roi);
    if (c->rpn) rn_rpn_operands(c->rpn, c->rpn_req, B, rpn);
    if (c->box_head) rn_box_head_operands(c->box_head, c->det_req, B, c->rpn_req->post_nms_top_n, box);
    for (int i = 0; i < RN_NECK_HEADS; ++i) {
        const rn_roi_head *s = &c->head[i];
        if (!s->tower) continue;
        s->operands(s, B * c->det_req->detections_per_img, c->image_h, c->image_w, head[i]);
        RN_TRY(check_operands(ctx, fn, head[i], RN_ROI_HEAD_OPERANDS));
    }
    if (c->chain) roi[2].ptr = NULL;  // the one exception: rois_dev IS the rpn's out.rois, which stands for it below
    rn_operand_group groups[5 + RN_NECK_HEADS] = {{others, n_others},
                                        {levels, n_out},
                                        {roi, rp ? kRoiOperands : 0},
                                        {rpn, c->rpn ? RN_RPN_OPERANDS : 0},
                                        {box, c->box_head ? RN_BOX_HEAD_OPERANDS : 0}};
    for (int i = 0; i < RN_NECK_HEADS; ++i) groups[5 + i] = {head[i], c->head[i].tower ? RN_ROI_HEAD_OPERANDS : 0};
    return check_operand_groups(ctx, fn, groups, 5 + RN_NECK_HEADS);
}

int rn_neck_reserve(const rn_neck_call *c, uint64_t images_at_once)
{
    RN_TRY(rn_fpn_reserve(c->fpn, images_at_once, c->h, c->w));
    if (c->rpn) RN_TRY(rn_rpn_reserve(c->rpn, images_at_once, c->hl, c->wl, c->rpn_req->pre_nms_top_n));
    if (c->box_head) RN_TRY(rn_box_head_reserve(c->box_head, images_at_once, c->rpn_req->post_nms_top_n));
    for (int i = 0; i < RN_NECK_HEADS; ++i)
        if (c->head[i].tower) RN_TRY(rn_roi_tower_reserve(c->head[i].tower, images_at_once * c->det_req->detections_per_img, 1));
    return RN_OK;
}

int rn_neck_plan(const rn_neck_call *c, uint64_t B, int step, const char **op, const char **layer, double *flops, double *bytes)
{
    int kind = -1, level = 0;
    const int steps = neck_step_at(c, step, &kind, &level);
    if (kind < 0) return steps;
    const rn_roi_pool *rp = c->roi;
    const uint64_t post = c->rpn ? c->rpn_req->post_nms_top_n : 0;
    const char *name = NULL, *lay = "fpn";
    double fl = 0.0, by = 0.0;
    switch (kind) {
    case NECK_RPN:  // 2 L + 3 launches under one record
        name = "rpn_stage", lay = "rpn";
        by = (double)(B * (uint64_t)(c->n + c->extra) * c->rpn_req->pre_nms_top_n) * 25.0;
        break;
    case NECK_ROI:
        // bytes: the outputs only.  What the RoIs gather is several times that (profiles/roi_align) but depends on every
        // box's size against its level, which the host does not look at: the record's GB/s is the OUTPUT rate
        name = "roi_align";
        if (c->chain) {
            by = (double)(B * post * c->a * rp->PH * rp->PW) * 4.0;
        } else {
            const double outs = (double)(rp->K * c->a * rp->PH * rp->PW);
            const double share = (double)B / (double)c->images;  // the RoIs are taken as spread evenly over the images
            const double taps = 4.0 * (double)(rp->sampling_ratio * rp->sampling_ratio);
            fl = share * outs * 2.0 * taps, by = share * outs * 4.0;
        }
        break;
    case NECK_BOX:  // three contractions and three launches under one record
        name = "box_stage", lay = "roi_heads";
        by = (double)(B * post * (c->a * rp->PH * rp->PW)) * 4.0;
        break;
    case NECK_MASK:      // the RoI former, the pooler, the contractions and the head's own launches (the mask head's predict
    case NECK_KEYPOINT: {  // and paste, the keypoint head's predict) under one record
        const rn_roi_head *s = &c->head[kind - NECK_MASK];
        name = s->stage, lay = "roi_heads";
        by = (double)(B * c->det_req->detections_per_img * s->tower->M * s->tower->M * c->a) * 4.0;
        break;
    }
    default:
        name = rn_fpn_op_name(c->fpn, kind, level);
        rn_fpn_cost(c->fpn, kind, level, B, c->h, c->w, &fl, &by);
    }
    if (op) *op = name;
    if (layer) *layer = lay;
    if (flops) *flops = fl;
    if (bytes) *bytes = by;
    return steps;
}

int rn_neck_step(const rn_neck_call *c, rn_ctx *ctx, int step, uint64_t sub0, uint64_t img0, uint64_t B)
{
    int kind = -1, level = 0;
    neck_step_at(c, step, &kind, &level);
    const rn_roi_pool *rp = c->roi;
    const uint64_t post = c->rpn ? c->rpn_req->post_nms_top_n : 0;
    switch (kind) {
    case -1: return rn_set_error(ctx, RN_ERR_INVALID, "rn_neck_step: no such step");
    case NECK_RPN: return neck_rpn_step(c, ctx, sub0, img0, B);
    case NECK_ROI:
        if (c->chain) return neck_roi_step(c, ctx, sub0, img0, B, img0 * post, B * post, 1);  // this part's own proposals
        return neck_roi_step(c, ctx, sub0, img0, B, 0, rp->K, img0 == 0);
    case NECK_BOX: {  // this part's own rows, behind its own pooler launch
        const uint64_t feat = c->a * rp->PH * rp->PW, row0 = img0 * post;
        return rn_box_head_step(c->box_head, ctx, rp->pooled + row0 * feat, rp->rois_dev + row0 * 5, sub0, img0, B, post,
                                c->image_h, c->image_w, c->det_req);
    }
    case NECK_MASK:
    case NECK_KEYPOINT: return neck_head_step(c, ctx, &c->head[kind - NECK_MASK], sub0, img0, B);
    case RN_FPN_EXPORT:  // into the caller's buffer from image img0 on
        return rn_fpn_step(c->fpn, ctx, kind, level, NULL, sub0, B, c->h, c->w, c->out[level] + img0 * c->a * c->hl[level] * c->wl[level]);
    default: return rn_fpn_step(c->fpn, ctx, kind, level, NULL, sub0, B, c->h, c->w, NULL);
    }
}

namespace {

// a refusal of fpn_forward names the entry point that was called
#define FPN_REQUIRE(cond, msg)                                                       \
    do {                                                                             \
        if (!(cond)) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, (msg)); \
    } while (0)

// the stand-alone family (fn names the entry point): its own refusals -- the maps, their boundary, the 2^31 limit --
// then the shared check, the reserve, the laterals and the steps
int fpn_forward(const char *fn, rn_neck_call *c, const void *const *x_nhwc, const uint64_t *h, const uint64_t *w)
{
    static float *const none[kFpnMaxLevels + 1] = {NULL, NULL, NULL, NULL, NULL};
    static const char *const map_names[kFpnMaxLevels] = {"x_nhwc[0]", "x_nhwc[1]", "x_nhwc[2]", "x_nhwc[3]"};
    rn_fpn *f = c->fpn;
    if (!f) return RN_ERR_INVALID;
    rn_ctx *ctx = f->ctx;
    RN_ENTER(ctx);
    FPN_REQUIRE(f->finalized, "the neck is not finalized");
    FPN_REQUIRE(x_nhwc && h && w && (c->out || c->roi || c->rpn), "x_nhwc, h, w or out_nchw is NULL");
    if (!c->out) c->out = none;
    const uint64_t B = c->images;
    operand maps[kFpnMaxLevels];
    for (int i = 0; i < f->n; ++i) {
        FPN_REQUIRE(x_nhwc[i], "a level's map is NULL");
        FPN_REQUIRE((reinterpret_cast<uintptr_t>(x_nhwc[i]) & 15) == 0, "a level's map is off a 16-byte boundary");
        FPN_REQUIRE(h[i] >= 1 && w[i] >= 1, "h and w must be >= 1");
        FPN_REQUIRE(h[i] < (1ull << 31) && w[i] < (1ull << 31) && B < (1ull << 31) && B * h[i] * w[i] < (1ull << 31),
                    "B * h * w must be below 2^31");
        c->h[i] = h[i], c->w[i] = w[i];
        maps[i] = {x_nhwc[i], B * h[i] * w[i] * f->cin[i] * rn_elem_size(f->dtype), map_names[i], false, false};
    }
    RN_TRY(rn_neck_check(c, ctx, fn, maps, f->n));
    if (B == 0) return RN_OK;
    RN_TRY(rn_neck_reserve(c, B));
    const int saved_layout = ctx->layout;
    ctx->layout = RN_LAYOUT_NHWC;
    const int steps = rn_neck_plan(c, B, -1, NULL, NULL, NULL, NULL);
    int st = RN_OK;
    for (int i = 0; i < f->n && st == RN_OK; ++i) st = rn_fpn_step(f, ctx, RN_FPN_INNER, i, x_nhwc[i], 0, B, h, w, NULL);
    for (int s = 0; s < steps && st == RN_OK; ++s) st = rn_neck_step(c, ctx, s, 0, 0, B);
    ctx->layout = saved_layout;
    return st;
}

#undef FPN_REQUIRE

}  // namespace

int rn_fpn_forward(rn_fpn *f, const void *const *x_nhwc, uint64_t B, const uint64_t *h, const uint64_t *w,
                   float *const *out_nchw)
{
    rn_neck_call c = {};
    c.fpn = f, c.out = out_nchw, c.images = B;
    return fpn_forward(__func__, &c, x_nhwc, h, w);
}

int rn_fpn_forward_rois(rn_fpn *f, const void *const *x_nhwc, uint64_t B, const uint64_t *h, const uint64_t *w,
                        float *const *out_nchw, const rn_roi_pool *rois)
{
    rn_neck_call c = {};
    c.fpn = f, c.out = out_nchw, c.images = B, c.roi = rois;
    if (f && !rois) return rn_set_error(f->ctx, RN_ERR_INVALID, "%s: rois is NULL", __func__);
    return fpn_forward(__func__, &c, x_nhwc, h, w);
}

int rn_fpn_forward_proposals(rn_fpn *f, rn_rpn *rpn, const void *const *x_nhwc, uint64_t B, const uint64_t *h, const uint64_t *w,
                             float *const *out_nchw, uint64_t image_h, uint64_t image_w, const rn_rpn_request *req,
                             const rn_roi_pool *rois)
{
    rn_neck_call c = {};
    c.fpn = f, c.out = out_nchw, c.images = B, c.roi = rois, c.rpn = rpn, c.rpn_req = req, c.image_h = image_h, c.image_w = image_w;
    if (f && !rpn) return rn_set_error(f->ctx, RN_ERR_INVALID, "%s: rpn is NULL", __func__);
    if (f && !req) return rn_set_error(f->ctx, RN_ERR_INVALID, "%s: req is NULL", __func__);
    return fpn_forward(__func__, &c, x_nhwc, h, w);
}

int rn_fpn_forward_detections(rn_fpn *f, rn_rpn *rpn, rn_box_head *bh, const void *const *x_nhwc, uint64_t B, const uint64_t *h,
                              const uint64_t *w, float *const *out_nchw, uint64_t image_h, uint64_t image_w,
                              const rn_rpn_request *req, const rn_roi_pool *rois, const rn_detect_request *det_req)
{
    rn_neck_call c = {};
    c.fpn = f, c.out = out_nchw, c.images = B, c.roi = rois, c.rpn = rpn, c.rpn_req = req, c.image_h = image_h, c.image_w = image_w;
    c.box_head = bh, c.det_req = det_req;
    if (f && (!rpn || !req)) return rn_set_error(f->ctx, RN_ERR_INVALID, "%s: rpn or req is NULL", __func__);
    if (f && (!bh || !det_req)) return rn_set_error(f->ctx, RN_ERR_INVALID, "%s: the box head or its request is NULL", __func__);
    return fpn_forward(__func__, &c, x_nhwc, h, w);
}

int rn_fpn_forward_masks(rn_fpn *f, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh, const void *const *x_nhwc, uint64_t B,
                         const uint64_t *h, const uint64_t *w, float *const *out_nchw, uint64_t image_h, uint64_t image_w,
                         const rn_rpn_request *req, const rn_roi_pool *rois, const rn_detect_request *det_req,
                         const rn_mask_request *mask_req)
{
    rn_neck_call c = {};
    c.fpn = f, c.out = out_nchw, c.images = B, c.roi = rois, c.rpn = rpn, c.rpn_req = req, c.image_h = image_h, c.image_w = image_w;
    c.box_head = bh, c.det_req = det_req;
    rn_mask_head_slot(mh, mask_req, &c.head[RN_NECK_MASK_SLOT]);
    if (f && (!rpn || !req)) return rn_set_error(f->ctx, RN_ERR_INVALID, "%s: rpn or req is NULL", __func__);
    if (f && !mh) return rn_set_error(f->ctx, RN_ERR_INVALID, "%s: the mask head is NULL", __func__);
    return fpn_forward(__func__, &c, x_nhwc, h, w);
}

int rn_fpn_forward_keypoints(rn_fpn *f, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh, rn_keypoint_head *kh, const void *const *x_nhwc,
                             uint64_t B, const uint64_t *h, const uint64_t *w, float *const *out_nchw, uint64_t image_h,
                             uint64_t image_w, const rn_rpn_request *req, const rn_roi_pool *rois, const rn_detect_request *det_req,
                             const rn_mask_request *mask_req, const rn_keypoint_request *kp_req)
{
    rn_neck_call c = {};
    c.fpn = f, c.out = out_nchw, c.images = B, c.roi = rois, c.rpn = rpn, c.rpn_req = req, c.image_h = image_h, c.image_w = image_w;
    c.box_head = bh, c.det_req = det_req;
    rn_mask_head_slot(mh, mask_req, &c.head[RN_NECK_MASK_SLOT]), rn_keypoint_head_slot(kh, kp_req, &c.head[RN_NECK_KEYPOINT_SLOT]);
    if (f && (!rpn || !req)) return rn_set_error(f->ctx, RN_ERR_INVALID, "%s: rpn or req is NULL", __func__);
    if (f && !kh) return rn_set_error(f->ctx, RN_ERR_INVALID, "%s: the keypoint head is NULL", __func__);
    return fpn_forward(__func__, &c, x_nhwc, h, w);
}

}  // extern "C"
