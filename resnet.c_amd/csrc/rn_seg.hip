// Semantic segmentation: the bilinear upsample of per-pixel class scores with an optional fused argmax
// (rn_upsample_bilinear_forward) and torchvision's FCNHead as an object over the library's own convolutions
// (rn_seg_head_*).  The reference classifies whole images only; nothing here has a counterpart in it.
#include <stdlib.h>
#include <string.h>

#include "rn_internal.h"
#include "rn_private.h"

// The upsample's arithmetic is a contract, operation by operation (rn_hip.h): no product of this file is fused into
// an add.  (HIP's __fmul_rn / __fadd_rn are plain operators in a header compiled with contraction on: after
// inlining they fuse like any other, so the kernel writes plain operators under this pragma instead.)
#pragma clang fp contract(off)

namespace {

// ---- the upsample kernel ----------------------------------------------------------------------------------
// One block: kSegTY output rows x kSegTX output columns of one image, 256 threads = 16 rows of 16 lanes, every
// lane a run of four consecutive output X (lanes adjacent along W).  The source pixels the tile reads -- rows
// y0(first row) .. y1(last row), columns likewise, all `classes` channels -- are staged in LDS once, pixel-major
// with an odd pitch (classes | 1), from 16-byte loads along the channels.  A tile whose footprint does not fit
// the LDS the launch was given (shrinking, or identity on a large map) reads the source from global memory
// instead: the same arithmetic, merely correct.  A thread then walks the channels: four outputs per channel from
// the contract's fp32 operations, none fused; the running maximum and its index stay in registers; scores go to
// the channel's NCHW plane.
// Stores follow rn_nhwc_to_nchw_dt's rule: 16 bytes wherever four consecutive outputs share an aligned 16 bytes of
// dst, whatever W and the address of dst are.  The thread's run is fixed (the argmax needs that), so an aligned
// quad that starts s = 1..3 floats into the run takes its last s values from the next lane (one __shfl_down per
// value); the run's first s values then belong to the previous lane's quad.  Scalars remain at the ends of a
// tile row: where no previous lane or no full quad exists.  Labels do the same with bytes and 4-byte words.
constexpr int kSegTX = 64, kSegTY = 16;
constexpr uint32_t kSegLdsCap = 32 * 1024;  // bytes of LDS a launch asks for at most

// the contract's source coordinate of output o: index pair and the weight of the second
__device__ inline void seg_coord(uint32_t o, float scale, uint32_t n_in, uint32_t *i0, uint32_t *i1, float *l1)
{
    const float c = (float)o + 0.5f;
    float s = scale * c - 0.5f;
    s = s > 0.0f ? s : 0.0f;
    uint32_t a = (uint32_t)(int)s;
    if (a > n_in - 1) a = n_in - 1;
    *i0 = a;
    *i1 = a + 1 < n_in ? a + 1 : n_in - 1;
    *l1 = s - (float)a;
}

struct seg_args {
    const float *src;
    float *scores;
    uint8_t *labels;
    uint32_t h, w, classes, cs, H, W, tiles_x;
    float scale_h, scale_w;
    uint32_t lds_floats;
};

// the channel walk of one thread.  v: element (row 0, column 0, channel 0) of what the offsets index (the LDS
// tile or the image in global memory); oy / ox: float offsets of the two rows and of the 2 x 4 columns
template <bool SCORES, bool LABELS, typename O>  // O: uint32_t inside the LDS tile, uint64_t inside an image
__device__ inline void seg_walk(const seg_args &p, const float *v, O oy0, O oy1, float a0, float a1,
                                const O (&ox0)[4], const O (&ox1)[4], const float (&b0)[4],
                                const float (&b1)[4], uint64_t img, uint32_t Y, bool row_ok, uint32_t X0, uint32_t Xend,
                                uint32_t q)
{
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t arg[4] = {0, 0, 0, 0};
    const bool nb_ok = q < 15;  // lane + 1 holds the next run of the same tile row
    const uint64_t HW = (uint64_t)p.H * p.W;
    for (uint32_t c = 0; c < p.classes; ++c) {
        const float *r0 = v + oy0 + c, *r1 = v + oy1 + c;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float top = b0[e] * r0[ox0[e]] + b1[e] * r0[ox1[e]];
            const float bot = b0[e] * r1[ox0[e]] + b1[e] * r1[ox1[e]];
            o[e] = a0 * top + a1 * bot;
            if (LABELS) {
                if (c == 0) best[e] = o[e];
                else if (o[e] > best[e]) best[e] = o[e], arg[e] = c;
            }
        }
        if (SCORES) {
            float *row = p.scores + (img * p.classes + c) * HW + (uint64_t)Y * p.W;  // (c, Y, 0)
            const uint32_t s = (0u - (uint32_t)(reinterpret_cast<uintptr_t>(row + X0) >> 2)) & 3;  // floats to the aligned quad
            const float n0 = __shfl_down(o[0], 1), n1 = __shfl_down(o[1], 1), n2 = __shfl_down(o[2], 1);
            if (row_ok) {
                if (s == 0) {
                    if (X0 + 3 < Xend) {
                        *reinterpret_cast<float4 *>(row + X0) = make_float4(o[0], o[1], o[2], o[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (X0 + e < Xend) row[X0 + e] = o[e];
                    }
                } else {
                    const bool prev_full = q > 0 && X0 + s - 1 < Xend;  // the previous lane's quad ends at X0 + s - 1
                    const bool full = nb_ok && X0 + s + 3 < Xend;
#pragma unroll
                    for (int e = 0; e < 3; ++e)
                        if (!prev_full && (uint32_t)e < s && X0 + e < Xend) row[X0 + e] = o[e];
                    if (full) {
                        float4 t;
                        if (s == 1) t = make_float4(o[1], o[2], o[3], n0);
                        else if (s == 2) t = make_float4(o[2], o[3], n0, n1);
                        else t = make_float4(o[3], n0, n1, n2);
                        *reinterpret_cast<float4 *>(row + X0 + s) = t;
                    } else {
#pragma unroll
                        for (int e = 1; e < 4; ++e)
                            if ((uint32_t)e >= s && X0 + e < Xend) row[X0 + e] = o[e];
                    }
                }
            }
        }
    }
    if (LABELS) {
        uint8_t *row = p.labels + img * HW + (uint64_t)Y * p.W;
        const uint32_t s = (0u - (uint32_t)reinterpret_cast<uintptr_t>(row + X0)) & 3;  // bytes to the aligned word
        const uint32_t mine = arg[0] | arg[1] << 8 | arg[2] << 16 | arg[3] << 24;
        const uint32_t next = __shfl_down(mine, 1);
        if (row_ok) {
            const bool prev_full = q > 0 && X0 + s - 1 < Xend;
            const bool full = (s == 0 || nb_ok) && X0 + s + 3 < Xend;
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (!prev_full && (uint32_t)e < s && X0 + e < Xend) row[X0 + e] = (uint8_t)arg[e];
            if (full) {
                const uint64_t both = (uint64_t)next << 32 | mine;
                *reinterpret_cast<uint32_t *>(row + X0 + s) = (uint32_t)(both >> (8 * s));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((uint32_t)e >= s && X0 + e < Xend) row[X0 + e] = (uint8_t)arg[e];
            }
        }
    }
}

template <bool SCORES, bool LABELS>
__global__ __launch_bounds__(256) void upsample_bilinear_kernel(const seg_args p)
{
    extern __shared__ float tile[];  // [rows][cols][classes | 1] of the tile's source pixels
    const uint32_t q = threadIdx.x & 15, r = threadIdx.x >> 4;
    const uint32_t by = blockIdx.x / p.tiles_x, bx = blockIdx.x - by * p.tiles_x;
    const uint64_t img = blockIdx.y;
    const uint32_t Xt = bx * kSegTX, Yt = by * kSegTY;
    const uint32_t Xend = p.W - Xt < (uint32_t)kSegTX ? p.W : Xt + kSegTX;
    const uint32_t Yend = p.H - Yt < (uint32_t)kSegTY ? p.H : Yt + kSegTY;
    // the tile's footprint in the source: the coordinate is monotonic in the output index
    uint32_t ys, ye, xs, xe, u;
    float f;
    seg_coord(Yt, p.scale_h, p.h, &ys, &u, &f);
    seg_coord(Yend - 1, p.scale_h, p.h, &u, &ye, &f);
    seg_coord(Xt, p.scale_w, p.w, &xs, &u, &f);
    seg_coord(Xend - 1, p.scale_w, p.w, &u, &xe, &f);
    const uint32_t nr = ye - ys + 1, nc = xe - xs + 1, pitch = p.classes | 1;
    const bool staged = (uint64_t)nr * nc * pitch <= (uint64_t)p.lds_floats;  // the same for the whole block
    const float *image = p.src + img * p.h * p.w * p.cs;
    if (staged) {
        const uint32_t c4 = (p.classes + 3) / 4, items = nr * nc * c4;  // 4 * c4 <= cs: cs % 4 == 0, cs >= classes
        for (uint32_t i = threadIdx.x; i < items; i += 256) {
            const uint32_t pix = i / c4, k = i - pix * c4, pr = pix / nc, pc = pix - pr * nc;
            const float4 t = *reinterpret_cast<const float4 *>(image + ((uint64_t)(ys + pr) * p.w + xs + pc) * p.cs + 4 * k);
            const float e[4] = {t.x, t.y, t.z, t.w};
            float *d = tile + pix * pitch + 4 * k;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * k + j < p.classes) d[j] = e[j];
        }
        __syncthreads();
    }
    // rows and columns past the image repeat its last ones: every lane computes (the shuffles want all of them)
    // and reads inside the footprint; their stores are dropped
    const uint32_t Y = Yt + r, X0 = Xt + 4 * q;
    const bool row_ok = Y < Yend;
    uint32_t y0, y1, x0[4], x1[4];
    float a0, a1, b0[4], b1[4];
    seg_coord(row_ok ? Y : Yend - 1, p.scale_h, p.h, &y0, &y1, &a1);
    a0 = 1.0f - a1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        seg_coord(X0 + e < Xend ? X0 + e : Xend - 1, p.scale_w, p.w, &x0[e], &x1[e], &b1[e]);
        b0[e] = 1.0f - b1[e];
    }
    if (staged) {
        const uint32_t rs = nc * pitch;  // floats from a row of the tile to the next
        uint32_t ox0[4], ox1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ox0[e] = (x0[e] - xs) * pitch, ox1[e] = (x1[e] - xs) * pitch;
        seg_walk<SCORES, LABELS, uint32_t>(p, tile, (y0 - ys) * rs, (y1 - ys) * rs, a0, a1, ox0, ox1, b0, b1, img, Y,
                                           row_ok, X0, Xend, q);
    } else {
        const uint64_t rs = (uint64_t)p.w * p.cs;
        uint64_t ox0[4], ox1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ox0[e] = (uint64_t)x0[e] * p.cs, ox1[e] = (uint64_t)x1[e] * p.cs;
        seg_walk<SCORES, LABELS, uint64_t>(p, image, y0 * rs, y1 * rs, a0, a1, ox0, ox1, b0, b1, img, Y, row_ok, X0, Xend,
                                           q);
    }
}

// source rows (columns) a tile of `t` outputs can touch at this scale, with room for the rounding of the coordinate;
// an estimate only: the kernel measures its footprint and stages it when it fits what the launch was given
uint64_t seg_span(float scale, uint64_t t, uint64_t n_in)
{
    const uint64_t s = (uint64_t)(scale * (float)(t - 1)) + 3;
    return s < n_in ? s : n_in;
}

}  // namespace

struct rn_seg_head {
    rn_ctx *ctx;
    uint64_t cin, mid, classes;
    // what the two convolutions run with: mid rounded up to a multiple of 64 (the bf16 contraction's K granule; the
    // added channels have zero weights, scale 0 and shift 0, so they hold ReLU(0) = 0 and meet zero columns of the
    // 1x1 panel: exact zeros added to every sum) and classes rounded up to a multiple of 4 (16-byte coarse pixels)
    uint64_t midp, cpad;
    int dtype, finalized;
    float *raw[7];     // the state dict's tensors on the device, fp32, padded to midp / cpad
    int is_set[7];
    void *packed1, *packed2;
    float *scale, *shift;
    void *mid_t;       // [cap, h, w, mid] of the storage type
    float *coarse;     // [cap, h, w, cpad] fp32
    uint64_t cap_pix;  // pixels (images x h x w) the two scratch tensors hold
};

namespace {

const char *const kSegKeys[7] = {"classifier.0.weight",       "classifier.1.weight",      "classifier.1.bias",
                                 "classifier.1.running_mean", "classifier.1.running_var", "classifier.4.weight",
                                 "classifier.4.bias"};

uint64_t seg_key_numel(const rn_seg_head *hd, int i)
{
    if (i == 0) return hd->mid * hd->cin * 9;
    if (i <= 4) return hd->mid;
    return i == 5 ? hd->classes * hd->mid : hd->classes;
}

uint64_t seg_elem(const rn_seg_head *hd) { return hd->dtype == RN_DTYPE_BF16 ? 2 : 4; }

}  // namespace

extern "C" {

int rn_upsample_bilinear_forward(rn_ctx *ctx, const float *src_nhwc, uint64_t B, uint64_t h, uint64_t w,
                                 uint64_t classes, uint64_t src_channels, uint64_t H, uint64_t W, float *scores_nchw,
                                 uint8_t *labels)
{
    RN_ENTER(ctx);
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, src_nhwc, "src_nhwc is NULL");
    RN_REQUIRE(ctx, scores_nchw || labels, "both outputs (scores_nchw, labels) are NULL");
    RN_REQUIRE(ctx, classes >= 1 && classes <= 256, "classes must be 1..256");
    RN_REQUIRE(ctx, src_channels >= classes && src_channels <= 256 && src_channels % 4 == 0,
               "src_channels must be a multiple of 4, >= classes and <= 256");
    RN_REQUIRE(ctx, h >= 1 && w >= 1 && H >= 1 && W >= 1, "h, w, H, W must be >= 1");
    RN_REQUIRE(ctx, h < (1ull << 31) && w < (1ull << 31) && h * w < (1ull << 31) && H < (1ull << 31) &&
                        W < (1ull << 31) && H * W < (1ull << 31),
               "h * w and H * W must be below 2^31");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(src_nhwc) & 15) == 0, "src_nhwc must be 16-byte aligned");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(scores_nchw) & 3) == 0, "scores_nchw must be 4-byte aligned");
    seg_args p;
    p.h = (uint32_t)h, p.w = (uint32_t)w, p.classes = (uint32_t)classes, p.cs = (uint32_t)src_channels;
    p.H = (uint32_t)H, p.W = (uint32_t)W;
    p.scale_h = (float)h / (float)H, p.scale_w = (float)w / (float)W;
    const uint64_t tx = rn_ceil_div(W, kSegTX), ty = rn_ceil_div(H, kSegTY);
    p.tiles_x = (uint32_t)tx;
    const uint64_t want = seg_span(p.scale_h, kSegTY, h) * seg_span(p.scale_w, kSegTX, w) * (classes | 1) * sizeof(float);
    const uint32_t lds = want <= kSegLdsCap ? (uint32_t)want : 0;  // 0: every tile reads global memory
    p.lds_floats = lds / 4;
    // gridDim.y is limited to 65535: walk the batch in slabs
    for (uint64_t b0 = 0; b0 < B; b0 += 65535) {
        const uint64_t nb = (B - b0) < 65535 ? (B - b0) : 65535;
        const dim3 grid((unsigned)(tx * ty), (unsigned)nb);
        p.src = src_nhwc + b0 * h * w * src_channels;
        p.scores = scores_nchw ? scores_nchw + b0 * classes * H * W : NULL;
        p.labels = labels ? labels + b0 * H * W : NULL;
        if (scores_nchw && labels)
            upsample_bilinear_kernel<true, true><<<grid, 256, lds, ctx->stream>>>(p);
        else if (scores_nchw)
            upsample_bilinear_kernel<true, false><<<grid, 256, lds, ctx->stream>>>(p);
        else
            upsample_bilinear_kernel<false, true><<<grid, 256, lds, ctx->stream>>>(p);
    }
    return rn_after_launch(ctx, "rn_upsample_bilinear_forward");
}

// ---- the head ---------------------------------------------------------------------------------------------

int rn_seg_head_create(rn_ctx *ctx, rn_seg_head **out, uint64_t in_channels, uint64_t mid_channels, uint64_t classes)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    RN_REQUIRE(ctx, in_channels >= 64 && in_channels % 64 == 0 && in_channels <= 8192,
               "in_channels must be a multiple of 64 (at most 8192)");
    RN_REQUIRE(ctx, mid_channels >= 1 && mid_channels <= 8192, "mid_channels must be 1..8192");
    RN_REQUIRE(ctx, classes >= 1 && classes <= 256, "classes must be 1..256");
    rn_seg_head *hd = (rn_seg_head *)calloc(1, sizeof(*hd));
    if (!hd) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_seg_head_create: out of host memory");
    hd->ctx = ctx;
    hd->cin = in_channels, hd->mid = mid_channels, hd->classes = classes;
    hd->midp = (mid_channels + 63) / 64 * 64, hd->cpad = (classes + 3) / 4 * 4;
    hd->dtype = RN_DTYPE_F32;
    *out = hd;
    return RN_OK;
}

int rn_seg_head_set_dtype(rn_seg_head *hd, int dtype)
{
    if (!hd) return RN_ERR_INVALID;
    RN_REQUIRE(hd->ctx, !hd->finalized, "the head is finalized");
    RN_REQUIRE(hd->ctx, dtype == RN_DTYPE_F32 || dtype == RN_DTYPE_BF16, "unknown dtype");
    hd->dtype = dtype;
    return RN_OK;
}

int rn_seg_head_set_tensor(rn_seg_head *hd, const char *key, const float *host_data, uint64_t numel)
{
    if (!hd) return RN_ERR_INVALID;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, key && host_data, "key or host_data is NULL");
    RN_REQUIRE(ctx, !hd->finalized, "the head is finalized");
    int i = 0;
    while (i < 7 && strcmp(key, kSegKeys[i]) != 0) ++i;
    if (i == 7) return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head_set_tensor: unknown key '%s'", key);
    if (numel != seg_key_numel(hd, i))
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head_set_tensor: %s has %llu elements, not %llu", key,
                            (unsigned long long)seg_key_numel(hd, i), (unsigned long long)numel);
    // padded on the host: rows of `len` values become rows of `pitch`, `rows` rows become `prows`; everything added
    // is zero but the running variance of an added mid channel (1: scale = 0 / sqrt(1 + eps) = 0, shift = 0)
    const uint64_t rows = i == 0 ? hd->mid : i <= 4 ? 1 : hd->classes, prows = i == 0 ? hd->midp : i <= 4 ? 1 : hd->cpad;
    const uint64_t len = i == 0 ? hd->cin * 9 : i <= 5 ? hd->mid : 1, pitch = i == 0 ? len : i <= 5 ? hd->midp : 1;
    float *padded = (float *)calloc(prows * pitch, sizeof(float));
    if (!padded) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_seg_head_set_tensor: out of host memory");
    for (uint64_t r = 0; r < rows; ++r) memcpy(padded + r * pitch, host_data + r * len, len * sizeof(float));
    if (i == 4)
        for (uint64_t c = hd->mid; c < hd->midp; ++c) padded[c] = 1.0f;
    int st = hd->raw[i] ? RN_OK : rn_malloc(ctx, (void **)&hd->raw[i], prows * pitch * sizeof(float));
    if (st == RN_OK) st = rn_ctx_upload_sync(ctx, hd->raw[i], padded, prows * pitch * sizeof(float));
    free(padded);
    RN_TRY(st);
    hd->is_set[i] = 1;
    return RN_OK;
}

int rn_seg_head_finalize(rn_seg_head *hd)
{
    if (!hd) return RN_ERR_INVALID;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    if (hd->finalized) return RN_OK;
    for (int i = 0; i < 7; ++i)
        if (!hd->is_set[i]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head_finalize: %s is not set", kSegKeys[i]);
    const uint64_t es = seg_elem(hd);
    RN_TRY(rn_malloc(ctx, (void **)&hd->scale, hd->midp * sizeof(float)));
    RN_TRY(rn_malloc(ctx, (void **)&hd->shift, hd->midp * sizeof(float)));
    RN_TRY(rn_malloc(ctx, &hd->packed1, rn_conv2d_packed_weight_numel_dt(hd->dtype, hd->cin, hd->midp, 3) * es));
    RN_TRY(rn_malloc(ctx, &hd->packed2, rn_conv2d_packed_weight_numel_dt(hd->dtype, hd->midp, hd->cpad, 1) * es));
    RN_TRY(rn_batchnorm2d_fold(ctx, hd->raw[1], hd->raw[2], hd->raw[3], hd->raw[4], hd->scale, hd->shift, hd->midp));
    RN_TRY(rn_conv2d_pack_weight_dt(ctx, hd->dtype, hd->raw[0], hd->packed1, hd->cin, hd->midp, 3));
    RN_TRY(rn_conv2d_pack_weight_dt(ctx, hd->dtype, hd->raw[5], hd->packed2, hd->midp, hd->cpad, 1));
    RN_TRY(rn_sync(ctx));
    for (int i = 0; i < 6; ++i) {  // the bias (raw[6]) stays: it is the 1x1 convolution's shift
        RN_TRY(rn_free(ctx, hd->raw[i]));
        hd->raw[i] = NULL;
    }
    hd->finalized = 1;
    return RN_OK;
}

int rn_seg_head_destroy(rn_seg_head *hd)
{
    if (!hd) return RN_OK;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    RN_TRY(rn_sync(ctx));
    void *bufs[6] = {hd->packed1, hd->packed2, hd->scale, hd->shift, hd->mid_t, hd->coarse};
    for (int i = 0; i < 7; ++i)
        if (hd->raw[i]) rn_free(ctx, hd->raw[i]);
    for (int i = 0; i < 6; ++i)
        if (bufs[i]) rn_free(ctx, bufs[i]);
    free(hd);
    return RN_OK;
}

// library-internal (rn_private.h): what the model driver asks of a head and queues of it
int rn_seg_head_matches(const rn_seg_head *hd, uint64_t in_channels, int dtype, const char **why)
{
    const char *w = NULL;
    if (!hd) w = "the head is NULL";
    else if (!hd->finalized) w = "the head is not finalized";
    else if (hd->cin != in_channels) w = "the head's in_channels is not the width of the model's layer4";
    else if (hd->dtype != dtype) w = "the head's storage type (dtype) is not the model's";
    if (why) *why = w;
    return w == NULL;
}

void rn_seg_head_dims(const rn_seg_head *hd, uint64_t dims[4])
{
    dims[0] = hd->cin, dims[1] = hd->midp, dims[2] = hd->classes, dims[3] = hd->cpad;
}

// the two scratch tensors for `pixels` coarse pixels (images x h x w); they grow like the model's logits buffer:
// never on a stream that is being captured, never while a captured graph of the context may hold them
int rn_seg_head_reserve(rn_seg_head *hd, uint64_t pixels)
{
    rn_ctx *ctx = hd->ctx;
    if (pixels <= hd->cap_pix) return RN_OK;
    if (rn_ctx_is_capturing(ctx))
        return rn_set_error(ctx, RN_ERR_UNSUPPORTED, "rn_seg_head: the scratch cannot grow on a stream that is being captured");
    if (hd->cap_pix > 0 && ctx->graphs_live > 0)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head: the scratch cannot grow while a captured graph lives");
    RN_TRY(rn_sync(ctx));
    if (hd->mid_t) RN_TRY(rn_free(ctx, hd->mid_t));
    hd->mid_t = NULL;
    if (hd->coarse) RN_TRY(rn_free(ctx, hd->coarse));
    hd->coarse = NULL;
    hd->cap_pix = 0;
    RN_TRY(rn_malloc(ctx, &hd->mid_t, pixels * hd->midp * seg_elem(hd)));
    RN_TRY(rn_malloc(ctx, (void **)&hd->coarse, pixels * hd->cpad * sizeof(float)));
    hd->cap_pix = pixels;
    return RN_OK;
}

// one of the head's three launches on `ctx` (the head's own context, or the context of the model's stream the
// images run on): B images whose scratch starts `pix0` coarse pixels into the head's two tensors
int rn_seg_head_step(rn_seg_head *hd, rn_ctx *ctx, int step, const void *x_nhwc, uint64_t pix0, uint64_t B, uint64_t h,
                     uint64_t w, uint64_t H, uint64_t W, float *scores_nchw, uint8_t *labels)
{
    void *mid = (char *)hd->mid_t + pix0 * hd->midp * seg_elem(hd);
    float *coarse = hd->coarse + pix0 * hd->cpad;
    rn_epilogue ep;
    ep.residual = NULL;
    if (pix0 + B * h * w > hd->cap_pix) return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head: scratch not reserved");
    if (step == 0) {
        ep.scale = hd->scale, ep.shift = hd->shift, ep.relu = 1;
        return rn_conv2d_nhwc_forward_dt(ctx, hd->dtype, hd->dtype, x_nhwc, mid, hd->packed1, 3, 1, 1, h, w, B, hd->cin,
                                         hd->midp, h, w, &ep);
    }
    if (step == 1) {
        ep.scale = NULL, ep.shift = hd->raw[6], ep.relu = 0;
        return rn_conv2d_nhwc_forward_dt(ctx, hd->dtype, RN_DTYPE_F32, mid, coarse, hd->packed2, 1, 1, 0, h, w, B,
                                         hd->midp, hd->cpad, h, w, &ep);
    }
    return rn_upsample_bilinear_forward(ctx, coarse, B, h, w, hd->classes, hd->cpad, H, W, scores_nchw, labels);
}

int rn_seg_head_forward(rn_seg_head *hd, const void *x_nhwc, uint64_t B, uint64_t h, uint64_t w, uint64_t H, uint64_t W,
                        float *scores_nchw, uint8_t *labels)
{
    if (!hd) return RN_ERR_INVALID;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, hd->finalized, "the head is not finalized");
    RN_REQUIRE(ctx, x_nhwc, "x_nhwc is NULL");
    RN_REQUIRE(ctx, scores_nchw || labels, "both outputs (scores_nchw, labels) are NULL");
    RN_REQUIRE(ctx, h >= 1 && w >= 1 && H >= 1 && W >= 1, "h, w, H, W must be >= 1");
    RN_REQUIRE(ctx, h < (1ull << 31) && w < (1ull << 31) && B * h * w < (1ull << 31), "B * h * w must be below 2^31");
    if (B == 0) return RN_OK;
    const int saved_layout = ctx->layout;
    RN_TRY(rn_seg_head_reserve(hd, B * h * w));
    ctx->layout = RN_LAYOUT_NHWC;
    int st = RN_OK;
    for (int step = 0; step < 3 && st == RN_OK; ++step)
        st = rn_seg_head_step(hd, ctx, step, x_nhwc, 0, B, h, w, H, W, scores_nchw, labels);
    ctx->layout = saved_layout;
    return st;
}

}  // extern "C"
