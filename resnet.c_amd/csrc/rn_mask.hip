// The mask branch of a two-stage detector behind the box head: torchvision's MaskRCNNHeads and MaskRCNNPredictor,
// maskrcnn_inference and paste_masks_in_image.  The five convolutions are the library's contractions (the transposed
// one as ONE 1x1 panel of 4 * Cr channels: kernel 2 at stride 2 overlaps nothing); three kernels are this file's:
//   detection_rois_kernel: the detections' boxes and labels as the pooler's RoI rows, padding rows as rows the pooler
//     answers with zeros;
//   mask_predict_kernel: the label's row of mask_fcn_logits on the deconvolution's output and the sigmoid, 1 / (C - 1)
//     of the predictor's products; no [K, C, 2M, 2M] tensor exists;
//   paste_masks_kernel: one detection's probability map resized into its box in the image, as fp32 and / or as bytes
//     of (mask > threshold), every byte of the outputs written once.
// No atomics anywhere.  The reference classifies whole images only; nothing here has a counterpart in it.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "rn_conv_params.h"
#include "rn_internal.h"
#include "rn_private.h"

// The arithmetic of the paste and the summation order of the predictor are contracts (rn_hip.h): no product of this
// file is fused into an add.
#pragma clang fp contract(off)

namespace {

constexpr uint32_t kMaskBlock = 256;
constexpr uint32_t kMaskMaxC = 1024;   // classes, background included
constexpr uint32_t kMaskMaxCr = 1024;  // dim_reduced: the label's weight row in LDS
constexpr uint32_t kMaskMaxM = 32;     // the head's resolution
constexpr uint32_t kMaskMaxMo = 64;    // the side of a probability map the paste reads

// ---- detections -> RoI rows -------------------------------------------------------------------------------------
// A thread writes one aligned quad of the flat [n * 5] output (the run's head and tail: scalars), whatever the address.
struct drois_args {
    const float *boxes;     // [n, 4]
    const int32_t *labels;  // [n]
    float *rois;            // [n, 5]
    uint32_t n, D, img0, mul_d, shr_d;
};

__global__ __launch_bounds__(kMaskBlock) void detection_rois_kernel(const drois_args p)
{
    const uint32_t total = p.n * 5;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p.rois) >> 2) & 3;  // floats behind the aligned quad
    const uint32_t quads = (total + sh + 3) >> 2;
    for (uint32_t q = blockIdx.x * kMaskBlock + threadIdx.x; q < quads; q += gridDim.x * kMaskBlock) {
        const uint32_t t0 = 4 * q - sh;  // wraps below 0: those elements are outside the run
        float v[4];
        bool in[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t t = t0 + e;
            in[e] = t < total;
            v[e] = 0.0f;
            if (in[e]) {
                const uint32_t r = t / 5, j = t - r * 5;
                const bool real = p.labels[r] >= 1;
                if (j == 0) v[e] = real ? (float)(p.img0 + rn_gemm::fast_div(r, (int)p.D, p.mul_d, p.shr_d)) : -1.0f;
                else v[e] = real ? p.boxes[(uint64_t)r * 4 + (j - 1)] : 0.0f;
            }
        }
        if (in[0] && in[3]) {  // p.rois + t0 is 16-byte aligned by construction
            *reinterpret_cast<float4 *>(p.rois + t0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (in[e]) p.rois[(uint32_t)(t0 + e)] = v[e];
        }
    }
}

// ---- the class-selected predictor -------------------------------------------------------------------------------
// One block: one detection and kPredPix pixels of its M x M map; the label's weight row sits in LDS.  A wave takes a
// pixel at a time: the pixel's 4 * Cr floats are one run, quarter g = dy * 2 + dx of it on lanes 16 g .. 16 g + 15, each
// lane loading 16-byte chunks li, li + 16, ... of its quarter (a quarter-wave reads 256 consecutive bytes per trip).
// The sum of an output: every lane adds its products to 0 in ascending channel order, then the sixteen partial sums
// fold by the butterfly 8, 4, 2, 1.  That order depends on Cr alone.
constexpr uint32_t kPredPix = 16;

struct predict_args {
    const float4 *t;        // [K, M * M, 4 * Cr]
    const int32_t *labels;  // [K]
    const float *weight;    // [C, Cr]
    const float *bias;      // [C]
    float *probs;           // [K, 2M, 2M]
    uint32_t K, M, MM, Cr, C, mul_m, shr_m;
};

__global__ __launch_bounds__(kMaskBlock) void mask_predict_kernel(const predict_args p)
{
    __shared__ float4 wrow[kMaskMaxCr / 4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const uint32_t cr4 = p.Cr >> 2;
    for (uint32_t k = blockIdx.y; k < p.K; k += gridDim.y) {
        const int32_t l = p.labels[k];
        const bool valid = l >= 1 && l < (int32_t)p.C;  // uniform in the block
        int32_t lc = l < 0 ? 0 : l;                      // unconditional: no label indexes outside the weights
        lc = lc > (int32_t)p.C - 1 ? (int32_t)p.C - 1 : lc;
        const float4 *wsrc = reinterpret_cast<const float4 *>(p.weight + (uint64_t)lc * p.Cr);
        for (uint32_t i = tid; i < cr4; i += kMaskBlock) wrow[i] = wsrc[i];
        const float bias = p.bias[lc];
        __syncthreads();
        const uint32_t pix0 = blockIdx.x * kPredPix;
        for (uint32_t pp = wave; pp < kPredPix; pp += kMaskBlock / 64) {
            const uint32_t pix = pix0 + pp;
            if (pix >= p.MM) break;  // uniform in the wave
            float prob = 0.0f;
            if (valid) {
                const float4 *src = p.t + ((uint64_t)k * p.MM + pix) * p.Cr + g * cr4;
                float acc = 0.0f;
                for (uint32_t j = li; j < cr4; j += 16) {
                    const float4 a = src[j], w = wrow[j];
                    acc = acc + w.x * a.x;
                    acc = acc + w.y * a.y;
                    acc = acc + w.z * a.z;
                    acc = acc + w.w * a.w;
                }
                acc = acc + __shfl_xor(acc, 8, 64);
                acc = acc + __shfl_xor(acc, 4, 64);
                acc = acc + __shfl_xor(acc, 2, 64);
                acc = acc + __shfl_xor(acc, 1, 64);
                const float z = bias + acc;
                prob = 1.0f / (1.0f + expf(-z));
            }
            if (li == 0) {
                const uint32_t y = rn_gemm::fast_div(pix, (int)p.M, p.mul_m, p.shr_m), x = pix - y * p.M;
                p.probs[(uint64_t)k * 4 * p.MM + (uint64_t)(2 * y + (g >> 1)) * (2 * p.M) + 2 * x + (g & 1)] = prob;
            }
        }
        __syncthreads();  // the next detection of the block reuses the weight row
    }
}

// ---- the paste --------------------------------------------------------------------------------------------------
// One block: one detection and kPasteSpan consecutive elements of its H * W plane, four to a thread per trip (the run
// is fixed: thread t of trip i holds elements 1024 i + 4 t ..).  A block none of whose rows meets the box stores zeros
// and reads nothing; any other stages the detection's zero-padded map in LDS first.  Stores follow
// rn_upsample_bilinear_forward's rule: an aligned unit that starts s elements into a thread's run takes its last s
// values from the next lane; scalars remain where a wave has no next lane and at the plane's ends.
constexpr uint32_t kPasteTrips = 8, kPasteSpan = kPasteTrips * kMaskBlock * 4;

struct paste_args {
    const float *probs;     // [K, Mo, Mo]
    const float *boxes;     // [K, 4]
    const int32_t *labels;  // [K] or NULL
    float *masks;           // [K, H, W] or NULL
    uint8_t *bits;          // [K, H, W] or NULL
    uint32_t K, Mo, H, W, HW, mul_w, shr_w, mul_p, shr_p;
    float s, threshold;
};

// rn_upsample_bilinear_forward's per-axis rule: the index pair (always inside [0, n_in)) and the second's weight
__device__ __forceinline__ void paste_coord(uint32_t o, float scale, uint32_t n_in, uint32_t *i0, uint32_t *i1, float *l1)
{
    const float c = (float)o + 0.5f;
    float s = scale * c - 0.5f;
    s = s > 0.0f ? s : 0.0f;
    uint32_t a = (uint32_t)(int)s;
    if (a > n_in - 1) a = n_in - 1;  // unconditional: no box content indexes outside the padded map
    *i0 = a;
    *i1 = a + 1 < n_in ? a + 1 : n_in - 1;
    *l1 = s - (float)a;
}

__device__ __forceinline__ float paste_clamp(float v)
{
    v = v < -1073741824.0f ? -1073741824.0f : v;
    return v > 1073741824.0f ? 1073741824.0f : v;
}

template <bool MASKS, bool BITS>
__global__ __launch_bounds__(kMaskBlock) void paste_masks_kernel(const paste_args p)
{
    extern __shared__ float pad[];  // (Mo + 2)^2
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t side = p.Mo + 2;
    const uint32_t e0 = blockIdx.x * kPasteSpan;
    const uint32_t e1 = p.HW - e0 < kPasteSpan ? p.HW : e0 + kPasteSpan;
    const uint32_t yb0 = rn_gemm::fast_div(e0, (int)p.W, p.mul_w, p.shr_w);
    const uint32_t yb1 = rn_gemm::fast_div(e1 - 1, (int)p.W, p.mul_w, p.shr_w);
    for (uint32_t k = blockIdx.y; k < p.K; k += gridDim.y) {
        const float *bx = p.boxes + (uint64_t)k * 4;
        const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
        const float wh = ((x2 - x1) * 0.5f) * p.s, hh = ((y2 - y1) * 0.5f) * p.s;
        const float xc = (x2 + x1) * 0.5f, yc = (y2 + y1) * 0.5f;
        const float fx0 = xc - wh, fy0 = yc - hh, fx1 = xc + wh, fy1 = yc + hh;
        bool live = !p.labels || p.labels[k] >= 1;
        live = live && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
        live = live && isfinite(fx0) && isfinite(fy0) && isfinite(fx1) && isfinite(fy1);  // (an overflow of the expansion)
        const int bx0 = live ? (int)paste_clamp(fx0) : 0, by0 = live ? (int)paste_clamp(fy0) : 0;
        const int bx1 = live ? (int)paste_clamp(fx1) : 0, by1 = live ? (int)paste_clamp(fy1) : 0;
        long long bw = (long long)bx1 - bx0 + 1, bh = (long long)by1 - by0 + 1;
        bw = bw < 1 ? 1 : bw, bh = bh < 1 ? 1 : bh;
        const float scale_w = (float)side / (float)bw, scale_h = (float)side / (float)bh;
        // the pasted pixels: xs <= x < xe, ys <= y < ye (none where the row is dead)
        const long long xe64 = (long long)bx1 + 1 < (long long)p.W ? (long long)bx1 + 1 : (long long)p.W;
        const long long ye64 = (long long)by1 + 1 < (long long)p.H ? (long long)by1 + 1 : (long long)p.H;
        const int xs = bx0 > 0 ? bx0 : 0, ys = by0 > 0 ? by0 : 0;
        const int xe = live ? (int)xe64 : 0, ye = live ? (int)ye64 : 0;
        const bool hits = xs < xe && ys < ye && (int)yb0 < ye && (int)yb1 >= ys;  // uniform in the block
        if (hits) {
            const float *src = p.probs + (uint64_t)k * p.Mo * p.Mo;
            for (uint32_t i = tid; i < side * side; i += kMaskBlock) {
                const uint32_t r = rn_gemm::fast_div(i, (int)side, p.mul_p, p.shr_p), c = i - r * side;
                const bool inner = r >= 1 && r <= p.Mo && c >= 1 && c <= p.Mo;
                pad[i] = inner ? src[(r - 1) * p.Mo + (c - 1)] : 0.0f;
            }
            __syncthreads();
        }
        float *mplane = MASKS ? p.masks + (uint64_t)k * p.HW : nullptr;
        uint8_t *bplane = BITS ? p.bits + (uint64_t)k * p.HW : nullptr;
        for (uint32_t base = e0; base < e1; base += kMaskBlock * 4) {  // uniform trips: the shuffles want every lane
            const uint32_t p0 = base + tid * 4;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (hits && p0 < e1) {
                uint32_t yy = rn_gemm::fast_div(p0, (int)p.W, p.mul_w, p.shr_w), xx = p0 - yy * p.W;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if ((int)yy >= ys && (int)yy < ye && (int)xx >= xs && (int)xx < xe) {
                        uint32_t r0, r1, c0, c1;
                        float a1, b1;
                        paste_coord((uint32_t)((int)yy - by0), scale_h, side, &r0, &r1, &a1);
                        paste_coord((uint32_t)((int)xx - bx0), scale_w, side, &c0, &c1, &b1);
                        const float a0 = 1.0f - a1, b0 = 1.0f - b1;
                        const float top = b0 * pad[r0 * side + c0] + b1 * pad[r0 * side + c1];
                        const float bot = b0 * pad[r1 * side + c0] + b1 * pad[r1 * side + c1];
                        v[e] = a0 * top + a1 * bot;
                    }
                    if (++xx == p.W) xx = 0, ++yy;
                }
            }
            const bool nb_ok = lane < 63;  // lane + 1 holds the next run
            if (MASKS) {
                const uint32_t s = (0u - (uint32_t)(reinterpret_cast<uintptr_t>(mplane + p0) >> 2)) & 3;  // floats to the aligned quad
                const float n0 = __shfl_down(v[0], 1), n1 = __shfl_down(v[1], 1), n2 = __shfl_down(v[2], 1);
                if (s == 0) {
                    if (p0 + 3 < e1) {
                        *reinterpret_cast<float4 *>(mplane + p0) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (p0 + e < e1) mplane[p0 + e] = v[e];
                    }
                } else {
                    const bool prev_full = lane > 0 && p0 + s - 1 < e1;  // the previous lane's quad ends at p0 + s - 1
                    const bool full = nb_ok && p0 + s + 3 < e1;
#pragma unroll
                    for (int e = 0; e < 3; ++e)
                        if (!prev_full && (uint32_t)e < s && p0 + e < e1) mplane[p0 + e] = v[e];
                    if (full) {
                        float4 t;
                        if (s == 1) t = make_float4(v[1], v[2], v[3], n0);
                        else if (s == 2) t = make_float4(v[2], v[3], n0, n1);
                        else t = make_float4(v[3], n0, n1, n2);
                        *reinterpret_cast<float4 *>(mplane + p0 + s) = t;
                    } else {
#pragma unroll
                        for (int e = 1; e < 4; ++e)
                            if ((uint32_t)e >= s && p0 + e < e1) mplane[p0 + e] = v[e];
                    }
                }
            }
            if (BITS) {
                uint32_t bit[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) bit[e] = v[e] > p.threshold ? 1u : 0u;
                const uint32_t s = (0u - (uint32_t)reinterpret_cast<uintptr_t>(bplane + p0)) & 3;  // bytes to the aligned word
                const uint32_t mine = bit[0] | bit[1] << 8 | bit[2] << 16 | bit[3] << 24;
                const uint32_t next = __shfl_down(mine, 1);
                const bool prev_full = s > 0 && lane > 0 && p0 + s - 1 < e1;
                const bool full = (s == 0 || nb_ok) && p0 + s + 3 < e1;
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (!prev_full && (uint32_t)e < s && p0 + e < e1) bplane[p0 + e] = (uint8_t)bit[e];
                if (full) {
                    const uint64_t both = (uint64_t)next << 32 | mine;
                    *reinterpret_cast<uint32_t *>(bplane + p0 + s) = (uint32_t)(both >> (8 * s));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((uint32_t)e >= s && p0 + e < e1) bplane[p0 + e] = (uint8_t)bit[e];
                }
            }
        }
        __syncthreads();  // the next detection of the block reuses the padded map
    }
}

// ---- host side --------------------------------------------------------------------------------------------------
int rois_launch(rn_ctx *ctx, const float *boxes, const int32_t *labels, uint64_t img0, uint64_t B, uint64_t D, float *rois,
                const char *what)
{
    drois_args a;
    memset(&a, 0, sizeof(a));
    a.boxes = boxes, a.labels = labels, a.rois = rois;
    a.n = (uint32_t)(B * D), a.D = (uint32_t)D, a.img0 = (uint32_t)img0;
    rn_fast_div((unsigned)D, &a.mul_d, &a.shr_d);
    detection_rois_kernel<<<rn_stream_grid((B * D * 5 + 6) / 4 + 1, kMaskBlock), kMaskBlock, 0, ctx->stream>>>(a);
    return rn_after_launch(ctx, what);
}

int predict_launch(rn_ctx *ctx, const float *t, const int32_t *labels, const float *weight, const float *bias, uint64_t K,
                   uint64_t M, uint64_t Cr, uint64_t C, float *probs, const char *what)
{
    predict_args a;
    memset(&a, 0, sizeof(a));
    a.t = (const float4 *)t, a.labels = labels, a.weight = weight, a.bias = bias, a.probs = probs;
    a.K = (uint32_t)K, a.M = (uint32_t)M, a.MM = (uint32_t)(M * M), a.Cr = (uint32_t)Cr, a.C = (uint32_t)C;
    rn_fast_div((unsigned)M, &a.mul_m, &a.shr_m);
    const dim3 grid((unsigned)rn_ceil_div(M * M, kPredPix), (unsigned)(K < 65535 ? K : 65535));
    mask_predict_kernel<<<grid, kMaskBlock, 0, ctx->stream>>>(a);
    return rn_after_launch(ctx, what);
}

int paste_launch(rn_ctx *ctx, const float *probs, const float *boxes, const int32_t *labels, uint64_t K, uint64_t Mo,
                 uint64_t H, uint64_t W, float threshold, float *masks, uint8_t *bits, const char *what)
{
    paste_args a;
    memset(&a, 0, sizeof(a));
    a.probs = probs, a.boxes = boxes, a.labels = labels, a.masks = masks, a.bits = bits;
    a.K = (uint32_t)K, a.Mo = (uint32_t)Mo, a.H = (uint32_t)H, a.W = (uint32_t)W, a.HW = (uint32_t)(H * W);
    rn_fast_div((unsigned)W, &a.mul_w, &a.shr_w);
    rn_fast_div((unsigned)(Mo + 2), &a.mul_p, &a.shr_p);
    a.s = (float)((double)(Mo + 2) / (double)Mo), a.threshold = threshold;
    const size_t lds = (size_t)(Mo + 2) * (Mo + 2) * sizeof(float);
    const dim3 grid((unsigned)rn_ceil_div(H * W, kPasteSpan), (unsigned)(K < 65535 ? K : 65535));
    if (masks && bits) paste_masks_kernel<true, true><<<grid, kMaskBlock, lds, ctx->stream>>>(a);
    else if (masks) paste_masks_kernel<true, false><<<grid, kMaskBlock, lds, ctx->stream>>>(a);
    else paste_masks_kernel<false, true><<<grid, kMaskBlock, lds, ctx->stream>>>(a);
    return rn_after_launch(ctx, what);
}

// every refusal of the paste's shapes; fn: the entry point's name
int paste_check(rn_ctx *ctx, const char *fn, uint64_t K, uint64_t Mo, uint64_t H, uint64_t W, float threshold)
{
    const char *why = NULL;
    if (Mo < 1 || Mo > kMaskMaxMo) why = "Mo must be 1..64";
    else if (H < 1 || W < 1 || H >= (1ull << 24) || W >= (1ull << 24) || H * W >= (1ull << 31) - kPasteSpan)
        why = "H and W must be 1 .. 2^24 - 1 and H * W below 2^31 - 8192";
    else if (K >= (1ull << 31)) why = "K must be below 2^31";
    else if (threshold != threshold) why = "threshold is a NaN";
    if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
    return RN_OK;
}

}  // namespace

extern "C" {

int rn_detection_rois_window(rn_ctx *ctx, const float *boxes, const int32_t *labels, uint64_t img0, uint64_t B, uint64_t D,
                             float *rois)
{
    return rois_launch(ctx, boxes, labels, img0, B, D, rois, "rn_detection_rois_forward");
}

int rn_detection_rois_forward(rn_ctx *ctx, const float *boxes, const int32_t *labels, uint64_t B, uint64_t D, float *rois)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, B < (1ull << 24) && D < (1ull << 24) && B * D * 5 < (1ull << 31) - 8, "B * D * 5 must be below 2^31 (B below 2^24)");
    if (B == 0 || D == 0) return RN_OK;
    RN_REQUIRE(ctx, boxes, "boxes is NULL");
    RN_REQUIRE(ctx, labels, "labels is NULL");
    RN_REQUIRE(ctx, rois, "rois is NULL");
    const operand ops[3] = {{rois, B * D * 20, "rois", true, false},
                            {boxes, B * D * 16, "boxes", false, false},
                            {labels, B * D * 4, "labels", false, false}};
    RN_TRY(check_operands(ctx, __func__, ops, 3));
    return rois_launch(ctx, boxes, labels, 0, B, D, rois, __func__);
}

int rn_mask_predict_forward(rn_ctx *ctx, const float *t, const int32_t *labels, const float *weight, const float *bias,
                            uint64_t K, uint64_t M, uint64_t Cr, uint64_t C, float *probs)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, Cr >= 64 && Cr <= kMaskMaxCr && Cr % 64 == 0, "Cr must be a multiple of 64 up to 1024");
    RN_REQUIRE(ctx, M >= 1 && M <= kMaskMaxM, "M must be 1..32");
    RN_REQUIRE(ctx, C >= 2 && C <= kMaskMaxC, "C must be 2..1024");
    RN_REQUIRE(ctx, K < (1ull << 31), "K must be below 2^31");
    if (K == 0) return RN_OK;
    RN_REQUIRE(ctx, t, "t is NULL");
    RN_REQUIRE(ctx, labels, "labels is NULL");
    RN_REQUIRE(ctx, weight && bias, "weight or bias is NULL");
    RN_REQUIRE(ctx, probs, "probs is NULL");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(t) & 15) == 0, "t is off a 16-byte boundary");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(weight) & 15) == 0, "weight is off a 16-byte boundary");
    const operand ops[5] = {{probs, K * 4 * M * M * 4, "probs", true, false},
                            {t, K * M * M * 4 * Cr * 4, "t", false, false},
                            {labels, K * 4, "labels", false, false},
                            {weight, C * Cr * 4, "weight", false, false},
                            {bias, C * 4, "bias", false, false}};
    RN_TRY(check_operands(ctx, __func__, ops, 5));
    return predict_launch(ctx, t, labels, weight, bias, K, M, Cr, C, probs, __func__);
}

int rn_paste_masks_forward(rn_ctx *ctx, const float *probs, const float *boxes, const int32_t *labels, uint64_t K, uint64_t Mo,
                           uint64_t H, uint64_t W, float threshold, float *masks, uint8_t *bits)
{
    RN_ENTER(ctx);
    RN_TRY(paste_check(ctx, __func__, K, Mo, H, W, threshold));
    RN_REQUIRE(ctx, masks || bits, "masks and bits are both NULL");
    if (K == 0) return RN_OK;
    RN_REQUIRE(ctx, probs, "probs is NULL");
    RN_REQUIRE(ctx, boxes, "boxes is NULL");
    const operand ops[5] = {{masks, K * H * W * 4, "masks", true, false},
                            {bits, K * H * W, "bits", true, true},
                            {probs, K * Mo * Mo * 4, "probs", false, false},
                            {boxes, K * 16, "boxes", false, false},
                            {labels, K * 4, "labels", false, false}};
    RN_TRY(check_operands(ctx, __func__, ops, 5));
    return paste_launch(ctx, probs, boxes, labels, K, Mo, H, W, threshold, masks, bits, __func__);
}

// ---- the object: MaskRCNNHeads (the RoI tower of rn_stage.hip) and MaskRCNNPredictor in front of the predict and paste
// launches ----
struct rn_mask_head {
    rn_roi_tower tower;  // its panel: the transposed convolution as ONE 1x1 Clast -> 4 Cr (its shift: conv5_mask's bias four
                         // times), ReLU; its extra tensor: the probabilities [., 2M, 2M] of a forward that does not export them;
                         // its table behind the layers: conv5_mask: 2n, 2n + 1; mask_fcn_logits: 2n + 2, 2n + 3
    uint64_t Cr, C;
    float *lw, *lb;      // mask_fcn_logits on the device, torchvision's layout
};

// either spelling of a layer ("mask_head.0.0.weight", "mask_head.mask_fcn1.weight")
static void mask_layer_key(int i, const char *leaf, char key[RN_PARAM_KEY], char alt[RN_PARAM_KEY])
{
    snprintf(key, RN_PARAM_KEY, "mask_head.%d.0.%s", i, leaf);
    snprintf(alt, RN_PARAM_KEY, "mask_head.mask_fcn%d.%s", i + 1, leaf);
}

int rn_mask_head_create(rn_ctx *ctx, rn_mask_head **out, uint64_t in_channels, uint64_t n_layers, const uint64_t *layer_channels,
                        uint64_t dim_reduced, uint64_t classes, uint64_t resolution)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    const char *own = NULL;
    if (dim_reduced < 64 || dim_reduced % 64 != 0 || dim_reduced > kMaskMaxCr) own = "dim_reduced must be a multiple of 64 up to 1024";
    else if (classes < 2 || classes > kMaskMaxC) own = "classes must be 2..1024";
    RN_TRY(rn_roi_tower_check(ctx, __func__, in_channels, n_layers, layer_channels, own, resolution, kMaskMaxM));
    rn_mask_head *h = (rn_mask_head *)calloc(1, sizeof(*h));
    if (!h) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_mask_head_create: out of host memory");
    const uint64_t Cr = h->Cr = dim_reduced;
    h->C = classes;
    rn_roi_tower *t = &h->tower;
    t->name = "rn_mask_head", t->what = "the mask head", t->panel = 4 * Cr, t->panel_relu = 1, t->extra_floats = 4;
    rn_roi_tower_init(t, ctx, in_channels, n_layers, layer_channels, resolution, mask_layer_key);
    const uint64_t last = t->ch[n_layers - 1];
    rn_params_add(&t->params, "mask_predictor.conv5_mask.weight", NULL, last, Cr * 4, last, Cr * 4, 0.0f);
    rn_params_add(&t->params, "mask_predictor.conv5_mask.bias", NULL, 1, Cr, 1, Cr, 0.0f);
    rn_params_add(&t->params, "mask_predictor.mask_fcn_logits.weight", NULL, classes, Cr, classes, Cr, 0.0f);
    rn_params_add(&t->params, "mask_predictor.mask_fcn_logits.bias", NULL, 1, classes, 1, classes, 0.0f);
    *out = h;
    return RN_OK;
}

int rn_mask_head_set_tensor(rn_mask_head *h, const char *key, const float *host_data, uint64_t numel)
{
    if (!h) return RN_ERR_INVALID;
    rn_roi_tower *t = &h->tower;
    return rn_stage_set_tensor(t->ctx, __func__, t->what, t->finalized, &t->params, key, host_data, numel);
}

int rn_mask_head_finalize(rn_mask_head *h)
{
    if (!h) return RN_ERR_INVALID;
    rn_roi_tower *t = &h->tower;
    rn_ctx *ctx = t->ctx;
    RN_ENTER(ctx);
    if (t->finalized) return RN_OK;
    RN_TRY(rn_roi_tower_pack_layers(t, __func__));
    const uint64_t n = t->n_layers, Cr = h->Cr, last = t->ch[n - 1];
    const rn_params_entry *p = t->params.p;
    // ConvTranspose2d(last, Cr, 2, 2), weight [last, Cr, 2, 2]: output (2y + dy, 2x + dx) reads input (y, x) alone, so
    // it is the 1x1 convolution whose row (dy * 2 + dx) * Cr + co is W[:, co, dy, dx]; the bias four times
    float *w = (float *)malloc((4 * Cr * last + 4 * Cr) * sizeof(float));
    if (!w) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_mask_head_finalize: out of host memory");
    const float *dw = p[2 * n].host, *db = p[2 * n + 1].host;
    for (uint64_t q = 0; q < 4; ++q)
        for (uint64_t co = 0; co < Cr; ++co) {
            for (uint64_t ci = 0; ci < last; ++ci) w[(q * Cr + co) * last + ci] = dw[(ci * Cr + co) * 4 + q];
            w[4 * Cr * last + q * Cr + co] = db[co];
        }
    int st = rn_roi_tower_pack_panel(t, w, w + 4 * Cr * last);
    free(w);
    if (st == RN_OK && !h->lw) st = rn_malloc(ctx, (void **)&h->lw, h->C * Cr * sizeof(float));
    if (st == RN_OK && !h->lb) st = rn_malloc(ctx, (void **)&h->lb, h->C * sizeof(float));
    if (st == RN_OK) st = rn_ctx_upload_sync(ctx, h->lw, p[2 * n + 2].host, h->C * Cr * sizeof(float));
    if (st == RN_OK) st = rn_ctx_upload_sync(ctx, h->lb, p[2 * n + 3].host, h->C * sizeof(float));
    if (st != RN_OK) return st;
    rn_params_free(&t->params);
    t->finalized = 1;
    return RN_OK;
}

int rn_mask_head_destroy(rn_mask_head *h)
{
    if (!h) return RN_OK;
    rn_ctx *ctx = h->tower.ctx;
    RN_ENTER(ctx);
    RN_TRY(rn_sync(ctx));
    rn_roi_tower_free(&h->tower);
    rn_free_null(ctx, (void **)&h->lw), rn_free_null(ctx, (void **)&h->lb);
    free(h);
    return RN_OK;
}

// ---- what differs from another RoI head (rn_private.h: rn_roi_head) ----

// every refusal that concerns the request and the shapes alone, for `rows` detections; boxes_given: a paste is possible
static int mask_head_check(const rn_roi_head *s, rn_ctx *ctx, const char *fn, uint64_t rows, int boxes_given, uint64_t image_h,
                           uint64_t image_w)
{
    const rn_mask_request *q = (const rn_mask_request *)s->req;
    const uint64_t M = s->tower->M;
    if (!q) return rn_set_error(ctx, RN_ERR_INVALID, "%s: the mask request is NULL", fn);
    const char *why = NULL;
    if (!q->probs && !q->masks && !q->bits) why = "probs, masks and bits of the mask request are all NULL";
    else if ((q->masks || q->bits) && !boxes_given) why = "boxes is NULL and the mask request wants pasted masks";
    else if (rows >= (1ull << 31) || rows * M * M >= (1ull << 31)) why = "K * M * M must be below 2^31";
    if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
    if (q->masks || q->bits) RN_TRY(paste_check(ctx, fn, rows, 2 * M, image_h, image_w, q->threshold));
    return RN_OK;
}

static int mask_head_operands(const rn_roi_head *s, uint64_t rows, uint64_t image_h, uint64_t image_w, rn_operand ops[RN_ROI_HEAD_OPERANDS])
{
    const rn_mask_request *q = (const rn_mask_request *)s->req;
    const uint64_t M = s->tower->M, plane = (q->masks || q->bits) ? image_h * image_w : 0;
    ops[0] = {q->rois, rows * 20, "mask.rois", true, false};
    ops[1] = {q->pooled, rows * M * M * s->tower->Cin * 4, "mask.pooled", true, false};
    ops[2] = {q->probs, rows * 4 * M * M * 4, "mask.probs", true, false};
    ops[3] = {q->masks, rows * plane * 4, "mask.masks", true, false};
    ops[4] = {q->bits, rows * plane, "mask.bits", true, true};
    return RN_ROI_HEAD_OPERANDS;
}

// the predict launch, and the paste where masks or bits is given
static int mask_head_behind(const rn_roi_head *s, rn_ctx *ctx, const float *t, float *extra, const int32_t *labels, const float *boxes,
                            uint64_t row0, uint64_t K, uint64_t image_h, uint64_t image_w)
{
    const rn_mask_head *h = (const rn_mask_head *)s->head;
    const rn_mask_request *q = (const rn_mask_request *)s->req;
    const uint64_t M = s->tower->M, plane = image_h * image_w;
    float *probs = q->probs ? q->probs + row0 * 4 * M * M : extra;
    RN_TRY(predict_launch(ctx, t, labels, h->lw, h->lb, K, M, h->Cr, h->C, probs, "rn_mask_head (predict)"));
    if (!q->masks && !q->bits) return RN_OK;
    return paste_launch(ctx, probs, boxes, labels, K, 2 * M, image_h, image_w, q->threshold, q->masks ? q->masks + row0 * plane : NULL,
                        q->bits ? q->bits + row0 * plane : NULL, "rn_mask_head (paste)");
}

void rn_mask_head_slot(rn_mask_head *h, const rn_mask_request *q, rn_roi_head *s)
{
    *s = {};
    if (!h) return;
    s->who = "mask", s->stage = "mask_stage", s->tower = &h->tower, s->head = h, s->req = q;
    s->check = mask_head_check, s->operands = mask_head_operands, s->behind = mask_head_behind;
    if (q) s->pool = {q->n_levels, q->level, q->sampling_ratio, q->aligned, q->canonical_scale, q->canonical_level, q->rois, q->pooled};
}

int rn_mask_head_forward(rn_mask_head *h, const float *pooled_nhwc, const int32_t *labels, const float *boxes, uint64_t K,
                         uint64_t image_h, uint64_t image_w, const rn_mask_request *req)
{
    if (!h) return RN_ERR_INVALID;
    rn_ctx *ctx = h->tower.ctx;
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, h->tower.finalized, "the mask head is not finalized");
    rn_roi_head s;
    rn_mask_head_slot(h, req, &s);
    RN_TRY(mask_head_check(&s, ctx, __func__, K, boxes != NULL, image_h, image_w));
    if (K == 0) return RN_OK;
    operand ops[RN_ROI_HEAD_OPERANDS + 3];
    mask_head_operands(&s, K, image_h, image_w, ops);
    ops[0].ptr = ops[1].ptr = NULL;  // the request's rois and pooled are the route's: nothing here writes them
    ops[5] = {pooled_nhwc, K * h->tower.M * h->tower.M * h->tower.Cin * 4, "pooled_nhwc", false, false};
    ops[6] = {labels, K * 4, "labels", false, false};
    ops[7] = {boxes, K * 16, "boxes", false, false};
    return rn_roi_head_forward(&s, __func__, pooled_nhwc, labels ? NULL : "labels is NULL", ops, RN_ROI_HEAD_OPERANDS + 3, labels, boxes,
                               K, image_h, image_w);
}

}  // extern "C"
