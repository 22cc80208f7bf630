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

// ---- the object: MaskRCNNHeads and MaskRCNNPredictor in front of the predict and paste launches ------------------
enum { kMaskMaxLayers = 8, kMaskRows = 0, kMaskPool = 1, kMaskScratch = 6 };

struct rn_mask_head {
    rn_ctx *ctx;
    uint64_t Cin, n_layers, ch[kMaskMaxLayers], Cr, C, M;
    int finalized;
    rn_params params;                   // layer i: 2i, 2i + 1; conv5_mask: 2n, 2n + 1; mask_fcn_logits: 2n + 2, 2n + 3
    rn_stage_unit unit[kMaskMaxLayers + 1];  // the 3x3 layers, then the transposed convolution as ONE 1x1 panel Clast -> 4 Cr
                                        // (its shift: conv5_mask's bias four times)
    float *lw, *lb;                     // mask_fcn_logits on the device, torchvision's layout
    // scratch for cap rows: two ping-pong maps [., M, M, widest], the deconvolution's output [., M, M, 4 Cr] and the
    // probabilities [., 2M, 2M] of a forward that does not export them
    float *ping, *pong, *t, *probs;
    float *rois, *pooled;               // behind a neck: the RoI rows [., 5] and the pooled features [., M, M, Cin] of cap_pool rows
    uint64_t cap[2], widest;            // cap: rows (kMaskRows), of them with RoI rows and pooled features (kMaskPool)
};

// the scratch tensors for `rows` detections, `pool` of them behind a neck; returns how many
static int mask_head_scratch(rn_mask_head *h, uint64_t rows, uint64_t pool, rn_scratch_item *list)
{
    const uint64_t px = rows * h->M * h->M;
    list[0] = {(void **)&h->ping, px * h->widest * sizeof(float)};
    list[1] = {(void **)&h->pong, px * h->widest * sizeof(float)};
    list[2] = {(void **)&h->t, px * 4 * h->Cr * sizeof(float)};
    list[3] = {(void **)&h->probs, px * 4 * sizeof(float)};
    list[4] = {(void **)&h->rois, pool * 5 * sizeof(float)};
    list[5] = {(void **)&h->pooled, pool * h->M * h->M * h->Cin * sizeof(float)};
    return kMaskScratch;
}

int rn_mask_head_create(rn_ctx *ctx, rn_mask_head **out, uint64_t in_channels, uint64_t n_layers, const uint64_t *layer_channels,
                        uint64_t dim_reduced, uint64_t classes, uint64_t resolution)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    RN_REQUIRE(ctx, in_channels >= 64 && in_channels % 64 == 0 && in_channels <= 8192, "in_channels must be a multiple of 64 (at most 8192)");
    RN_REQUIRE(ctx, n_layers >= 1 && n_layers <= kMaskMaxLayers, "n_layers must be 1..8");
    RN_REQUIRE(ctx, layer_channels, "layer_channels is NULL");
    for (uint64_t i = 0; i < n_layers; ++i)
        RN_REQUIRE(ctx, layer_channels[i] >= 64 && layer_channels[i] % 64 == 0 && layer_channels[i] <= 8192,
                   "every layer's channels must be a multiple of 64 (at most 8192)");
    RN_REQUIRE(ctx, dim_reduced >= 64 && dim_reduced % 64 == 0 && dim_reduced <= kMaskMaxCr,
               "dim_reduced must be a multiple of 64 up to 1024");
    RN_REQUIRE(ctx, classes >= 2 && classes <= kMaskMaxC, "classes must be 2..1024");
    RN_REQUIRE(ctx, resolution >= 1 && resolution <= kMaskMaxM, "resolution must be 1..32");
    rn_mask_head *h = (rn_mask_head *)calloc(1, sizeof(*h));
    if (!h) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_mask_head_create: out of host memory");
    h->ctx = ctx, h->Cin = in_channels, h->n_layers = n_layers, h->Cr = dim_reduced, h->C = classes, h->M = resolution;
    h->widest = in_channels;
    for (uint64_t i = 0; i < n_layers; ++i) {
        h->ch[i] = layer_channels[i];
        if (h->ch[i] > h->widest) h->widest = h->ch[i];
    }
    // either spelling of a layer ("mask_head.0.0.weight", "mask_head.mask_fcn1.weight"), with or without "roi_heads."
    h->params.prefix = "roi_heads.";
    for (uint64_t i = 0; i < n_layers; ++i)
        for (int j = 0; j < 2; ++j) {
            char key[RN_PARAM_KEY], alt[RN_PARAM_KEY];
            snprintf(key, sizeof(key), "mask_head.%d.0.%s", (int)i, j ? "bias" : "weight");
            snprintf(alt, sizeof(alt), "mask_head.mask_fcn%d.%s", (int)i + 1, j ? "bias" : "weight");
            const uint64_t rows = j ? 1 : h->ch[i], len = j ? h->ch[i] : (i == 0 ? h->Cin : h->ch[i - 1]) * 9;
            rn_params_add(&h->params, key, alt, rows, len, rows, len, 0.0f);
        }
    const uint64_t last = h->ch[n_layers - 1], Cr = dim_reduced;
    rn_params_add(&h->params, "mask_predictor.conv5_mask.weight", NULL, last, Cr * 4, last, Cr * 4, 0.0f);
    rn_params_add(&h->params, "mask_predictor.conv5_mask.bias", NULL, 1, Cr, 1, Cr, 0.0f);
    rn_params_add(&h->params, "mask_predictor.mask_fcn_logits.weight", NULL, classes, Cr, classes, Cr, 0.0f);
    rn_params_add(&h->params, "mask_predictor.mask_fcn_logits.bias", NULL, 1, classes, 1, classes, 0.0f);
    *out = h;
    return RN_OK;
}

int rn_mask_head_set_tensor(rn_mask_head *h, const char *key, const float *host_data, uint64_t numel)
{
    if (!h) return RN_ERR_INVALID;
    return rn_stage_set_tensor(h->ctx, __func__, "the mask head", h->finalized, &h->params, key, host_data, numel);
}

int rn_mask_head_finalize(rn_mask_head *h)
{
    if (!h) return RN_ERR_INVALID;
    rn_ctx *ctx = h->ctx;
    RN_ENTER(ctx);
    if (h->finalized) return RN_OK;
    RN_TRY(rn_stage_all_set(ctx, __func__, &h->params));
    const uint64_t n = h->n_layers, Cr = h->Cr, last = h->ch[n - 1];
    const rn_params_entry *p = h->params.p;
    for (uint64_t i = 0; i < n; ++i)
        RN_TRY(rn_stage_pack(ctx, RN_DTYPE_F32, p[2 * i].host, i == 0 ? h->Cin : h->ch[i - 1], h->ch[i], 3, p[2 * i + 1].host, NULL,
                             &h->unit[i]));
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
    int st = rn_stage_pack(ctx, RN_DTYPE_F32, w, last, 4 * Cr, 1, w + 4 * Cr * last, NULL, &h->unit[n]);
    free(w);
    if (st == RN_OK && !h->lw) st = rn_malloc(ctx, (void **)&h->lw, h->C * Cr * sizeof(float));
    if (st == RN_OK && !h->lb) st = rn_malloc(ctx, (void **)&h->lb, h->C * sizeof(float));
    if (st == RN_OK) st = rn_ctx_upload_sync(ctx, h->lw, p[2 * n + 2].host, h->C * Cr * sizeof(float));
    if (st == RN_OK) st = rn_ctx_upload_sync(ctx, h->lb, p[2 * n + 3].host, h->C * sizeof(float));
    if (st != RN_OK) return st;
    rn_params_free(&h->params);
    h->finalized = 1;
    return RN_OK;
}

int rn_mask_head_destroy(rn_mask_head *h)
{
    if (!h) return RN_OK;
    rn_ctx *ctx = h->ctx;
    RN_ENTER(ctx);
    RN_TRY(rn_sync(ctx));
    rn_scratch_item list[kMaskScratch];
    rn_stage_free_list(ctx, list, mask_head_scratch(h, 0, 0, list));
    rn_params_free(&h->params);
    for (int i = 0; i <= kMaskMaxLayers; ++i) rn_stage_unit_free(ctx, &h->unit[i]);
    rn_free_null(ctx, (void **)&h->lw), rn_free_null(ctx, (void **)&h->lb);
    free(h);
    return RN_OK;
}

// ---- library-internal (rn_private.h) ----

int rn_mask_head_matches(const rn_mask_head *h, const rn_ctx *ctx, uint64_t in_channels, const char **why)
{
    const char *w = NULL;
    if (!h) w = "the mask head is NULL";
    else if (!h->finalized) w = "the mask head is not finalized";
    else if (h->ctx->device != ctx->device) w = "the mask head's context is on another device";
    else if (h->Cin != in_channels) w = "the mask head's in_channels is not the neck's out_channels";
    if (why) *why = w;
    return w == NULL;
}

uint64_t rn_mask_head_resolution(const rn_mask_head *h) { return h->M; }

// the object's scratch for `rows` detections (rn_stage_grow's rule); with_pool: the RoI rows and the pooled features of a
// forward behind a neck as well
int rn_mask_head_reserve(rn_mask_head *h, uint64_t rows, int with_pool)
{
    if (rows <= h->cap[kMaskRows] && (!with_pool || rows <= h->cap[kMaskPool])) return RN_OK;
    const uint64_t want[2] = {rows > h->cap[kMaskRows] ? rows : h->cap[kMaskRows],
                              with_pool && rows > h->cap[kMaskPool] ? rows : h->cap[kMaskPool]};
    rn_scratch_item list[kMaskScratch];
    return rn_stage_grow(h->ctx, "rn_mask_head", list, mask_head_scratch(h, want[kMaskRows], want[kMaskPool], list), h->cap, want, 2);
}

// every refusal that concerns the request and the shapes alone, for `rows` detections
int rn_mask_head_check(const rn_mask_head *h, rn_ctx *ctx, const char *fn, const rn_mask_request *q, uint64_t rows,
                       int paste_possible, uint64_t image_h, uint64_t image_w)
{
    if (!q) return rn_set_error(ctx, RN_ERR_INVALID, "%s: the mask request is NULL", fn);
    const char *why = NULL;
    if (!q->probs && !q->masks && !q->bits) why = "probs, masks and bits of the mask request are all NULL";
    else if ((q->masks || q->bits) && !paste_possible) why = "boxes is NULL and the mask request wants pasted masks";
    else if (rows >= (1ull << 31) || rows * h->M * h->M >= (1ull << 31)) why = "K * M * M must be below 2^31";
    if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
    if (q->masks || q->bits) RN_TRY(paste_check(ctx, fn, rows, 2 * h->M, image_h, image_w, q->threshold));
    return RN_OK;
}

int rn_mask_head_operands(const rn_mask_head *h, const rn_mask_request *q, uint64_t rows, uint64_t image_h, uint64_t image_w,
                          rn_operand ops[RN_MASK_HEAD_OPERANDS])
{
    const uint64_t M = h->M, plane = (q->masks || q->bits) ? image_h * image_w : 0;
    ops[0] = {q->rois, rows * 20, "mask.rois", true, false};
    ops[1] = {q->pooled, rows * M * M * h->Cin * 4, "mask.pooled", true, false};
    ops[2] = {q->probs, rows * 4 * M * M * 4, "mask.probs", true, false};
    ops[3] = {q->masks, rows * plane * 4, "mask.masks", true, false};
    ops[4] = {q->bits, rows * plane, "mask.bits", true, true};
    return RN_MASK_HEAD_OPERANDS;
}

// The head's launches on ctx for K detections whose scratch starts sub0 rows into the object's tensors: n_layers + 1
// contractions, the predict launch, the paste where masks or bits is given.  ctx->layout is NHWC.
int rn_mask_head_step(rn_mask_head *h, rn_ctx *ctx, const float *pooled_nhwc, const int32_t *labels, const float *boxes,
                      uint64_t sub0, uint64_t K, uint64_t image_h, uint64_t image_w, float threshold, float *probs_out,
                      float *masks, uint8_t *bits)
{
    if (sub0 + K > h->cap[kMaskRows]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_mask_head: scratch not reserved");
    const uint64_t M = h->M, px0 = sub0 * M * M;
    float *ping = h->ping + px0 * h->widest, *pong = h->pong + px0 * h->widest, *t = h->t + px0 * 4 * h->Cr;
    rn_epilogue ep;
    ep.scale = NULL, ep.residual = NULL, ep.relu = 1;
    const float *x = pooled_nhwc;
    uint64_t cin = h->Cin;
    for (uint64_t i = 0; i < h->n_layers; ++i) {
        float *y = i % 2 == 0 ? ping : pong;
        ep.shift = h->unit[i].shift;
        RN_TRY(rn_conv2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, RN_DTYPE_F32, x, y, h->unit[i].packed, 3, 1, 1, M, M, K, cin, h->ch[i], M, M, &ep));
        x = y, cin = h->ch[i];
    }
    ep.shift = h->unit[h->n_layers].shift;
    RN_TRY(rn_conv2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, RN_DTYPE_F32, x, t, h->unit[h->n_layers].packed, 1, 1, 0, M, M, K, cin, 4 * h->Cr, M, M, &ep));
    float *probs = probs_out ? probs_out : h->probs + px0 * 4;
    RN_TRY(predict_launch(ctx, t, labels, h->lw, h->lb, K, M, h->Cr, h->C, probs, "rn_mask_head (predict)"));
    if (!masks && !bits) return RN_OK;
    return paste_launch(ctx, probs, boxes, labels, K, 2 * M, image_h, image_w, threshold, masks, bits, "rn_mask_head (paste)");
}

// The stage behind a neck for the B images from the caller's image img0 on (D detections each), whose scratch starts
// sub0 images into the object's tensors: the RoIs of these images' detection rows, the NHWC pooler on these images'
// maps (maps[i]: level i of image img0), the head.  boxes, labels and the request's outputs: the whole call's.
int rn_mask_head_stage(rn_mask_head *h, rn_ctx *ctx, uint64_t n_levels, const void *const *maps, const uint64_t *hs,
                       const uint64_t *ws, const float *scales, const float *thr, uint64_t images, uint64_t sub0, uint64_t img0,
                       uint64_t B, uint64_t D, const float *boxes, const int32_t *labels, uint64_t image_h, uint64_t image_w,
                       const rn_mask_request *q)
{
    const uint64_t M = h->M, K = B * D, row0 = img0 * D, srow0 = sub0 * D, feat = M * M * h->Cin;
    if ((!q->rois || !q->pooled) && srow0 + K > h->cap[kMaskPool]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_mask_head: scratch not reserved");
    float *rois = q->rois ? q->rois + row0 * 5 : h->rois + srow0 * 5;
    float *pooled = q->pooled ? q->pooled + row0 * feat : h->pooled + srow0 * feat;
    const uint64_t plane = image_h * image_w;
    RN_TRY(rn_detection_rois_window(ctx, boxes + row0 * 4, labels + row0, img0, B, D, rois));
    RN_TRY(rn_roi_align_nhwc_window(ctx, RN_DTYPE_F32, n_levels, maps, hs, ws, scales, thr, images, img0, B, 1, h->Cin, rois, K, M,
                                    M, q->sampling_ratio, q->aligned, pooled, NULL));
    return rn_mask_head_step(h, ctx, pooled, labels + row0, boxes + row0 * 4, srow0, K, image_h, image_w, q->threshold,
                             q->probs ? q->probs + row0 * 4 * M * M : NULL, q->masks ? q->masks + row0 * plane : NULL,
                             q->bits ? q->bits + row0 * plane : NULL);
}

int rn_mask_head_forward(rn_mask_head *h, const float *pooled_nhwc, const int32_t *labels, const float *boxes, uint64_t K,
                         uint64_t image_h, uint64_t image_w, const rn_mask_request *req)
{
    if (!h) return RN_ERR_INVALID;
    rn_ctx *ctx = h->ctx;
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, h->finalized, "the mask head is not finalized");
    RN_TRY(rn_mask_head_check(h, ctx, __func__, req, K, boxes != NULL, image_h, image_w));
    if (K == 0) return RN_OK;
    RN_REQUIRE(ctx, pooled_nhwc, "pooled_nhwc is NULL");
    RN_REQUIRE(ctx, labels, "labels is NULL");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(pooled_nhwc) & 15) == 0, "pooled_nhwc is off a 16-byte boundary");
    const uint64_t M = h->M;
    operand ops[RN_MASK_HEAD_OPERANDS + 3];
    rn_mask_head_operands(h, req, K, image_h, image_w, ops);
    ops[0].ptr = ops[1].ptr = NULL;  // the request's rois and pooled are the route's: nothing here writes them
    ops[5] = {pooled_nhwc, K * M * M * h->Cin * 4, "pooled_nhwc", false, false};
    ops[6] = {labels, K * 4, "labels", false, false};
    ops[7] = {boxes, K * 16, "boxes", false, false};
    RN_TRY(check_operands(ctx, __func__, ops, RN_MASK_HEAD_OPERANDS + 3));
    RN_TRY(rn_mask_head_reserve(h, K, 0));
    const int saved_layout = ctx->layout;
    ctx->layout = RN_LAYOUT_NHWC;
    const int st = rn_mask_head_step(h, ctx, pooled_nhwc, labels, boxes, 0, K, image_h, image_w, req->threshold, req->probs,
                                     req->masks, req->bits);
    ctx->layout = saved_layout;
    return st;
}

}  // extern "C"
