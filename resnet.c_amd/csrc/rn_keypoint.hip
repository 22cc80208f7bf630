// The keypoint branch of a two-stage detector behind the box head: torchvision's KeypointRCNNHeads and
// KeypointRCNNPredictor, keypointrcnn_inference and heatmaps_to_keypoints.  The convolutions are the library's
// contractions (the transposed one, kernel 4 at stride 2 and padding 1, as ONE 1x1 panel of 16 * Kp channels that holds
// the products only: its taps overlap); one kernel is this file's:
//   keypoint_kernel: one block per (detection, keypoint).  From the panel's output it adds the at most 2 x 2 taps of
//     every pixel of the 2M x 2M map, resizes that bilinearly to S x S (S = 4M) in LDS, and -- the search -- resizes the
//     S x S map bicubically to the size of the detection's own box and takes the argmax.  The resized map never exists:
//     a chunk of 128 output columns at a time, the horizontal pass of all S source rows goes to LDS and the vertical pass
//     of every output row of the chunk feeds a running (value, index) maximum.  The same kernel searches a caller's
//     heat maps (rn_heatmaps_to_keypoints_forward).
// No atomics anywhere.  The reference classifies whole images only; nothing here has a counterpart in it.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "rn_conv_params.h"
#include "rn_internal.h"
#include "rn_private.h"

// The arithmetic of both resizes and of the keypoint's coordinates is a contract (rn_hip.h): no product of this file is
// fused into an add.
#pragma clang fp contract(off)

namespace {

constexpr uint32_t kKpBlock = 256;
constexpr uint32_t kKpMaxM = 16;     // the head's resolution: S = 4M is at most kKpMaxS
constexpr uint32_t kKpMaxS = 64;     // the side of a heat map the search reads
constexpr uint32_t kKpMaxKp = 256;   // keypoints
constexpr uint32_t kKpMaxSide = 8192;  // max_h, max_w: the image a box is resized into
constexpr uint32_t kKpChunk = 128;   // output columns of one pass of the search
constexpr uint32_t kKpNone = 0xffffffffu;

struct keypoint_args {
    const float4 *t;        // [K, M, M, 16 * Kp], or NULL: heat_in holds the heat maps
    const float *bias;      // [Kp]
    const float *heat_in;   // [K, Kp, S, S]
    const float *boxes;     // [K, 4]
    const int32_t *labels;  // [K] or NULL
    float *heat_out;        // [K, Kp, S, S] or NULL
    float *keypoints;       // [K, Kp, 3] or NULL (no search)
    float *scores;          // [K, Kp]
    uint32_t K, M, Kp, S, max_h, max_w;
};

// rn_upsample_bilinear_forward's per-axis rule at scale 0.5: the index pair and the second's weight
__device__ __forceinline__ void kp_linear(uint32_t o, uint32_t n_in, uint32_t *i0, uint32_t *i1, float *l1)
{
    const float c = (float)o + 0.5f;
    float s = 0.5f * c - 0.5f;
    s = s > 0.0f ? s : 0.0f;
    uint32_t a = (uint32_t)(int)s;
    if (a > n_in - 1) a = n_in - 1;
    *i0 = a;
    *i1 = a + 1 < n_in ? a + 1 : n_in - 1;
    *l1 = s - (float)a;
}

// torch's cubic rule (A = -0.75, the source coordinate not clamped at 0) for output index o of an axis resized from
// n_in by `scale`: the four taps, each clamped to [0, n_in), and their coefficients
__device__ __forceinline__ void kp_cubic(uint32_t o, float scale, uint32_t n_in, uint32_t idx[4], float cf[4])
{
    const float A = -0.75f;
    const float src = scale * ((float)o + 0.5f) - 0.5f;
    const float fl = floorf(src);
    const float tt = src - fl;
    const int i = (int)fl;  // |src| < 64 * 8192
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int q = i - 1 + e;
        q = q < 0 ? 0 : q;
        idx[e] = (uint32_t)q > n_in - 1 ? n_in - 1 : (uint32_t)q;  // unconditional: nothing a box holds indexes outside the map
    }
    float x = tt + 1.0f;
    cf[0] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
    x = tt;
    cf[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    x = 1.0f - tt;
    cf[2] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    x = 2.0f - tt;
    cf[3] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
}

// b replaces a where it is greater, or equal at a lower index: a total order on what the search keeps (never a NaN),
// so the result does not depend on which thread saw which pixel
__device__ __forceinline__ void kp_take(float *best, uint32_t *bidx, float v, uint32_t i)
{
    if (v > *best || (v == *best && i < *bidx)) *best = v, *bidx = i;
}

__global__ __launch_bounds__(kKpBlock) void keypoint_kernel(const keypoint_args p)
{
    __shared__ __attribute__((aligned(16))) float heat[kKpMaxS * kKpMaxS];
    // the panel's 16 columns [M * M][16] and the low-resolution map [2M][2M] behind them; then the search's row values
    // [S][kKpChunk]
    __shared__ __attribute__((aligned(16))) float work[kKpMaxS * kKpChunk];
    __shared__ float red_v[kKpBlock / 64];
    __shared__ uint32_t red_i[kKpBlock / 64];
    const uint32_t tid = threadIdx.x, j = blockIdx.x, S = p.S, SS = S * S;
    for (uint32_t k = blockIdx.y; k < p.K; k += gridDim.y) {
        const uint64_t plane = ((uint64_t)k * p.Kp + j) * SS;
        if (p.t) {
            const uint32_t M = p.M, MM = M * M, L = 2 * M, pitch = 4 * p.Kp;
            float4 *tile = reinterpret_cast<float4 *>(work);
            float *low = work + 16 * MM;
            const float4 *src = p.t + (uint64_t)k * MM * pitch + 4 * j;
            for (uint32_t i = tid; i < 4 * MM; i += kKpBlock) tile[i] = src[(uint64_t)(i >> 2) * pitch + (i & 3)];
            __syncthreads();
            const float b = p.bias[j];
            for (uint32_t i = tid; i < L * L; i += kKpBlock) {
                const uint32_t oy = i / L, ox = i - oy * L;
                float v = b;
#pragma unroll
                for (uint32_t ky = 0; ky < 4; ++ky) {
                    const int iy2 = (int)oy + 1 - (int)ky;  // 2 * iy
                    if ((iy2 & 1) || iy2 < 0 || iy2 >= (int)L) continue;
#pragma unroll
                    for (uint32_t kx = 0; kx < 4; ++kx) {
                        const int ix2 = (int)ox + 1 - (int)kx;
                        if ((ix2 & 1) || ix2 < 0 || ix2 >= (int)L) continue;
                        v = v + work[((uint32_t)(iy2 >> 1) * M + (uint32_t)(ix2 >> 1)) * 16 + ky * 4 + kx];
                    }
                }
                low[i] = v;
            }
            __syncthreads();
            for (uint32_t i = tid; i < SS; i += kKpBlock) {
                const uint32_t y = i / S, x = i - y * S;
                uint32_t r0, r1, c0, c1;
                float a1, b1;
                kp_linear(y, L, &r0, &r1, &a1);
                kp_linear(x, L, &c0, &c1, &b1);
                const float a0 = 1.0f - a1, b0 = 1.0f - b1;
                const float top = b0 * low[r0 * L + c0] + b1 * low[r0 * L + c1];
                const float bot = b0 * low[r1 * L + c0] + b1 * low[r1 * L + c1];
                const float v = a0 * top + a1 * bot;
                heat[i] = v;
                if (p.heat_out) p.heat_out[plane + i] = v;
            }
        } else {
            for (uint32_t i = tid; i < SS; i += kKpBlock) heat[i] = p.heat_in[plane + i];
        }
        __syncthreads();
        if (p.keypoints) {
            const float *bx = p.boxes + (uint64_t)k * 4;
            const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
            float w = x2 - x1, h = y2 - y1;
            w = w > 1.0f ? w : 1.0f, h = h > 1.0f ? h : 1.0f;
            const float cw = ceilf(w), ch = ceilf(h);
            bool live = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
            live = live && cw <= (float)p.max_w && ch <= (float)p.max_h;  // (an overflow of the difference: inf)
            live = live && (!p.labels || p.labels[k] >= 1);                 // uniform in the block
            float *kp = p.keypoints + ((uint64_t)k * p.Kp + j) * 3, *sc = p.scores + (uint64_t)k * p.Kp + j;
            if (!live) {
                if (tid == 0) kp[0] = 0.0f, kp[1] = 0.0f, kp[2] = 0.0f, *sc = 0.0f;
            } else {
                const uint32_t Wr = (uint32_t)(int)cw, Hr = (uint32_t)(int)ch;
                const float sx = (float)S / (float)Wr, sy = (float)S / (float)Hr;
                const uint32_t c = tid & (kKpChunk - 1), half = tid / kKpChunk;
                float best = -INFINITY, v0 = 0.0f;
                uint32_t bidx = kKpNone;
                for (uint32_t x0 = 0; x0 < Wr; x0 += kKpChunk) {
                    const uint32_t x = x0 + c;
                    const bool on = x < Wr;
                    uint32_t id[4];
                    float cf[4];
                    if (on) {
                        kp_cubic(x, sx, S, id, cf);
                        for (uint32_t r = half; r < S; r += kKpBlock / kKpChunk) {
                            const float *hr = heat + r * S;
                            work[r * kKpChunk + c] = ((cf[0] * hr[id[0]] + cf[1] * hr[id[1]]) + cf[2] * hr[id[2]]) + cf[3] * hr[id[3]];
                        }
                    }
                    __syncthreads();
                    if (on) {
                        for (uint32_t y = half; y < Hr; y += kKpBlock / kKpChunk) {
                            kp_cubic(y, sy, S, id, cf);
                            const float v = ((cf[0] * work[id[0] * kKpChunk + c] + cf[1] * work[id[1] * kKpChunk + c]) +
                                             cf[2] * work[id[2] * kKpChunk + c]) + cf[3] * work[id[3] * kKpChunk + c];
                            const uint32_t flat = y * Wr + x;
                            if (flat == 0) v0 = v;  // thread 0 alone
                            kp_take(&best, &bidx, v, flat);
                        }
                    }
                    __syncthreads();
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const float ov = __shfl_xor(best, off, 64);
                    const uint32_t oi = __shfl_xor(bidx, off, 64);
                    kp_take(&best, &bidx, ov, oi);
                }
                if ((tid & 63) == 0) red_v[tid >> 6] = best, red_i[tid >> 6] = bidx;
                __syncthreads();
                if (tid == 0) {
                    for (uint32_t q = 1; q < kKpBlock / 64; ++q) kp_take(&best, &bidx, red_v[q], red_i[q]);
                    // the search starts at index 0 and a value replaces the best only where it is greater: a NaN there stays
                    if (v0 != v0 || bidx == kKpNone) best = v0, bidx = 0;
                    const uint32_t yi = bidx / Wr, xi = bidx - yi * Wr;
                    kp[0] = ((float)xi + 0.5f) * (w / (float)Wr) + x1;
                    kp[1] = ((float)yi + 0.5f) * (h / (float)Hr) + y1;
                    kp[2] = 1.0f;
                    *sc = best;
                }
            }
        }
        __syncthreads();  // the next detection of the block reuses the maps
    }
}

int keypoint_launch(rn_ctx *ctx, const float *t, const float *bias, const float *heat_in, const float *boxes, const int32_t *labels,
                    uint64_t K, uint64_t M, uint64_t Kp, uint64_t S, uint64_t max_h, uint64_t max_w, float *heat_out,
                    float *keypoints, float *scores, const char *what)
{
    keypoint_args a;
    memset(&a, 0, sizeof(a));
    a.t = (const float4 *)t, a.bias = bias, a.heat_in = heat_in, a.boxes = boxes, a.labels = labels;
    a.heat_out = heat_out, a.keypoints = keypoints, a.scores = scores;
    a.K = (uint32_t)K, a.M = (uint32_t)M, a.Kp = (uint32_t)Kp, a.S = (uint32_t)S, a.max_h = (uint32_t)max_h, a.max_w = (uint32_t)max_w;
    const dim3 grid((unsigned)Kp, (unsigned)(K < 65535 ? K : 65535));
    keypoint_kernel<<<grid, kKpBlock, 0, ctx->stream>>>(a);
    return rn_after_launch(ctx, what);
}

// every refusal of the search's shapes; fn: the entry point's name
int keypoint_check(rn_ctx *ctx, const char *fn, uint64_t K, uint64_t Kp, uint64_t max_h, uint64_t max_w)
{
    const char *why = NULL;
    if (Kp < 1 || Kp > kKpMaxKp) why = "Kp must be 1..256";
    else if (max_h < 1 || max_h > kKpMaxSide || max_w < 1 || max_w > kKpMaxSide) why = "max_h and max_w must be 1..8192";
    else if (K >= (1ull << 24)) why = "K must be below 2^24";
    if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
    return RN_OK;
}

}  // namespace

extern "C" {

int rn_keypoint_predict_forward(rn_ctx *ctx, const float *t, const float *bias, const float *boxes, const int32_t *labels, uint64_t K,
                                uint64_t M, uint64_t Kp, uint64_t max_h, uint64_t max_w, float *heat, float *keypoints, float *scores)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, M >= 1 && M <= kKpMaxM, "M must be 1..16");
    RN_TRY(keypoint_check(ctx, __func__, K, Kp, max_h, max_w));
    RN_REQUIRE(ctx, heat || keypoints || scores, "heat, keypoints and scores are all NULL");
    RN_REQUIRE(ctx, (keypoints != NULL) == (scores != NULL), "keypoints and scores come together");
    if (K == 0) return RN_OK;
    RN_REQUIRE(ctx, t, "t is NULL");
    RN_REQUIRE(ctx, bias, "bias is NULL");
    RN_REQUIRE(ctx, !keypoints || boxes, "boxes is NULL");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(t) & 15) == 0, "t is off a 16-byte boundary");
    const operand ops[7] = {{heat, K * Kp * 16 * M * M * 4, "heat", true, false},
                            {keypoints, K * Kp * 12, "keypoints", true, false},
                            {scores, K * Kp * 4, "scores", true, false},
                            {t, K * M * M * 16 * Kp * 4, "t", false, false},
                            {bias, Kp * 4, "bias", false, false},
                            {keypoints ? boxes : NULL, K * 16, "boxes", false, false},
                            {keypoints ? labels : NULL, K * 4, "labels", false, false}};
    RN_TRY(check_operands(ctx, __func__, ops, 7));
    return keypoint_launch(ctx, t, bias, NULL, boxes, labels, K, M, Kp, 4 * M, max_h, max_w, heat, keypoints, scores, __func__);
}

int rn_heatmaps_to_keypoints_forward(rn_ctx *ctx, const float *heat, const float *boxes, const int32_t *labels, uint64_t K, uint64_t Kp,
                                     uint64_t S, uint64_t max_h, uint64_t max_w, float *keypoints, float *scores)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, S >= 1 && S <= kKpMaxS, "S must be 1..64");
    RN_TRY(keypoint_check(ctx, __func__, K, Kp, max_h, max_w));
    if (K == 0) return RN_OK;
    RN_REQUIRE(ctx, heat, "heat is NULL");
    RN_REQUIRE(ctx, boxes, "boxes is NULL");
    RN_REQUIRE(ctx, keypoints, "keypoints is NULL");
    RN_REQUIRE(ctx, scores, "scores is NULL");
    const operand ops[5] = {{keypoints, K * Kp * 12, "keypoints", true, false},
                            {scores, K * Kp * 4, "scores", true, false},
                            {heat, K * Kp * S * S * 4, "heat", false, false},
                            {boxes, K * 16, "boxes", false, false},
                            {labels, K * 4, "labels", false, false}};
    RN_TRY(check_operands(ctx, __func__, ops, 5));
    return keypoint_launch(ctx, NULL, NULL, heat, boxes, labels, K, 0, Kp, S, max_h, max_w, NULL, keypoints, scores, __func__);
}

// ---- the object: KeypointRCNNHeads (the RoI tower of rn_stage.hip) and kps_score_lowres in front of the predict launch ----
struct rn_keypoint_head {
    rn_roi_tower tower;  // its panel: the transposed convolution as ONE 1x1 Clast -> 16 Kp, no shift, no ReLU; no extra tensor;
                         // its table behind the layers: kps_score_lowres: 2n, 2n + 1
    uint64_t Kp;
    float *bias;         // kps_score_lowres.bias on the device
};

// torchvision's Sequential of (conv, ReLU) pairs: layer i is "keypoint_head.{2i}"
static void keypoint_layer_key(int i, const char *leaf, char key[RN_PARAM_KEY], char alt[RN_PARAM_KEY])
{
    snprintf(key, RN_PARAM_KEY, "keypoint_head.%d.%s", 2 * i, leaf);
    alt[0] = 0;
}

int rn_keypoint_head_create(rn_ctx *ctx, rn_keypoint_head **out, uint64_t in_channels, uint64_t n_layers, const uint64_t *layer_channels,
                            uint64_t keypoints, uint64_t resolution)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    RN_TRY(rn_roi_tower_check(ctx, __func__, in_channels, n_layers, layer_channels,
                              keypoints >= 1 && keypoints <= kKpMaxKp ? NULL : "keypoints must be 1..256", resolution, kKpMaxM));
    rn_keypoint_head *h = (rn_keypoint_head *)calloc(1, sizeof(*h));
    if (!h) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_keypoint_head_create: out of host memory");
    h->Kp = keypoints;
    rn_roi_tower *t = &h->tower;
    t->name = "rn_keypoint_head", t->what = "the keypoint head", t->panel = 16 * keypoints, t->panel_relu = 0, t->extra_floats = 0;
    rn_roi_tower_init(t, ctx, in_channels, n_layers, layer_channels, resolution, keypoint_layer_key);
    const uint64_t last = t->ch[n_layers - 1];
    rn_params_add(&t->params, "keypoint_predictor.kps_score_lowres.weight", NULL, last, keypoints * 16, last, keypoints * 16, 0.0f);
    rn_params_add(&t->params, "keypoint_predictor.kps_score_lowres.bias", NULL, 1, keypoints, 1, keypoints, 0.0f);
    *out = h;
    return RN_OK;
}

int rn_keypoint_head_set_tensor(rn_keypoint_head *h, const char *key, const float *host_data, uint64_t numel)
{
    if (!h) return RN_ERR_INVALID;
    rn_roi_tower *t = &h->tower;
    return rn_stage_set_tensor(t->ctx, __func__, t->what, t->finalized, &t->params, key, host_data, numel);
}

int rn_keypoint_head_finalize(rn_keypoint_head *h)
{
    if (!h) return RN_ERR_INVALID;
    rn_roi_tower *t = &h->tower;
    rn_ctx *ctx = t->ctx;
    RN_ENTER(ctx);
    if (t->finalized) return RN_OK;
    RN_TRY(rn_roi_tower_pack_layers(t, __func__));
    const uint64_t n = t->n_layers, Kp = h->Kp, last = t->ch[n - 1];
    const rn_params_entry *p = t->params.p;
    // ConvTranspose2d(last, Kp, 4, 2, 1), weight [last, Kp, 4, 4]: the 1x1 convolution whose row k * 16 + ky * 4 + kx is
    // W[:, k, ky, kx] holds every product; output (oy, ox) adds the taps with 2 iy = oy + 1 - ky, 2 ix = ox + 1 - kx
    float *w = (float *)malloc(16 * Kp * last * sizeof(float));
    if (!w) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_keypoint_head_finalize: out of host memory");
    const float *dw = p[2 * n].host;
    for (uint64_t r = 0; r < 16 * Kp; ++r)
        for (uint64_t ci = 0; ci < last; ++ci) w[r * last + ci] = dw[ci * 16 * Kp + r];
    int st = rn_roi_tower_pack_panel(t, w, NULL);
    free(w);
    if (st == RN_OK && !h->bias) st = rn_malloc(ctx, (void **)&h->bias, Kp * sizeof(float));
    if (st == RN_OK) st = rn_ctx_upload_sync(ctx, h->bias, p[2 * n + 1].host, Kp * sizeof(float));
    if (st != RN_OK) return st;
    rn_params_free(&t->params);
    t->finalized = 1;
    return RN_OK;
}

int rn_keypoint_head_destroy(rn_keypoint_head *h)
{
    if (!h) return RN_OK;
    rn_ctx *ctx = h->tower.ctx;
    RN_ENTER(ctx);
    RN_TRY(rn_sync(ctx));
    rn_roi_tower_free(&h->tower);
    rn_free_null(ctx, (void **)&h->bias);
    free(h);
    return RN_OK;
}

// ---- what differs from another RoI head (rn_private.h: rn_roi_head) ----

// every refusal that concerns the request and the shapes alone, for `rows` detections
static int keypoint_head_check(const rn_roi_head *s, rn_ctx *ctx, const char *fn, uint64_t rows, int boxes_given, uint64_t image_h,
                               uint64_t image_w)
{
    const rn_keypoint_request *q = (const rn_keypoint_request *)s->req;
    if (!q) return rn_set_error(ctx, RN_ERR_INVALID, "%s: the keypoint request is NULL", fn);
    const char *why = NULL;
    if (!q->heat && !q->keypoints && !q->scores) why = "heat, keypoints and scores of the keypoint request are all NULL";
    else if ((q->keypoints != NULL) != (q->scores != NULL)) why = "keypoints and scores of the keypoint request come together";
    else if (q->keypoints && !boxes_given) why = "boxes is NULL and the keypoint request wants keypoints";
    if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
    return keypoint_check(ctx, fn, rows, ((const rn_keypoint_head *)s->head)->Kp, image_h, image_w);
}

static int keypoint_head_operands(const rn_roi_head *s, uint64_t rows, uint64_t, uint64_t, rn_operand ops[RN_ROI_HEAD_OPERANDS])
{
    const rn_keypoint_request *q = (const rn_keypoint_request *)s->req;
    const uint64_t M = s->tower->M, Kp = ((const rn_keypoint_head *)s->head)->Kp;
    ops[0] = {q->rois, rows * 20, "keypoint.rois", true, false};
    ops[1] = {q->pooled, rows * M * M * s->tower->Cin * 4, "keypoint.pooled", true, false};
    ops[2] = {q->heat, rows * Kp * 16 * M * M * 4, "keypoint.heat", true, false};
    ops[3] = {q->keypoints, rows * Kp * 12, "keypoint.keypoints", true, false};
    ops[4] = {q->scores, rows * Kp * 4, "keypoint.scores", true, false};
    return RN_ROI_HEAD_OPERANDS;
}

// the predict launch
static int keypoint_head_behind(const rn_roi_head *s, rn_ctx *ctx, const float *t, float *, const int32_t *labels, const float *boxes,
                                uint64_t row0, uint64_t K, uint64_t image_h, uint64_t image_w)
{
    const rn_keypoint_head *h = (const rn_keypoint_head *)s->head;
    const rn_keypoint_request *q = (const rn_keypoint_request *)s->req;
    const uint64_t M = s->tower->M, Kp = h->Kp;
    return keypoint_launch(ctx, t, h->bias, NULL, boxes, labels, K, M, Kp, 4 * M, image_h, image_w,
                           q->heat ? q->heat + row0 * Kp * 16 * M * M : NULL, q->keypoints ? q->keypoints + row0 * Kp * 3 : NULL,
                           q->scores ? q->scores + row0 * Kp : NULL, "rn_keypoint_head (predict)");
}

void rn_keypoint_head_slot(rn_keypoint_head *h, const rn_keypoint_request *q, rn_roi_head *s)
{
    *s = {};
    if (!h) return;
    s->who = "keypoint", s->stage = "keypoint_stage", s->tower = &h->tower, s->head = h, s->req = q;
    s->check = keypoint_head_check, s->operands = keypoint_head_operands, s->behind = keypoint_head_behind;
    if (q) s->pool = {q->n_levels, q->level, q->sampling_ratio, q->aligned, q->canonical_scale, q->canonical_level, q->rois, q->pooled};
}

int rn_keypoint_head_forward(rn_keypoint_head *h, const float *pooled_nhwc, const int32_t *labels, const float *boxes, uint64_t K,
                             uint64_t image_h, uint64_t image_w, const rn_keypoint_request *req)
{
    if (!h) return RN_ERR_INVALID;
    rn_ctx *ctx = h->tower.ctx;
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, h->tower.finalized, "the keypoint head is not finalized");
    rn_roi_head s;
    rn_keypoint_head_slot(h, req, &s);
    RN_TRY(keypoint_head_check(&s, ctx, __func__, K, boxes != NULL, image_h, image_w));
    const uint64_t M = h->tower.M;
    RN_REQUIRE(ctx, K * M * M < (1ull << 31), "K * M * M must be below 2^31");
    if (K == 0) return RN_OK;
    operand ops[RN_ROI_HEAD_OPERANDS + 3];
    keypoint_head_operands(&s, K, image_h, image_w, ops);
    ops[0].ptr = ops[1].ptr = NULL;  // the request's rois and pooled are the route's: nothing here writes them
    ops[5] = {pooled_nhwc, K * M * M * h->tower.Cin * 4, "pooled_nhwc", false, false};
    ops[6] = {req->keypoints ? labels : NULL, K * 4, "labels", false, false};
    ops[7] = {req->keypoints ? boxes : NULL, K * 16, "boxes", false, false};
    return rn_roi_head_forward(&s, __func__, pooled_nhwc, NULL, ops, RN_ROI_HEAD_OPERANDS + 3, labels, boxes, K, image_h, image_w);
}

}  // extern "C"
