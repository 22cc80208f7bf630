// The launches between the neck and the pooler of a two-stage detector: torchvision's RegionProposalNetwork in eval
// mode behind its head.  Three kernels and the ops around them:
//   select + decode (rn_rpn_select_decode_forward): per (image, level) the pre_nms_top_n best anchors by logit, in
//     rank order, decoded against their anchors, clipped to the image and marked valid or not;
//   IoU mask + scan (rn_nms_forward): greedy NMS of segments of boxes that are already in score order;
//   IoU mask + scan and merge (rn_rpn_nms_merge_forward): NMS per (image, level), then the post_nms_top_n best
//     survivors of an image over all its levels;
//   rn_box_decode_forward: BoxCoder.decode on its own, the same device function.
// The reference classifies whole images only; nothing here has a counterpart in it.
//
// Order (the code: rn_box_dev.h, shared with rn_detect.hip).  A selection orders 64-bit keys that are unique by construction: a monotone image of the logit in the high
// word (NaN as -inf, -0 as +0), the complement of the index in the low word -- so "greater key" IS rn_topk_forward's
// "(v_i, i) precedes (v_j, j)".  rpn_select_sort finds the k-th key exactly with an MSB-first radix select (8 passes
// of 8 bits, a 256-bin histogram in LDS), gathers the k keys at or above it into LDS and sorts them with a bitonic
// network.  The gather's order (it goes through an LDS counter) never reaches an output: the sort removes it.
// Atomics: integer adds in LDS only.  No floating-point atomics, no atomics on global memory.
#include <math.h>
#include <string.h>

#include "rn_box_dev.h"
#include "rn_conv_params.h"
#include "rn_internal.h"
#include "rn_private.h"

// The arithmetic of the decode, the validity rule and the IoU is a contract, operation by operation (rn_hip.h): no
// product of this file is fused into an add.
#pragma clang fp contract(off)

namespace {

constexpr int kRpnMaxLevels = 5;
constexpr int kRpnMaxAnchors = 12;
constexpr int kNmsScratchSlot = 6;    // the context's scratch slot of the IoU mask

__global__ __launch_bounds__(256) void box_decode_kernel(const float *anchors, const float *deltas, float *boxes, uint64_t N,
                                                         const decode_consts k)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
        float a[4], d[4], o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] = anchors[4 * i + c], d[c] = deltas[4 * i + c];
        rpn_decode(a, d, k, o);
#pragma unroll
        for (int c = 0; c < 4; ++c) boxes[4 * i + c] = o[c];
    }
}

// ---- select + decode ----------------------------------------------------------------------------------------
struct select_args {
    const float *head[kRpnMaxLevels];  // [B,h,w,P]
    uint32_t h[kRpnMaxLevels], w[kRpnMaxLevels], sh[kRpnMaxLevels], sw[kRpnMaxLevels];
    float base[kRpnMaxLevels][kRpnMaxAnchors][4];
    uint32_t L, A, P, pre, mul_a, shr_a;
    decode_consts dc;
    float min_size, logit_thresh;
    int32_t *cand_index;
    float *cand_logit, *cand_box;
    uint8_t *cand_valid;
    int32_t *cand_count;
};

__global__ __launch_bounds__(kRpnBlock) void rpn_select_decode_kernel(const select_args p)
{
    __shared__ sel_smem s;
    const uint32_t l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float *head = p.head[0];
    uint32_t h = p.h[0], w = p.w[0], sh = p.sh[0], sw = p.sw[0];
#pragma unroll
    for (int j = 1; j < kRpnMaxLevels; ++j)
        if (l == (uint32_t)j) head = p.head[j], h = p.h[j], w = p.w[j], sh = p.sh[j], sw = p.sw[j];
    const uint32_t n = h * w * p.A, want = n < p.pre ? n : p.pre;
    const float *img = head + (uint64_t)b * h * w * p.P;
    const int A = (int)p.A;
    const uint32_t P = p.P, mul_a = p.mul_a, shr_a = p.shr_a;
    rpn_select_sort(s, n, want, [=](uint32_t i) {
        const uint32_t pos = rn_gemm::fast_div(i, A, mul_a, shr_a);
        return rpn_key(img[(uint64_t)pos * P + (i - pos * (uint32_t)A)], i);
    });
    const uint64_t seg = ((uint64_t)b * p.L + l) * p.pre;
    for (uint32_t r = tid; r < p.pre; r += kRpnBlock) {
        int32_t index = -1;
        float logit = -INFINITY, box[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool valid = false;
        if (r < want) {
            const uint32_t i = ~(uint32_t)s.keys[r];
            const uint32_t pos = rn_gemm::fast_div(i, A, mul_a, shr_a), a = i - pos * (uint32_t)A;
            const uint32_t y = pos / w, x = pos - y * w;
            const float *px = img + (uint64_t)pos * P;
            index = (int32_t)i;
            logit = px[a];
            float d[4], an[4];
            const float fx = (float)(x * sw), fy = (float)(y * sh);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                d[c] = px[p.A + 4 * a + c];
                an[c] = p.base[l][a][c] + ((c & 1) ? fy : fx);
            }
            rpn_decode(an, d, p.dc, box);
            valid = (box[2] - box[0] >= p.min_size) && (box[3] - box[1] >= p.min_size) && (logit >= p.logit_thresh);
        }
        if (p.cand_index) p.cand_index[seg + r] = index;
        if (p.cand_logit) p.cand_logit[seg + r] = logit;
        if (p.cand_valid) p.cand_valid[seg + r] = valid ? 1 : 0;
        if (p.cand_box) {
#pragma unroll
            for (int c = 0; c < 4; ++c) p.cand_box[(seg + r) * 4 + c] = box[c];
        }
    }
    if (tid == 0 && p.cand_count) p.cand_count[(uint64_t)b * p.L + l] = (int32_t)want;
}

// ---- IoU mask -----------------------------------------------------------------------------------------------
// One wave: rows r0 .. r0 + 63 of a segment against columns c0 .. c0 + 63, c0 >= r0 (the upper triangle); lane j
// forms row r0 + j's 64-bit word: bit q set when column c0 + q comes after the row, is inside the segment and
// overlaps the row by more than the threshold.  Words are stored with vector stores; words[seg][row][nw].
struct mask_args {
    const float *boxes;     // [S, n, 4]
    const int32_t *count;   // [S] rows of a segment that can be valid, or NULL: n
    uint64_t *words;
    uint32_t n, nw;
    float thresh;
};

__global__ __launch_bounds__(64) void nms_mask_kernel(const mask_args p)
{
    __shared__ float cb[64][4];
    const uint32_t cbk = blockIdx.x, rbk = blockIdx.y, sgm = blockIdx.z, lane = threadIdx.x;
    if (cbk < rbk) return;
    uint32_t cnt = p.n;
    if (p.count) {
        const int32_t c = p.count[sgm];
        cnt = c < 0 ? 0u : ((uint32_t)c < p.n ? (uint32_t)c : p.n);
    }
    if (rbk * 64 >= cnt || cbk * 64 >= cnt) return;  // uniform: the scan reads no word of these rows or columns
    const float *seg = p.boxes + (uint64_t)sgm * p.n * 4;
    const uint32_t col = cbk * 64 + lane, row = rbk * 64 + lane;
#pragma unroll
    for (int c = 0; c < 4; ++c) cb[lane][c] = col < cnt ? seg[(uint64_t)col * 4 + c] : 0.0f;
    __syncthreads();
    if (row >= cnt) return;
    const float x1 = seg[(uint64_t)row * 4], y1 = seg[(uint64_t)row * 4 + 1], x2 = seg[(uint64_t)row * 4 + 2],
                y2 = seg[(uint64_t)row * 4 + 3];
    const float area = (x2 - x1) * (y2 - y1);
    uint64_t word = 0;
    for (uint32_t q = 0; q < 64; ++q) {
        const uint32_t c = cbk * 64 + q;
        const float iou = rpn_iou(x1, y1, x2, y2, area, cb[q][0], cb[q][1], cb[q][2], cb[q][3]);
        if (c > row && c < cnt && iou > p.thresh) word |= 1ull << q;
    }
    p.words[((uint64_t)sgm * p.n + row) * p.nw + cbk] = word;
}

// ---- the scan: one wave walks a segment's mask rows ---------------------------------------------------------
// Lane v holds word v of the removed set (n <= 4096: 64 words).  Invalid candidates and rows at or past cnt start
// removed: they neither survive nor suppress.  Per block of 64 rows: the block's own word is resolved in registers
// from the 64 diagonal words (one load), then the rows that survived OR their words into the later lanes.
// Returns this lane's word of the KEPT set.
__device__ uint64_t nms_scan_wave(const uint64_t *words, const uint8_t *valid, uint32_t cnt, uint32_t nw, uint32_t lane)
{
    const uint32_t nb = (cnt + 63) / 64;
    uint64_t removed = ~0ull;
    for (uint32_t c = 0; c < nb; ++c) {
        const uint32_t i = c * 64 + lane;
        const bool ok = i < cnt && (!valid || valid[i] != 0);
        const uint64_t bal = __ballot(ok);
        if (lane == c) removed = ~bal;
    }
    for (uint32_t rb = 0; rb < nb; ++rb) {
        const uint32_t row = rb * 64 + lane;
        const uint64_t *rows = words + (uint64_t)rb * 64 * nw;
        const uint64_t diag = row < cnt ? rows[(uint64_t)lane * nw + rb] : 0ull;
        uint64_t cur = __shfl(removed, (int)rb, 64);
#pragma unroll 1
        for (int j = 0; j < 64; ++j) {
            const uint64_t dj = __shfl(diag, j, 64);
            if (!((cur >> j) & 1ull)) cur |= dj;
        }
        if (lane == rb) removed = cur;
        const uint64_t kept = ~cur;  // rows of this block that survive (rows at or past cnt were removed at the start)
        const bool mine = lane > rb && lane < nb;
#pragma unroll 1
        for (int j0 = 0; j0 < 64; j0 += 8) {
            if (((kept >> j0) & 0xFFull) == 0) continue;  // uniform
            uint64_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                v[u] = (mine && ((kept >> (j0 + u)) & 1ull)) ? rows[(uint64_t)(j0 + u) * nw + lane] : 0ull;
#pragma unroll
            for (int u = 0; u < 8; ++u) removed |= v[u];
        }
    }
    return lane < nb ? ~removed : 0ull;
}

struct scan_args {
    const uint64_t *words;
    const uint8_t *valid;  // [S, n] or NULL
    uint8_t *keep;         // [S, n]
    int32_t *keep_count;   // [S] or NULL
    uint32_t n, nw;
};

__global__ __launch_bounds__(64) void nms_scan_kernel(const scan_args p)
{
    const uint32_t sgm = blockIdx.x, lane = threadIdx.x;
    const uint64_t kept = nms_scan_wave(p.words + (uint64_t)sgm * p.n * p.nw, p.valid ? p.valid + (uint64_t)sgm * p.n : nullptr,
                                        p.n, p.nw, lane);
    for (uint32_t c = 0; c < p.nw; ++c) {
        const uint64_t wd = __shfl(kept, (int)c, 64);
        const uint32_t i = c * 64 + lane;
        if (i < p.n) p.keep[(uint64_t)sgm * p.n + i] = (uint8_t)((wd >> lane) & 1ull);
    }
    uint32_t total = (uint32_t)__popcll(kept);
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
    if (lane == 0 && p.keep_count) p.keep_count[sgm] = (int32_t)total;
}

// ---- scan + merge: one block per image ----------------------------------------------------------------------
struct merge_args {
    const uint64_t *words;      // [B * L segments][pre][nw]
    const float *cand_logit, *cand_box;
    const uint8_t *cand_valid;
    const int32_t *cand_count;  // [B, L]
    uint32_t L, pre, post, nw, mul_pre, shr_pre;
    uint32_t img0;              // the image index of this launch's first image (the RoI rows' first column)
    float *boxes, *logits, *rois;
    int32_t *levels, *count;
    uint8_t *cand_keep;         // [B, L, pre] or NULL
};

__global__ __launch_bounds__(kRpnBlock) void rpn_merge_kernel(const merge_args p)
{
    __shared__ sel_smem s;
    __shared__ uint64_t skeep[kRpnMaxLevels][64];
    __shared__ uint32_t skept[kRpnMaxLevels];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (wave < p.L) {
        const uint64_t sgm = (uint64_t)b * p.L + wave;
        const int32_t c = p.cand_count[sgm];
        const uint32_t cnt = c < 0 ? 0u : ((uint32_t)c < p.pre ? (uint32_t)c : p.pre);
        const uint64_t kept = nms_scan_wave(p.words + sgm * p.pre * p.nw, p.cand_valid + sgm * p.pre, cnt, p.nw, lane);
        skeep[wave][lane] = kept;
        uint32_t total = (uint32_t)__popcll(kept);
        for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
        if (lane == 0) skept[wave] = total;
    }
    __syncthreads();
    uint32_t survivors = 0;
    for (uint32_t l = 0; l < p.L; ++l) survivors += skept[l];
    const uint32_t want = survivors < p.post ? survivors : p.post;
    const uint32_t n = p.L * p.pre;
    const float *logit = p.cand_logit + (uint64_t)b * n;
    const int pre = (int)p.pre;
    const uint32_t mul_pre = p.mul_pre, shr_pre = p.shr_pre;
    if (p.cand_keep) {
        for (uint32_t i = tid; i < n; i += kRpnBlock) {
            const uint32_t l = rn_gemm::fast_div(i, pre, mul_pre, shr_pre), r = i - l * (uint32_t)pre;
            p.cand_keep[(uint64_t)b * n + i] = (uint8_t)((skeep[l][r >> 6] >> (r & 63)) & 1ull);
        }
    }
    if (want > 0) {  // uniform
        rpn_select_sort(s, n, want, [=](uint32_t i) -> uint64_t {
            const uint32_t l = rn_gemm::fast_div(i, pre, mul_pre, shr_pre), r = i - l * (uint32_t)pre;
            if (!((skeep[l][r >> 6] >> (r & 63)) & 1ull)) return 0ull;
            return rpn_key(logit[i], i);
        });
    }
    for (uint32_t r = tid; r < p.post; r += kRpnBlock) {
        float box[4] = {0.0f, 0.0f, 0.0f, 0.0f}, lg = -INFINITY, image = -1.0f;
        int32_t level = -1;
        if (r < want) {
            const uint32_t i = ~(uint32_t)s.keys[r];
            level = (int32_t)rn_gemm::fast_div(i, pre, mul_pre, shr_pre);
            lg = logit[i];
            image = (float)(p.img0 + b);
#pragma unroll
            for (int c = 0; c < 4; ++c) box[c] = p.cand_box[((uint64_t)b * n + i) * 4 + c];
        }
        const uint64_t o = (uint64_t)b * p.post + r;
        if (p.logits) p.logits[o] = lg;
        if (p.levels) p.levels[o] = level;
        if (p.boxes) {
#pragma unroll
            for (int c = 0; c < 4; ++c) p.boxes[o * 4 + c] = box[c];
        }
        if (p.rois) {
            p.rois[o * 5] = image;
#pragma unroll
            for (int c = 0; c < 4; ++c) p.rois[o * 5 + 1 + c] = box[c];
        }
    }
    if (tid == 0 && p.count) p.count[b] = (int32_t)want;
}

// ---- host side ----------------------------------------------------------------------------------------------
int mask_launch(rn_ctx *ctx, const float *boxes, const int32_t *count, uint64_t *words, uint64_t S, uint64_t n, float thresh,
                const char *what)
{
    mask_args p;
    memset(&p, 0, sizeof(p));
    p.boxes = boxes, p.count = count, p.words = words, p.n = (uint32_t)n, p.nw = (uint32_t)rn_ceil_div(n, 64), p.thresh = thresh;
    const dim3 grid(p.nw, p.nw, (unsigned)S);
    nms_mask_kernel<<<grid, 64, 0, ctx->stream>>>(p);
    return rn_after_launch(ctx, what);
}

// the select + decode launch, no checks
int select_launch(rn_ctx *ctx, uint64_t L, const float *const *head_nhwc, uint64_t B, const uint64_t *h, const uint64_t *w,
                  uint64_t A, const float *base_anchors, uint64_t image_h, uint64_t image_w, uint64_t pre, float min_size,
                  float logit_thresh, const rn_rpn_candidates *cand, const char *what)
{
    select_args p;
    memset(&p, 0, sizeof(p));
    for (uint64_t l = 0; l < L; ++l) {
        p.head[l] = head_nhwc[l], p.h[l] = (uint32_t)h[l], p.w[l] = (uint32_t)w[l];
        p.sh[l] = (uint32_t)(image_h / h[l]), p.sw[l] = (uint32_t)(image_w / w[l]);
        for (uint64_t a = 0; a < A; ++a)
            for (int c = 0; c < 4; ++c) p.base[l][a][c] = base_anchors[(l * A + a) * 4 + c];
    }
    p.L = (uint32_t)L, p.A = (uint32_t)A, p.P = (uint32_t)((5 * A + 3) & ~(uint64_t)3), p.pre = (uint32_t)pre;
    rn_fast_div((unsigned)A, &p.mul_a, &p.shr_a);
    p.dc = {1.0f, 1.0f, 1.0f, 1.0f, (float)log(1000.0 / 16.0), (float)image_w, (float)image_h};
    p.min_size = min_size, p.logit_thresh = logit_thresh;
    p.cand_index = cand->index, p.cand_logit = cand->logit, p.cand_box = cand->box, p.cand_valid = cand->valid;
    p.cand_count = cand->count;
    rpn_select_decode_kernel<<<dim3((unsigned)L, (unsigned)B), kRpnBlock, 0, ctx->stream>>>(p);
    return rn_after_launch(ctx, what);
}

// the scan + merge launch, no checks; img0: the image index of the launch's first image
int merge_launch(rn_ctx *ctx, const uint64_t *words, const rn_rpn_candidates *cand, uint64_t B, uint64_t L, uint64_t pre,
                 uint64_t post, uint64_t img0, const rn_rpn_proposals *out, const char *what)
{
    merge_args p;
    memset(&p, 0, sizeof(p));
    p.words = words, p.cand_logit = cand->logit, p.cand_box = cand->box, p.cand_valid = cand->valid, p.cand_count = cand->count;
    p.L = (uint32_t)L, p.pre = (uint32_t)pre, p.post = (uint32_t)post, p.nw = (uint32_t)rn_ceil_div(pre, 64);
    p.img0 = (uint32_t)img0;
    rn_fast_div((unsigned)pre, &p.mul_pre, &p.shr_pre);
    p.boxes = out->boxes, p.logits = out->logits, p.rois = out->rois, p.levels = out->levels, p.count = out->count;
    p.cand_keep = out->cand_keep;
    rpn_merge_kernel<<<(unsigned)B, kRpnBlock, 0, ctx->stream>>>(p);
    return rn_after_launch(ctx, what);
}

}  // namespace

extern "C" {

int rn_box_decode_forward(rn_ctx *ctx, const float *anchors, const float *deltas, uint64_t N, float wx, float wy, float ww,
                          float wh, float image_h, float image_w, float *boxes)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, wx > 0.0f && wy > 0.0f && ww > 0.0f && wh > 0.0f && isfinite(wx) && isfinite(wy) && isfinite(ww) && isfinite(wh),
               "the weights must be positive and finite");
    RN_REQUIRE(ctx, image_h > 0.0f && image_w > 0.0f, "image_h and image_w must be positive (INFINITY: no upper clip)");
    RN_REQUIRE(ctx, N < (1ull << 31), "N must be below 2^31");
    if (N == 0) return RN_OK;
    RN_REQUIRE(ctx, anchors, "anchors is NULL");
    RN_REQUIRE(ctx, deltas, "deltas is NULL");
    RN_REQUIRE(ctx, boxes, "boxes is NULL");
    const operand ops[] = {{anchors, N * 16, "anchors", false, false}, {deltas, N * 16, "deltas", false, false}, {boxes, N * 16, "boxes", true, false}};
    RN_TRY(check_operands(ctx, __func__, ops, 3));
    const decode_consts k = {wx, wy, ww, wh, (float)log(1000.0 / 16.0), image_w, image_h};
    box_decode_kernel<<<rn_stream_grid(N, 256), 256, 0, ctx->stream>>>(anchors, deltas, boxes, N, k);
    return rn_after_launch(ctx, "rn_box_decode_forward");
}

int rn_rpn_select_decode_forward(rn_ctx *ctx, uint64_t L, const float *const *head_nhwc, uint64_t B, const uint64_t *h,
                                 const uint64_t *w, uint64_t A, const float *base_anchors, uint64_t image_h, uint64_t image_w,
                                 uint64_t pre_nms_top_n, float min_size, float logit_thresh, const rn_rpn_candidates *cand)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, L >= 1 && L <= (uint64_t)kRpnMaxLevels, "L must be 1..5");
    RN_REQUIRE(ctx, A >= 1 && A <= (uint64_t)kRpnMaxAnchors, "A must be 1..12");
    RN_REQUIRE(ctx, head_nhwc && h && w && base_anchors, "head_nhwc, h, w or base_anchors is NULL");
    RN_REQUIRE(ctx, cand, "cand is NULL");
    RN_REQUIRE(ctx, cand->index || cand->logit || cand->box || cand->valid || cand->count, "every output of cand is NULL");
    RN_REQUIRE(ctx, pre_nms_top_n >= 1 && pre_nms_top_n <= kRpnMaxK, "pre_nms_top_n must be 1..4096");
    RN_REQUIRE(ctx, image_h >= 1 && image_w >= 1 && image_h < (1ull << 24) && image_w < (1ull << 24),
               "image_h and image_w must be 1 .. 2^24 - 1");
    RN_REQUIRE(ctx, B <= 65535, "B must be at most 65535");
    RN_REQUIRE(ctx, !(min_size != min_size) && !(logit_thresh != logit_thresh), "min_size or logit_thresh is a NaN");
    const uint64_t P = (5 * A + 3) & ~(uint64_t)3;
    for (uint64_t l = 0; l < L; ++l) {
        RN_REQUIRE(ctx, h[l] >= 1 && w[l] >= 1 && h[l] <= image_h && w[l] <= image_w, "h and w must be 1 .. the image's");
        RN_REQUIRE(ctx, h[l] * w[l] * A < (1ull << 31), "h * w * A must be below 2^31");
    }
    if (B == 0) return RN_OK;
    const uint64_t rows = B * L * pre_nms_top_n;
    operand ops[kRpnMaxLevels + 5];
    int n_ops = 0;
    for (uint64_t l = 0; l < L; ++l) {
        RN_REQUIRE(ctx, head_nhwc[l], "a level's head output is NULL");
        ops[n_ops++] = {head_nhwc[l], B * h[l] * w[l] * P * 4, "a level's head output", false, false};
    }
    ops[n_ops++] = {cand->index, rows * 4, "cand.index", true, false};
    ops[n_ops++] = {cand->logit, rows * 4, "cand.logit", true, false};
    ops[n_ops++] = {cand->box, rows * 16, "cand.box", true, false};
    ops[n_ops++] = {cand->valid, rows, "cand.valid", true, true};
    ops[n_ops++] = {cand->count, B * L * 4, "cand.count", true, false};
    RN_TRY(check_operands(ctx, __func__, ops, n_ops));
    return select_launch(ctx, L, head_nhwc, B, h, w, A, base_anchors, image_h, image_w, pre_nms_top_n, min_size, logit_thresh,
                         cand, "rn_rpn_select_decode_forward");
}

int rn_nms_forward(rn_ctx *ctx, const float *boxes, const uint8_t *valid, uint64_t S, uint64_t n, float iou_threshold,
                   uint8_t *keep, int32_t *keep_count)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, n <= kRpnMaxK, "n must be at most 4096");
    RN_REQUIRE(ctx, S <= 65535, "S must be at most 65535");
    RN_REQUIRE(ctx, !(iou_threshold != iou_threshold), "iou_threshold is a NaN");
    if (S == 0 || n == 0) return RN_OK;
    RN_REQUIRE(ctx, boxes, "boxes is NULL");
    RN_REQUIRE(ctx, keep, "keep is NULL");
    const operand ops[] = {{boxes, S * n * 16, "boxes", false, false},
                           {valid, S * n, "valid", false, true},
                           {keep, S * n, "keep", true, true},
                           {keep_count, S * 4, "keep_count", true, false}};
    RN_TRY(check_operands(ctx, __func__, ops, 4));
    const uint64_t nw = rn_ceil_div(n, 64);
    void *words = nullptr;
    RN_TRY(rn_scratch(ctx, kNmsScratchSlot, S * n * nw * 8, &words));
    RN_TRY(mask_launch(ctx, boxes, nullptr, (uint64_t *)words, S, n, iou_threshold, "rn_nms_forward (mask)"));
    scan_args p;
    memset(&p, 0, sizeof(p));
    p.words = (const uint64_t *)words, p.valid = valid, p.keep = keep, p.keep_count = keep_count;
    p.n = (uint32_t)n, p.nw = (uint32_t)nw;
    nms_scan_kernel<<<(unsigned)S, 64, 0, ctx->stream>>>(p);
    return rn_after_launch(ctx, "rn_nms_forward (scan)");
}

int rn_rpn_nms_merge_forward(rn_ctx *ctx, const rn_rpn_candidates *cand, uint64_t B, uint64_t L, uint64_t pre_nms_top_n,
                             uint64_t post_nms_top_n, float nms_thresh, const rn_rpn_proposals *out)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, L >= 1 && L <= (uint64_t)kRpnMaxLevels, "L must be 1..5");
    RN_REQUIRE(ctx, pre_nms_top_n >= 1 && pre_nms_top_n <= kRpnMaxK, "pre_nms_top_n must be 1..4096");
    RN_REQUIRE(ctx, post_nms_top_n >= 1 && post_nms_top_n <= kRpnMaxK, "post_nms_top_n must be 1..4096");
    RN_REQUIRE(ctx, !(nms_thresh != nms_thresh), "nms_thresh is a NaN");
    RN_REQUIRE(ctx, B <= 65535 / L, "B * L must be at most 65535");
    RN_REQUIRE(ctx, cand, "cand is NULL");
    RN_REQUIRE(ctx, out, "out is NULL");
    RN_REQUIRE(ctx, out->boxes || out->logits || out->levels || out->count || out->rois || out->cand_keep,
               "every output of out is NULL");
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, cand->logit && cand->box && cand->valid && cand->count, "cand.logit, cand.box, cand.valid or cand.count is NULL");
    const uint64_t rows = B * L * pre_nms_top_n, prop = B * post_nms_top_n;
    const operand ops[] = {{cand->logit, rows * 4, "cand.logit", false, false},   {cand->box, rows * 16, "cand.box", false, false},
                           {cand->valid, rows, "cand.valid", false, true},       {cand->count, B * L * 4, "cand.count", false, false},
                           {out->boxes, prop * 16, "out.boxes", true, false},     {out->logits, prop * 4, "out.logits", true, false},
                           {out->levels, prop * 4, "out.levels", true, false},    {out->count, B * 4, "out.count", true, false},
                           {out->rois, prop * 20, "out.rois", true, false},       {out->cand_keep, rows, "out.cand_keep", true, true}};
    RN_TRY(check_operands(ctx, __func__, ops, 10));
    void *words = nullptr;
    RN_TRY(rn_scratch(ctx, kNmsScratchSlot, rows * rn_ceil_div(pre_nms_top_n, 64) * 8, &words));
    RN_TRY(mask_launch(ctx, cand->box, cand->count, (uint64_t *)words, B * L, pre_nms_top_n, nms_thresh,
                       "rn_rpn_nms_merge_forward (mask)"));
    return merge_launch(ctx, (const uint64_t *)words, cand, B, L, pre_nms_top_n, post_nms_top_n, 0, out,
                        "rn_rpn_nms_merge_forward (merge)");
}

// ---- the object: RPNHead's two contractions per level in front of the three launches ---------------------------
// the state dict's six tensors (params): 0 conv weight [C,C,3,3], 1 conv bias [C], 2 cls_logits weight [A,C], 3 its
// bias [A], 4 bbox_pred weight [4A,C], 5 its bias [4A]
struct rn_rpn {
    rn_ctx *ctx;
    uint64_t C, L, A, P;
    int finalized;
    float base[kRpnMaxLevels * kRpnMaxAnchors * 4];
    rn_params params;
    rn_stage_unit conv, pred;  // the 3x3 C -> C; ONE 1x1 C -> P panel: cls_logits, bbox_pred, zero rows (rn_stage_side_by_side)
    // scratch for cap_img images: per level the 3x3's output [.,h,w,C] and the head output [.,h,w,P]; the candidates
    // per (image, level, rank) and the IoU mask
    float *t[kRpnMaxLevels], *head[kRpnMaxLevels];
    float *c_logit, *c_box;
    uint8_t *c_valid;
    int32_t *c_count;
    uint64_t *words;
    uint64_t cap[kRpnMaxLevels + 2];  // images, candidates per (image, level), then the pixels of every level
};
enum { kRpnImg, kRpnPre, kRpnPix, kRpnScratch = 2 * kRpnMaxLevels + 5 };

// the scratch tensors for the capacities `cap`; returns how many
static int rpn_scratch(rn_rpn *r, const uint64_t *cap, rn_scratch_item *list)
{
    int n = 0;
    for (uint64_t l = 0; l < r->L; ++l) {
        list[n++] = {(void **)&r->t[l], cap[kRpnPix + l] * r->C * sizeof(float)};
        list[n++] = {(void **)&r->head[l], cap[kRpnPix + l] * r->P * sizeof(float)};
    }
    const uint64_t rows = cap[kRpnImg] * r->L * cap[kRpnPre];
    list[n++] = {(void **)&r->c_logit, rows * 4};
    list[n++] = {(void **)&r->c_box, rows * 16};
    list[n++] = {(void **)&r->c_valid, rows};
    list[n++] = {(void **)&r->c_count, cap[kRpnImg] * r->L * 4};
    list[n++] = {(void **)&r->words, rows * rn_ceil_div(cap[kRpnPre], 64) * 8};
    return n;
}

int rn_rpn_create(rn_ctx *ctx, rn_rpn **out, uint64_t in_channels, uint64_t L, uint64_t A, const float *base_anchors)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    RN_REQUIRE(ctx, in_channels >= 64 && in_channels % 64 == 0 && in_channels <= 1024,
               "in_channels must be a multiple of 64 (at most 1024)");
    RN_REQUIRE(ctx, L >= 1 && L <= (uint64_t)kRpnMaxLevels, "L must be 1..5");
    RN_REQUIRE(ctx, A >= 1 && A <= (uint64_t)kRpnMaxAnchors, "A must be 1..12");
    RN_REQUIRE(ctx, base_anchors, "base_anchors is NULL");
    for (uint64_t i = 0; i < L * A * 4; ++i) RN_REQUIRE(ctx, isfinite(base_anchors[i]), "a base anchor is not finite");
    rn_rpn *r = (rn_rpn *)calloc(1, sizeof(*r));
    if (!r) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_rpn_create: out of host memory");
    r->ctx = ctx, r->C = in_channels, r->L = L, r->A = A, r->P = (5 * A + 3) & ~(uint64_t)3;
    memcpy(r->base, base_anchors, L * A * 4 * sizeof(float));
    const uint64_t C = in_channels;
    rn_params_add(&r->params, "head.conv.0.0.weight", "head.conv.weight", C, C * 9, C, C * 9, 0.0f);
    rn_params_add(&r->params, "head.conv.0.0.bias", "head.conv.bias", 1, C, 1, C, 0.0f);
    rn_params_add(&r->params, "head.cls_logits.weight", NULL, A, C, A, C, 0.0f);
    rn_params_add(&r->params, "head.cls_logits.bias", NULL, 1, A, 1, A, 0.0f);
    rn_params_add(&r->params, "head.bbox_pred.weight", NULL, 4 * A, C, 4 * A, C, 0.0f);
    rn_params_add(&r->params, "head.bbox_pred.bias", NULL, 1, 4 * A, 1, 4 * A, 0.0f);
    *out = r;
    return RN_OK;
}

int rn_rpn_set_tensor(rn_rpn *r, const char *key, const float *host_data, uint64_t numel)
{
    if (!r) return RN_ERR_INVALID;
    return rn_stage_set_tensor(r->ctx, __func__, "the rpn", r->finalized, &r->params, key, host_data, numel);
}

int rn_rpn_finalize(rn_rpn *r)
{
    if (!r) return RN_ERR_INVALID;
    rn_ctx *ctx = r->ctx;
    RN_ENTER(ctx);
    if (r->finalized) return RN_OK;
    RN_TRY(rn_stage_all_set(ctx, __func__, &r->params));
    const uint64_t C = r->C, A = r->A, P = r->P;
    const rn_params_entry *p = r->params.p;
    float *w = rn_stage_side_by_side(p[2].host, p[3].host, A, p[4].host, p[5].host, 4 * A, C, P);
    if (!w) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_rpn_finalize: out of host memory");
    int st = rn_stage_pack(ctx, RN_DTYPE_F32, p[0].host, C, C, 3, p[1].host, NULL, &r->conv);
    if (st == RN_OK) st = rn_stage_pack(ctx, RN_DTYPE_F32, w, C, P, 1, w + P * C, NULL, &r->pred);
    free(w);
    if (st != RN_OK) return st;
    rn_params_free(&r->params);
    r->finalized = 1;
    return RN_OK;
}

int rn_rpn_destroy(rn_rpn *r)
{
    if (!r) return RN_OK;
    rn_ctx *ctx = r->ctx;
    RN_ENTER(ctx);
    RN_TRY(rn_sync(ctx));
    rn_scratch_item list[kRpnScratch];
    rn_stage_free_list(ctx, list, rpn_scratch(r, r->cap, list));
    rn_params_free(&r->params);
    rn_stage_unit_free(ctx, &r->conv), rn_stage_unit_free(ctx, &r->pred);
    free(r);
    return RN_OK;
}

// ---- library-internal (rn_private.h) ----

int rn_rpn_matches(const rn_rpn *r, const rn_ctx *ctx, uint64_t in_channels, uint64_t n_levels, const char **why)
{
    const char *w = NULL;
    if (!r) w = "the rpn is NULL";
    else if (!r->finalized) w = "the rpn is not finalized";
    else if (r->ctx->device != ctx->device) w = "the rpn's context is on another device";
    else if (r->C != in_channels) w = "the rpn's in_channels is not the neck's out_channels";
    else if (r->L != n_levels) w = "the rpn's level count is not the neck's (its levels and, when it has one, the pool)";
    if (why) *why = w;
    return w == NULL;
}

int rn_rpn_reserve(rn_rpn *r, uint64_t images, const uint64_t *h, const uint64_t *w, uint64_t pre)
{
    uint64_t want[kRpnMaxLevels + 2] = {};
    want[kRpnImg] = images, want[kRpnPre] = pre;
    for (uint64_t l = 0; l < r->L; ++l) want[kRpnPix + l] = images * h[l] * w[l];
    bool fits = true;
    for (int i = 0; i < kRpnMaxLevels + 2; ++i) {
        fits = fits && want[i] <= r->cap[i];
        if (want[i] < r->cap[i]) want[i] = r->cap[i];
    }
    if (fits) return RN_OK;
    rn_scratch_item list[kRpnScratch];
    return rn_stage_grow(r->ctx, "rn_rpn", list, rpn_scratch(r, want, list), r->cap, want, kRpnMaxLevels + 2);
}

// every refusal that concerns the request alone, for `images` images (text in ctx)
int rn_rpn_check(const rn_rpn *r, rn_ctx *ctx, const rn_rpn_request *q, uint64_t images, const uint64_t *h, const uint64_t *w,
                 uint64_t image_h, uint64_t image_w)
{
    RN_REQUIRE(ctx, q, "the rpn's request is NULL");
    RN_REQUIRE(ctx, q->pre_nms_top_n >= 1 && q->pre_nms_top_n <= kRpnMaxK, "pre_nms_top_n must be 1..4096");
    RN_REQUIRE(ctx, q->post_nms_top_n >= 1 && q->post_nms_top_n <= kRpnMaxK, "post_nms_top_n must be 1..4096");
    RN_REQUIRE(ctx, !(q->nms_thresh != q->nms_thresh) && !(q->logit_thresh != q->logit_thresh) && !(q->min_size != q->min_size),
               "nms_thresh, logit_thresh or min_size is a NaN");
    RN_REQUIRE(ctx, image_h >= 1 && image_w >= 1 && image_h < (1ull << 24) && image_w < (1ull << 24),
               "image_h and image_w must be 1 .. 2^24 - 1");
    RN_REQUIRE(ctx, images <= 65535 / r->L, "B * L must be at most 65535");
    for (uint64_t l = 0; l < r->L; ++l) {
        RN_REQUIRE(ctx, h[l] >= 1 && w[l] >= 1 && h[l] <= image_h && w[l] <= image_w, "h and w must be 1 .. the image's");
        RN_REQUIRE(ctx, h[l] * w[l] * r->A < (1ull << 31), "h * w * A must be below 2^31");
    }
    const rn_rpn_proposals *o = &q->out;
    RN_REQUIRE(ctx, o->boxes || o->logits || o->levels || o->count || o->rois || o->cand_keep, "every output of the request is NULL");
    operand ops[RN_RPN_OPERANDS];
    return check_operands(ctx, "rn_rpn request", ops, rn_rpn_operands(r, q, images, ops));
}

int rn_rpn_operands(const rn_rpn *r, const rn_rpn_request *q, uint64_t images, rn_operand ops[RN_RPN_OPERANDS])
{
    const rn_rpn_proposals *o = &q->out;
    const uint64_t rows = images * r->L * q->pre_nms_top_n, prop = images * q->post_nms_top_n;
    const operand all[RN_RPN_OPERANDS] = {
        {o->boxes, prop * 16, "out.boxes", true, false},      {o->logits, prop * 4, "out.logits", true, false},
        {o->levels, prop * 4, "out.levels", true, false},     {o->count, images * 4, "out.count", true, false},
        {o->rois, prop * 20, "out.rois", true, false},        {o->cand_keep, rows, "out.cand_keep", true, true},
        {q->cand.index, rows * 4, "cand.index", true, false}, {q->cand.logit, rows * 4, "cand.logit", true, false},
        {q->cand.box, rows * 16, "cand.box", true, false},    {q->cand.valid, rows, "cand.valid", true, true},
        {q->cand.count, images * r->L * 4, "cand.count", true, false}};
    memcpy(ops, all, sizeof(all));
    return RN_RPN_OPERANDS;
}

// The stage's 2L + 3 launches on ctx for the B images from the caller's image img0 on, whose scratch starts sub0
// images into the object's tensors: per level the 3x3 with ReLU and the 1x1 panel, then select + decode, the IoU mask,
// scan + merge.  x: the L fp32 NHWC levels of these B images.
int rn_rpn_step(rn_rpn *r, rn_ctx *ctx, const float *const *x, uint64_t sub0, uint64_t img0, uint64_t B, const uint64_t *h,
                const uint64_t *w, uint64_t image_h, uint64_t image_w, const rn_rpn_request *q)
{
    const uint64_t L = r->L, C = r->C, P = r->P, pre = q->pre_nms_top_n, post = q->post_nms_top_n;
    if (sub0 + B > r->cap[kRpnImg] || pre > r->cap[kRpnPre]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_rpn: scratch not reserved");
    const float *heads[kRpnMaxLevels];
    rn_epilogue ep;
    ep.scale = NULL, ep.residual = NULL;
    for (uint64_t l = 0; l < L; ++l) {
        if ((sub0 + B) * h[l] * w[l] > r->cap[kRpnPix + l]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_rpn: scratch not reserved");
        float *t = r->t[l] + sub0 * h[l] * w[l] * C, *hd = r->head[l] + sub0 * h[l] * w[l] * P;
        ep.shift = r->conv.shift, ep.relu = 1;
        RN_TRY(rn_conv2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, RN_DTYPE_F32, x[l], t, r->conv.packed, 3, 1, 1, h[l], w[l], B, C, C,
                                         h[l], w[l], &ep));
        ep.shift = r->pred.shift, ep.relu = 0;
        RN_TRY(rn_conv2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, RN_DTYPE_F32, t, hd, r->pred.packed, 1, 1, 0, h[l], w[l], B, C, P,
                                         h[l], w[l], &ep));
        heads[l] = hd;
    }
    // the candidates: the caller's rows of these images where it asked for them, the scratch's otherwise
    const uint64_t urow = img0 * L * pre, srow = sub0 * L * pre;
    rn_rpn_candidates c;
    c.index = q->cand.index ? q->cand.index + urow : NULL;
    c.logit = q->cand.logit ? q->cand.logit + urow : r->c_logit + srow;
    c.box = q->cand.box ? q->cand.box + urow * 4 : r->c_box + srow * 4;
    c.valid = q->cand.valid ? q->cand.valid + urow : r->c_valid + srow;
    c.count = q->cand.count ? q->cand.count + img0 * L : r->c_count + sub0 * L;
    RN_TRY(select_launch(ctx, L, heads, B, h, w, r->A, r->base, image_h, image_w, pre, q->min_size, q->logit_thresh, &c,
                         "rn_rpn (select + decode)"));
    uint64_t *words = r->words + srow * rn_ceil_div(pre, 64);
    RN_TRY(mask_launch(ctx, c.box, c.count, words, B * L, pre, q->nms_thresh, "rn_rpn (mask)"));
    rn_rpn_proposals o;
    const uint64_t orow = img0 * post;
    o.boxes = q->out.boxes ? q->out.boxes + orow * 4 : NULL, o.logits = q->out.logits ? q->out.logits + orow : NULL;
    o.levels = q->out.levels ? q->out.levels + orow : NULL, o.count = q->out.count ? q->out.count + img0 : NULL;
    o.rois = q->out.rois ? q->out.rois + orow * 5 : NULL, o.cand_keep = q->out.cand_keep ? q->out.cand_keep + urow : NULL;
    return merge_launch(ctx, words, &c, B, L, pre, post, img0, &o, "rn_rpn (scan + merge)");
}

int rn_rpn_forward(rn_rpn *r, const float *const *x_nhwc, uint64_t B, const uint64_t *h, const uint64_t *w, uint64_t image_h,
                   uint64_t image_w, const rn_rpn_request *req)
{
    if (!r) return RN_ERR_INVALID;
    rn_ctx *ctx = r->ctx;
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, r->finalized, "the rpn is not finalized");
    RN_REQUIRE(ctx, x_nhwc && h && w, "x_nhwc, h or w is NULL");
    RN_TRY(rn_rpn_check(r, ctx, req, B, h, w, image_h, image_w));
    operand outs[RN_RPN_OPERANDS], maps[kRpnMaxLevels];
    for (uint64_t l = 0; l < r->L; ++l) {
        RN_REQUIRE(ctx, x_nhwc[l], "a level's map is NULL");
        RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(x_nhwc[l]) & 15) == 0, "a level's map is off a 16-byte boundary");
        maps[l] = {x_nhwc[l], B * h[l] * w[l] * r->C * sizeof(float), "a level's map", false, false};
    }
    const rn_operand_group groups[2] = {{maps, (int)r->L}, {outs, rn_rpn_operands(r, req, B, outs)}};
    RN_TRY(check_operand_groups(ctx, __func__, groups, 2));
    if (B == 0) return RN_OK;
    RN_TRY(rn_rpn_reserve(r, B, h, w, req->pre_nms_top_n));
    const int saved_layout = ctx->layout;
    ctx->layout = RN_LAYOUT_NHWC;
    const int st = rn_rpn_step(r, ctx, x_nhwc, 0, 0, B, h, w, image_h, image_w, req);
    ctx->layout = saved_layout;
    return st;
}

}  // extern "C"
