// The box head of a two-stage detector behind the pooler: torchvision's TwoMLPHead and FastRCNNPredictor as three
// contractions, then RoIHeads.postprocess_detections (softmax, per-class decode, clip, score threshold, small-box
// removal, per-class NMS, the best detections_per_img) as THREE launches whatever B, R and C:
//   score + decode (detect_score_kernel): one block of 256 threads per RoI row -- the block shape of
//     rn_softmax_forward, whose statistics it shares (rn_box_dev.h), so a probability is the same bits -- writes the
//     row's probabilities, its C - 1 decoded boxes, their validity and, per (image, class), a 32-bit order word per
//     RoI (0: not a candidate);
//   per-class sort + NMS (detect_class_nms_kernel): one block per (image, class).  It gathers the class's nonzero
//     words into LDS -- a class without a candidate ends there, before any sort -- sorts them with the RPN's bitonic
//     network and suppresses in chunks of 64 candidates: the wave that owns a chunk resolves it in registers, then
//     every later candidate is tested against the chunk's survivors, which lie in LDS.  One barrier per chunk; no
//     IoU mask exists anywhere.  The survivors' 64-bit merge keys leave in order, with their count;
//   merge (detect_merge_kernel): one block per image, the RPN's exact selection on the unique keys (score, f) of the
//     image's survivors, addressed through a prefix sum of the class counts.
// Scratch is O(B * C * R): 12 bytes per (RoI, class) of order words and keys, the class boxes where the caller does
// not ask for them, a count per (image, class).  Atomics: integer adds in LDS only.  The reference classifies whole
// images only; nothing here has a counterpart in it.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "rn_box_dev.h"
#include "rn_conv_params.h"
#include "rn_internal.h"
#include "rn_private.h"

// The arithmetic of the decode, the validity rule and the IoU is a contract, operation by operation (rn_hip.h): no
// product of this file is fused into an add.
#pragma clang fp contract(off)

namespace {

constexpr uint32_t kDetMaxC = 1024;                    // classes, background included: a row of logits in LDS
constexpr uint32_t kDetMaxD = 1024;                    // detections per image
constexpr int kDetSlots = kRpnMaxK / kRpnBlock;        // sorted candidates a thread of the class block holds
constexpr int kDetScratchSlot = 6;                     // the context's scratch slot the RPN's mask also uses

// ---- score + decode ---------------------------------------------------------------------------------------------
struct score_args {
    const float *head;  // [K, P]
    const float *rois;  // [K, 5]
    uint32_t R, C, P, mul_r, shr_r;
    uint32_t img0;      // the image index of this launch's first image (the RoI rows' first column)
    decode_consts dc;
    float score_thresh, min_size;
    float *probs;       // [K, C] or NULL
    float *boxes;       // [K, C, 4]: the caller's or the scratch's
    uint8_t *valid, *keep;  // [K, C] or NULL; keep is cleared here, the class blocks set the survivors
    uint32_t *skey;     // [B, C - 1, R]
};

__global__ __launch_bounds__(kHeadBlock) void detect_score_kernel(const score_args p)
{
    __shared__ float srow[kDetMaxC];
    __shared__ float red_v[kHeadWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t k = blockIdx.x, classes = p.C;
    const float *row = p.head + (uint64_t)k * p.P;
    const bool in_lds = true;
    float mx = -INFINITY;
    for (uint32_t i = tid; i < classes; i += kHeadBlock) {
        const float v = row[i];
        srow[i] = v;
        mx = fmaxf(mx, v);
    }
    float sum = 0.f;
    RN_HEAD_SOFTMAX_STATS(row, classes, in_lds, srow, red_v, tid, lane, wave, mx, sum);
    const uint32_t b = rn_gemm::fast_div(k, (int)p.R, p.mul_r, p.shr_r), r = k - b * p.R;
    const float *roi = p.rois + (uint64_t)k * 5;
    const float a[4] = {roi[1], roi[2], roi[3], roi[4]};
    const bool real = roi[0] == (float)(p.img0 + b);
    for (uint32_t c = tid; c < classes; c += kHeadBlock) {
        const float prob = head_prob(srow[c], mx, sum);
        float box[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool valid = false;
        if (c >= 1) {
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = row[classes + 4 * c + j];
            rpn_decode(a, d, p.dc, box);
            valid = real && (prob > p.score_thresh) && (box[2] - box[0] >= p.min_size) && (box[3] - box[1] >= p.min_size);
            p.skey[((uint64_t)b * (classes - 1) + (c - 1)) * p.R + r] = valid ? rpn_mono(prob) : 0u;
        }
        const uint64_t o = (uint64_t)k * classes + c;
        if (p.probs) p.probs[o] = prob;
        if (p.valid) p.valid[o] = valid ? 1 : 0;
        if (p.keep) p.keep[o] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) p.boxes[o * 4 + j] = box[j];
    }
}

// ---- per-class sort + NMS ---------------------------------------------------------------------------------------
struct class_args {
    const uint32_t *skey;  // [B, C - 1, R]
    const float *boxes;    // [K, C, 4]
    uint64_t *okeys;       // [B, C - 1, R]: a class's survivors in order, (order word, ~f)
    int32_t *ocount;       // [B, C - 1]
    uint8_t *keep;         // [K, C] or NULL
    uint32_t R, C;
    float thresh;
};

__global__ __launch_bounds__(kRpnBlock) void detect_class_nms_kernel(const class_args p)
{
    __shared__ sel_smem s;
    __shared__ float cb[2][64][4];
    __shared__ uint64_t cmask[2];
    const uint32_t c1 = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t C1 = p.C - 1;
    const uint64_t seg = (uint64_t)b * C1 + c1;
    const uint32_t *skey = p.skey + seg * p.R;
    if (tid == 0) s.fill = 0;
    __syncthreads();
    for (uint32_t r = tid; r < p.R; r += kRpnBlock) {
        const uint32_t u = skey[r];
        if (u) s.keys[atomicAdd(&s.fill, 1u)] = ((uint64_t)u << 32) | (uint32_t)~r;  // at most R <= kRpnMaxK
    }
    __syncthreads();
    const uint32_t n = s.fill;
    if (n == 0) {  // uniform: the common case
        if (tid == 0) p.ocount[seg] = 0;
        return;
    }
    rpn_sort_desc(s.keys, n);
    // thread tid holds the sorted candidates tid, tid + 1024, ...: a chunk of 64 is one wave's one slot
    float bx[kDetSlots][4];
    bool dead[kDetSlots];
#pragma unroll
    for (int t = 0; t < kDetSlots; ++t) {
        const uint32_t j = tid + (uint32_t)t * kRpnBlock;
        dead[t] = j >= n;
#pragma unroll
        for (int q = 0; q < 4; ++q) bx[t][q] = 0.0f;
        if (!dead[t]) {
            const uint32_t r = ~(uint32_t)s.keys[j];
            const float *src = p.boxes + (((uint64_t)b * p.R + r) * p.C + c1 + 1) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) bx[t][q] = src[q];
        }
    }
    uint32_t kept = 0;
    for (uint32_t c0 = 0, it = 0; c0 < n; c0 += 64, ++it) {
        const uint32_t buf = it & 1, own_wave = (c0 >> 6) & (kRpnBlock / 64 - 1), own_slot = c0 >> 10;
        if (wave == own_wave) {
            float x1 = 0.0f, y1 = 0.0f, x2 = 0.0f, y2 = 0.0f;
            bool gone = true;
#pragma unroll
            for (int t = 0; t < kDetSlots; ++t)
                if ((uint32_t)t == own_slot) x1 = bx[t][0], y1 = bx[t][1], x2 = bx[t][2], y2 = bx[t][3], gone = dead[t];
            uint64_t alive = __ballot(!gone);
#pragma unroll 1
            for (uint32_t q = 0; q < 64; ++q) {
                if (!((alive >> q) & 1ull)) continue;  // uniform in the wave
                const float u1 = __shfl(x1, (int)q, 64), v1 = __shfl(y1, (int)q, 64), u2 = __shfl(x2, (int)q, 64),
                            v2 = __shfl(y2, (int)q, 64);
                const float iou = rpn_iou(u1, v1, u2, v2, (u2 - u1) * (v2 - v1), x1, y1, x2, y2);
                alive &= ~__ballot(lane > q && iou > p.thresh);
            }
            cb[buf][lane][0] = x1, cb[buf][lane][1] = y1, cb[buf][lane][2] = x2, cb[buf][lane][3] = y2;
            if (lane == 0) cmask[buf] = alive;
            if ((alive >> lane) & 1ull) {
                const uint64_t key = s.keys[c0 + lane];
                const uint32_t r = ~(uint32_t)key, rank = kept + (uint32_t)__popcll(alive & ((1ull << lane) - 1ull));
                p.okeys[seg * p.R + rank] = (key & 0xFFFFFFFF00000000ull) | (uint32_t)~(r * C1 + c1);
                if (p.keep) p.keep[((uint64_t)b * p.R + r) * p.C + c1 + 1] = 1;
            }
        }
        __syncthreads();
        const uint64_t m = cmask[buf];
#pragma unroll
        for (int t = 0; t < kDetSlots; ++t) {
            const uint32_t j = tid + (uint32_t)t * kRpnBlock;
            if (dead[t] || j < c0 + 64) continue;
            uint64_t mm = m;
            while (mm) {
                const int q = __ffsll((unsigned long long)mm) - 1;
                mm &= mm - 1;
                const float u1 = cb[buf][q][0], v1 = cb[buf][q][1], u2 = cb[buf][q][2], v2 = cb[buf][q][3];
                const float iou = rpn_iou(u1, v1, u2, v2, (u2 - u1) * (v2 - v1), bx[t][0], bx[t][1], bx[t][2], bx[t][3]);
                if (iou > p.thresh) {
                    dead[t] = true;
                    break;
                }
            }
        }
        kept += (uint32_t)__popcll(m);
    }
    if (tid == 0) p.ocount[seg] = (int32_t)kept;
}

// ---- merge: one block per image ---------------------------------------------------------------------------------
struct dmerge_args {
    const uint64_t *okeys;
    const int32_t *ocount;
    const float *cboxes;  // [K, C, 4]
    uint32_t R, C, D, mul_c1, shr_c1;
    float *boxes, *scores;
    int32_t *labels, *roi, *count;
};

__global__ __launch_bounds__(kRpnBlock) void detect_merge_kernel(const dmerge_args p)
{
    __shared__ sel_smem s;
    __shared__ uint32_t soff[kRpnBlock];  // survivors of the classes in front of class tid
    __shared__ uint32_t wsum[kRpnBlock / 64];
    __shared__ uint32_t stotal;
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t C1 = p.C - 1;
    const uint32_t mine = tid < C1 ? (uint32_t)p.ocount[(uint64_t)b * C1 + tid] : 0u;
    uint32_t incl = mine;
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t front = 0;
    for (uint32_t w = 0; w < wave; ++w) front += wsum[w];
    soff[tid] = front + incl - mine;
    if (tid == kRpnBlock - 1) stotal = front + incl;
    __syncthreads();
    const uint32_t T = stotal, want = T < p.D ? T : p.D;
    const uint64_t *okeys = p.okeys + (uint64_t)b * C1 * p.R;
    const uint32_t R = p.R;
    if (want > 0) {  // uniform
        rpn_select_sort(s, T, want, [=](uint32_t i) -> uint64_t {
            uint32_t lo = 0, hi = C1;  // the last class whose offset is at most i holds survivor i
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (soff[mid] <= i) lo = mid;
                else hi = mid;
            }
            return okeys[(uint64_t)lo * R + (i - soff[lo])];
        });
    }
    for (uint32_t d = tid; d < p.D; d += kRpnBlock) {
        float box[4] = {0.0f, 0.0f, 0.0f, 0.0f}, score = 0.0f;
        int32_t label = -1, roi = -1;
        if (d < want) {
            const uint64_t key = s.keys[d];
            const uint32_t f = ~(uint32_t)key, r = rn_gemm::fast_div(f, (int)C1, p.mul_c1, p.shr_c1), c = f - r * C1 + 1;
            score = rpn_unmono((uint32_t)(key >> 32));
            label = (int32_t)c, roi = (int32_t)r;
            const float *src = p.cboxes + (((uint64_t)b * R + r) * p.C + c) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) box[q] = src[q];
        }
        const uint64_t o = (uint64_t)b * p.D + d;
        if (p.scores) p.scores[o] = score;
        if (p.labels) p.labels[o] = label;
        if (p.roi) p.roi[o] = roi;
        if (p.boxes) {
#pragma unroll
            for (int q = 0; q < 4; ++q) p.boxes[o * 4 + q] = box[q];
        }
    }
    if (tid == 0 && p.count) p.count[b] = (int32_t)want;
}

// ---- host side --------------------------------------------------------------------------------------------------
uint64_t head_pitch(uint64_t C) { return (5 * C + 3) & ~(uint64_t)3; }

// the stage's scratch for `images` images of R RoIs and C classes, carved from one block (okeys first: 8-byte words)
struct det_scratch {
    uint64_t *okeys;
    float *cboxes;
    uint32_t *skey;
    int32_t *ocount;
};

uint64_t det_scratch_bytes(uint64_t images, uint64_t R, uint64_t C)
{
    return images * ((C - 1) * R * 12 + R * C * 16 + (C - 1) * 4);
}

// the slice of `images` images that starts sub0 images into a block laid out for cap images
det_scratch det_carve(void *base, uint64_t cap, uint64_t sub0, uint64_t R, uint64_t C)
{
    char *at = (char *)base;
    det_scratch d;
    d.okeys = (uint64_t *)at + sub0 * (C - 1) * R, at += cap * (C - 1) * R * 8;
    d.cboxes = (float *)at + sub0 * R * C * 4, at += cap * R * C * 16;
    d.skey = (uint32_t *)at + sub0 * (C - 1) * R, at += cap * (C - 1) * R * 4;
    d.ocount = (int32_t *)at + sub0 * (C - 1);
    return d;
}

constexpr int kDetOutputs = 9;

// the request's outputs for `images` images as operands
void det_outputs(const rn_detections *o, uint64_t images, uint64_t R, uint64_t C, uint64_t D, operand *ops)
{
    const uint64_t K = images * R, rows = images * D;
    ops[0] = {o->boxes, rows * 16, "out.boxes", true, false};
    ops[1] = {o->scores, rows * 4, "out.scores", true, false};
    ops[2] = {o->labels, rows * 4, "out.labels", true, false};
    ops[3] = {o->roi, rows * 4, "out.roi", true, false};
    ops[4] = {o->count, images * 4, "out.count", true, false};
    ops[5] = {o->probs, K * C * 4, "out.probs", true, false};
    ops[6] = {o->class_boxes, K * C * 16, "out.class_boxes", true, false};
    ops[7] = {o->valid, K * C, "out.valid", true, true};
    ops[8] = {o->keep, K * C, "out.keep", true, true};
}

// every refusal that concerns the request and the shapes alone
int det_check(rn_ctx *ctx, const char *fn, const rn_detect_request *q, uint64_t B, uint64_t R, uint64_t C, uint64_t image_h,
              uint64_t image_w)
{
    if (!q) return rn_set_error(ctx, RN_ERR_INVALID, "%s: the request is NULL", fn);
    const char *why = NULL;
    if (R < 1 || R > kRpnMaxK) why = "R must be 1..4096";
    else if (C < 2 || C > kDetMaxC) why = "C must be 2..1024";
    else if (q->detections_per_img < 1 || q->detections_per_img > kDetMaxD) why = "detections_per_img must be 1..1024";
    else if (q->score_thresh != q->score_thresh || q->nms_thresh != q->nms_thresh || q->min_size != q->min_size)
        why = "score_thresh, nms_thresh or min_size is a NaN";
    else if (image_h < 1 || image_w < 1 || image_h >= (1ull << 24) || image_w >= (1ull << 24))
        why = "image_h and image_w must be 1 .. 2^24 - 1";
    else if (B > 65535) why = "B must be at most 65535";
    else if (B * R >= (1ull << 31)) why = "B * R must be below 2^31";
    else if (!q->out.boxes && !q->out.scores && !q->out.labels && !q->out.roi && !q->out.count)
        why = "every output of the request's detections is NULL";
    for (int i = 0; i < 4 && !why; ++i)
        if (!(q->weights[i] > 0.0f) || !isfinite(q->weights[i])) why = "the weights must be positive and finite";
    if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
    return RN_OK;
}

// the three launches, no checks: head [B*R, P] and rois [B*R, 5] of the B images from the caller's image img0 on;
// `out` already points at these images' rows
int det_launch(rn_ctx *ctx, const float *head, const float *rois, uint64_t B, uint64_t R, uint64_t C, uint64_t img0,
               uint64_t image_h, uint64_t image_w, const rn_detect_request *q, const rn_detections *out,
               const det_scratch &sc, const char *what)
{
    char name[96];
    float *cboxes = out->class_boxes ? out->class_boxes : sc.cboxes;
    score_args a;
    memset(&a, 0, sizeof(a));
    a.head = head, a.rois = rois, a.R = (uint32_t)R, a.C = (uint32_t)C, a.P = (uint32_t)head_pitch(C), a.img0 = (uint32_t)img0;
    rn_fast_div((unsigned)R, &a.mul_r, &a.shr_r);
    a.dc = {q->weights[0], q->weights[1], q->weights[2], q->weights[3], (float)log(1000.0 / 16.0), (float)image_w, (float)image_h};
    a.score_thresh = q->score_thresh, a.min_size = q->min_size;
    a.probs = out->probs, a.boxes = cboxes, a.valid = out->valid, a.keep = out->keep, a.skey = sc.skey;
    detect_score_kernel<<<(unsigned)(B * R), kHeadBlock, 0, ctx->stream>>>(a);
    snprintf(name, sizeof(name), "%s (score + decode)", what);
    RN_TRY(rn_after_launch(ctx, name));
    class_args c;
    memset(&c, 0, sizeof(c));
    c.skey = sc.skey, c.boxes = cboxes, c.okeys = sc.okeys, c.ocount = sc.ocount, c.keep = out->keep;
    c.R = (uint32_t)R, c.C = (uint32_t)C, c.thresh = q->nms_thresh;
    detect_class_nms_kernel<<<dim3((unsigned)(C - 1), (unsigned)B), kRpnBlock, 0, ctx->stream>>>(c);
    snprintf(name, sizeof(name), "%s (class sort + NMS)", what);
    RN_TRY(rn_after_launch(ctx, name));
    dmerge_args m;
    memset(&m, 0, sizeof(m));
    m.okeys = sc.okeys, m.ocount = sc.ocount, m.cboxes = cboxes;
    m.R = (uint32_t)R, m.C = (uint32_t)C, m.D = (uint32_t)q->detections_per_img;
    rn_fast_div((unsigned)(C - 1), &m.mul_c1, &m.shr_c1);
    m.boxes = out->boxes, m.scores = out->scores, m.labels = out->labels, m.roi = out->roi, m.count = out->count;
    detect_merge_kernel<<<(unsigned)B, kRpnBlock, 0, ctx->stream>>>(m);
    snprintf(name, sizeof(name), "%s (merge)", what);
    return rn_after_launch(ctx, name);
}

// the rows of the images from img0 on of a request's outputs
rn_detections det_rows(const rn_detections *o, uint64_t img0, uint64_t R, uint64_t C, uint64_t D)
{
    const uint64_t k0 = img0 * R, d0 = img0 * D;
    rn_detections r;
    r.boxes = o->boxes ? o->boxes + d0 * 4 : NULL, r.scores = o->scores ? o->scores + d0 : NULL;
    r.labels = o->labels ? o->labels + d0 : NULL, r.roi = o->roi ? o->roi + d0 : NULL, r.count = o->count ? o->count + img0 : NULL;
    r.probs = o->probs ? o->probs + k0 * C : NULL, r.class_boxes = o->class_boxes ? o->class_boxes + k0 * C * 4 : NULL;
    r.valid = o->valid ? o->valid + k0 * C : NULL, r.keep = o->keep ? o->keep + k0 * C : NULL;
    return r;
}

}  // namespace

extern "C" {

int rn_detect_postprocess_forward(rn_ctx *ctx, const float *head, const float *rois, uint64_t B, uint64_t R, uint64_t C,
                                  uint64_t image_h, uint64_t image_w, const rn_detect_request *req)
{
    RN_ENTER(ctx);
    RN_TRY(det_check(ctx, __func__, req, B, R, C, image_h, image_w));
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, head, "head is NULL");
    RN_REQUIRE(ctx, rois, "rois is NULL");
    operand ops[kDetOutputs + 2];
    ops[0] = {head, B * R * head_pitch(C) * 4, "head", false, false};
    ops[1] = {rois, B * R * 20, "rois", false, false};
    det_outputs(&req->out, B, R, C, req->detections_per_img, ops + 2);
    RN_TRY(check_operands(ctx, __func__, ops, kDetOutputs + 2));
    void *base = nullptr;
    RN_TRY(rn_scratch(ctx, kDetScratchSlot, det_scratch_bytes(B, R, C), &base));
    return det_launch(ctx, head, rois, B, R, C, 0, image_h, image_w, req, &req->out, det_carve(base, B, 0, R, C),
                      "rn_detect_postprocess_forward");
}

// ---- the object: TwoMLPHead and FastRCNNPredictor in front of the three launches --------------------------------
struct rn_box_head {
    rn_ctx *ctx;
    uint64_t F, M, C, P;  // in_features, representation, classes, the head output's pitch
    int finalized;
    rn_params params;       // the state dict's eight tensors: fc6, fc7, cls_score, bbox_pred, weight then bias
    rn_stage_unit unit[3];  // fc6 F -> M, fc7 M -> M, ONE panel M -> P: cls_score, bbox_pred, zero rows
    // scratch for cap[0] images of cap[1] RoIs: fc6's and fc7's outputs [., M], the head output [., P], the stage's
    float *t6, *t7, *head;
    void *det;
    uint64_t cap[2];
};
enum { kBoxImg, kBoxR, kBoxScratch = 4 };

// the scratch tensors for `img` images of `R` RoIs; returns how many
static int box_head_scratch(rn_box_head *h, uint64_t img, uint64_t R, rn_scratch_item *list)
{
    list[0] = {(void **)&h->t6, img * R * h->M * sizeof(float)};
    list[1] = {(void **)&h->t7, img * R * h->M * sizeof(float)};
    list[2] = {(void **)&h->head, img * R * h->P * sizeof(float)};
    list[3] = {&h->det, det_scratch_bytes(img, R, h->C)};
    return kBoxScratch;
}

int rn_box_head_create(rn_ctx *ctx, rn_box_head **out, uint64_t in_features, uint64_t representation, uint64_t classes)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    RN_REQUIRE(ctx, in_features >= 64 && in_features % 64 == 0 && in_features <= (1ull << 20),
               "in_features must be a multiple of 64 (at most 2^20)");
    RN_REQUIRE(ctx, representation >= 64 && representation % 64 == 0 && representation <= 16384,
               "representation must be a multiple of 64 (at most 16384)");
    RN_REQUIRE(ctx, classes >= 2 && classes <= kDetMaxC, "classes must be 2..1024");
    rn_box_head *h = (rn_box_head *)calloc(1, sizeof(*h));
    if (!h) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_box_head_create: out of host memory");
    h->ctx = ctx, h->F = in_features, h->M = representation, h->C = classes, h->P = head_pitch(classes);
    static const char *const layer[4] = {"box_head.fc6", "box_head.fc7", "box_predictor.cls_score", "box_predictor.bbox_pred"};
    const uint64_t rows[4] = {h->M, h->M, h->C, 4 * h->C};
    for (int i = 0; i < 4; ++i) {
        char key[RN_PARAM_KEY];
        const uint64_t len = i == 0 ? h->F : h->M;
        snprintf(key, sizeof(key), "%s.weight", layer[i]);
        rn_params_add(&h->params, key, NULL, rows[i], len, rows[i], len, 0.0f);
        snprintf(key, sizeof(key), "%s.bias", layer[i]);
        rn_params_add(&h->params, key, NULL, 1, rows[i], 1, rows[i], 0.0f);
    }
    *out = h;
    return RN_OK;
}

int rn_box_head_set_tensor(rn_box_head *h, const char *key, const float *host_data, uint64_t numel)
{
    if (!h) return RN_ERR_INVALID;
    return rn_stage_set_tensor(h->ctx, __func__, "the box head", h->finalized, &h->params, key, host_data, numel);
}

int rn_box_head_finalize(rn_box_head *h)
{
    if (!h) return RN_ERR_INVALID;
    rn_ctx *ctx = h->ctx;
    RN_ENTER(ctx);
    if (h->finalized) return RN_OK;
    RN_TRY(rn_stage_all_set(ctx, __func__, &h->params));
    const uint64_t M = h->M, C = h->C, P = h->P;
    const rn_params_entry *p = h->params.p;
    float *w = rn_stage_side_by_side(p[4].host, p[5].host, C, p[6].host, p[7].host, 4 * C, M, P);
    if (!w) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_box_head_finalize: out of host memory");
    int st = rn_stage_pack(ctx, RN_DTYPE_F32, p[0].host, h->F, M, 1, p[1].host, NULL, &h->unit[0]);
    if (st == RN_OK) st = rn_stage_pack(ctx, RN_DTYPE_F32, p[2].host, M, M, 1, p[3].host, NULL, &h->unit[1]);
    if (st == RN_OK) st = rn_stage_pack(ctx, RN_DTYPE_F32, w, M, P, 1, w + P * M, NULL, &h->unit[2]);
    free(w);
    if (st != RN_OK) return st;
    rn_params_free(&h->params);
    h->finalized = 1;
    return RN_OK;
}

int rn_box_head_destroy(rn_box_head *h)
{
    if (!h) return RN_OK;
    rn_ctx *ctx = h->ctx;
    RN_ENTER(ctx);
    RN_TRY(rn_sync(ctx));
    rn_scratch_item list[kBoxScratch];
    rn_stage_free_list(ctx, list, box_head_scratch(h, 0, 0, list));
    rn_params_free(&h->params);
    for (int i = 0; i < 3; ++i) rn_stage_unit_free(ctx, &h->unit[i]);
    free(h);
    return RN_OK;
}

// ---- library-internal (rn_private.h) ----

int rn_box_head_matches(const rn_box_head *h, const rn_ctx *ctx, uint64_t in_features, const char **why)
{
    const char *w = NULL;
    if (!h) w = "the box head is NULL";
    else if (!h->finalized) w = "the box head is not finalized";
    else if (h->ctx->device != ctx->device) w = "the box head's context is on another device";
    else if (h->F != in_features) w = "the box head's in_features is not the pooler's a * PH * PW";
    if (why) *why = w;
    return w == NULL;
}

int rn_box_head_reserve(rn_box_head *h, uint64_t images, uint64_t R)
{
    if (images <= h->cap[kBoxImg] && R <= h->cap[kBoxR]) return RN_OK;
    const uint64_t want[2] = {images > h->cap[kBoxImg] ? images : h->cap[kBoxImg], R > h->cap[kBoxR] ? R : h->cap[kBoxR]};
    rn_scratch_item list[kBoxScratch];
    return rn_stage_grow(h->ctx, "rn_box_head", list, box_head_scratch(h, want[kBoxImg], want[kBoxR], list), h->cap, want, 2);
}

// every refusal that concerns the request alone, for a forward of `images` images of R RoIs (text in ctx)
int rn_box_head_check(const rn_box_head *h, rn_ctx *ctx, const rn_detect_request *q, uint64_t images, uint64_t R,
                      uint64_t image_h, uint64_t image_w)
{
    RN_TRY(det_check(ctx, "rn_box_head request", q, images, R, h->C, image_h, image_w));
    operand ops[kDetOutputs];
    det_outputs(&q->out, images, R, h->C, q->detections_per_img, ops);
    return check_operands(ctx, "rn_box_head request", ops, kDetOutputs);
}

int rn_box_head_operands(const rn_box_head *h, const rn_detect_request *q, uint64_t images, uint64_t R,
                         rn_operand ops[RN_BOX_HEAD_OPERANDS])
{
    static_assert(RN_BOX_HEAD_OPERANDS == kDetOutputs, "the box head's operands are its request's outputs");
    det_outputs(&q->out, images, R, h->C, q->detections_per_img, ops);
    return kDetOutputs;
}

// The stage's launches (6 to 9: a contraction is one launch, or two where its plan finishes a chunked K sum in a second
// pass) on ctx for the B images from the caller's image img0 on, whose scratch starts sub0 images
// into the object's tensors: fc6 and fc7 with ReLU, the predictor's panel, then the three of the post-processing.
// pooled [B*R, F] and rois [B*R, 5]: the rows of these B images.
int rn_box_head_step(rn_box_head *h, rn_ctx *ctx, const float *pooled, const float *rois, uint64_t sub0, uint64_t img0,
                     uint64_t B, uint64_t R, uint64_t image_h, uint64_t image_w, const rn_detect_request *q)
{
    if (sub0 + B > h->cap[kBoxImg] || R > h->cap[kBoxR]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_box_head: scratch not reserved");
    const uint64_t K = B * R, row0 = sub0 * R;
    float *t6 = h->t6 + row0 * h->M, *t7 = h->t7 + row0 * h->M, *head = h->head + row0 * h->P;
    rn_epilogue ep;
    ep.scale = NULL, ep.residual = NULL;
    ep.shift = h->unit[0].shift, ep.relu = 1;
    RN_TRY(rn_conv2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, RN_DTYPE_F32, pooled, t6, h->unit[0].packed, 1, 1, 0, 1, 1, K, h->F, h->M, 1, 1, &ep));
    ep.shift = h->unit[1].shift;
    RN_TRY(rn_conv2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, RN_DTYPE_F32, t6, t7, h->unit[1].packed, 1, 1, 0, 1, 1, K, h->M, h->M, 1, 1, &ep));
    ep.shift = h->unit[2].shift, ep.relu = 0;
    RN_TRY(rn_conv2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, RN_DTYPE_F32, t7, head, h->unit[2].packed, 1, 1, 0, 1, 1, K, h->M, h->P, 1, 1, &ep));
    const rn_detections out = det_rows(&q->out, img0, R, h->C, q->detections_per_img);
    return det_launch(ctx, head, rois, B, R, h->C, img0, image_h, image_w, q, &out, det_carve(h->det, h->cap[kBoxImg], sub0, h->cap[kBoxR], h->C),
                      "rn_box_head");
}

int rn_box_head_forward(rn_box_head *h, const float *pooled, const float *rois, uint64_t B, uint64_t R, uint64_t image_h,
                        uint64_t image_w, const rn_detect_request *req, float *head_out)
{
    if (!h) return RN_ERR_INVALID;
    rn_ctx *ctx = h->ctx;
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, h->finalized, "the box head is not finalized");
    RN_TRY(rn_box_head_check(h, ctx, req, B, R, image_h, image_w));
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, pooled, "pooled is NULL");
    RN_REQUIRE(ctx, rois, "rois is NULL");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(pooled) & 15) == 0, "pooled is off a 16-byte boundary");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(rois) & 3) == 0, "rois is off a 4-byte boundary");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(head_out) & 3) == 0, "head_out is off a 4-byte boundary");
    const uint64_t K = B * R;
    operand outs[kDetOutputs];
    const operand own[3] = {{head_out, K * h->P * sizeof(float), "head_out", true, false},
                            {pooled, K * h->F * sizeof(float), "pooled", false, false},
                            {rois, K * 20, "rois", false, false}};
    rn_box_head_operands(h, req, B, R, outs);
    const rn_operand_group groups[2] = {{own, 3}, {outs, kDetOutputs}};
    RN_TRY(check_operand_groups(ctx, __func__, groups, 2));
    RN_TRY(check_operands(ctx, __func__, own, 3));  // head_out against pooled and rois
    RN_TRY(rn_box_head_reserve(h, B, R));
    const int saved_layout = ctx->layout;
    ctx->layout = RN_LAYOUT_NHWC;
    int st = rn_box_head_step(h, ctx, pooled, rois, 0, 0, B, R, image_h, image_w, req);
    ctx->layout = saved_layout;
    if (st == RN_OK && head_out) st = rn_memcpy_d2d(ctx, head_out, h->head, K * h->P * sizeof(float));
    return st;
}

}  // extern "C"
