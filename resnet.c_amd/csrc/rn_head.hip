// The classifier head behind the logits: softmax, top-k, and both from one read of the row; plus the
// bf16 -> fp32 widening of the pooled features.  One kernel serves the three entry points, so a
// probability is one expression -- expf(x - max) / sum with one max, one sum order, one division --
// wherever it is written ("The head").
//
// One block of 256 threads (four waves) per row, always: the bits of the sum depend on the block
// size and on nothing else (not on B, the row's place in the batch, the pointer alignment or k).
//   - a row of up to 4096 classes is read from global memory once, into LDS (16 KB); a longer row
//     (up to 65536) is read again from global memory by every pass: it stays in L2;
//   - max and (value, index) winners are exact under any reduction shape; the sum is per thread in
//     index order (i = tid, tid + 256, ...), a xor-shuffle tree inside the wave, then the four wave
//     sums in wave order;
//   - top-k is k rounds of a block arg-max.  The order (v_i > v_j, or v_i == v_j and i < j) is total,
//     so round j simply takes the first element that comes AFTER round j-1's winner: nothing is
//     struck out, nothing is stored per element;
//   - loads and stores are dwords: any 4-byte boundary, the same bits.  No atomics, no scratch.
// The statistics of the softmax (RN_HEAD_SOFTMAX_STATS) and head_prob live in rn_box_dev.h: the box head's class scores
// (rn_detect.hip) are these bits because they are this code.
#include "rn_box_dev.h"
#include "rn_internal.h"
#include "rn_private.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// NaN ranks as -inf (argmax_kernel's rule)
__device__ __forceinline__ float head_rank(float v) { return v != v ? -INFINITY : v; }

// (v, i) precedes (bv, bi)
__device__ __forceinline__ bool head_before(float v, uint32_t i, float bv, uint32_t bi)
{
    return v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(kHeadBlock) void head_kernel(const float *x, float *probs, float *top_val,
                                                          uint64_t *top_idx, uint32_t classes, uint32_t k,
                                                          int soft)
{
    __shared__ float srow[kHeadLdsRow];
    __shared__ float red_v[kHeadWaves];
    __shared__ uint32_t red_i[kHeadWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t b = blockIdx.x;
    const float *row = x + b * classes;
    const bool in_lds = classes <= kHeadLdsRow;

    // pass 1: the row into LDS (short rows) and its maximum
    float mx = -INFINITY;
    for (uint32_t i = tid; i < classes; i += kHeadBlock) {
        const float v = row[i];
        if (in_lds) srow[i] = v;
        mx = fmaxf(mx, v);
    }
    float sum = 0.f;
    if (soft) RN_HEAD_SOFTMAX_STATS(row, classes, in_lds, srow, red_v, tid, lane, wave, mx, sum);
    __syncthreads();  // srow is complete; red_v is free again

    // top-k: round j takes the first element after (pv, pi) in the order
    float pv = INFINITY;
    long long pi = -1;
    for (uint32_t j = 0; j < k; ++j) {
        float bv = -INFINITY;
        uint32_t bi = kNone;
        for (uint32_t i = tid; i < classes; i += kHeadBlock) {
            const float v = head_rank(in_lds ? srow[i] : row[i]);
            const bool after = v < pv || (v == pv && (long long)i > pi);
            if (after && head_before(v, i, bv, bi)) {
                bv = v;
                bi = i;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const uint32_t oi = __shfl_xor(bi, off, 64);
            if (head_before(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            red_v[wave] = bv;
            red_i[wave] = bi;
        }
        __syncthreads();
        bv = red_v[0];
        bi = red_i[0];
        for (int w = 1; w < kHeadWaves; ++w) {
            if (head_before(red_v[w], red_i[w], bv, bi)) {
                bv = red_v[w];
                bi = red_i[w];
            }
        }
        __syncthreads();
        pv = bv;
        pi = bi;
        if (tid == 0) {
            uint32_t win = bi;
            // argmax_kernel's exception, for k = 1 only: a NaN at index 0 is never displaced
            if (k == 1) {
                const float first = in_lds ? srow[0] : row[0];
                if (first != first) win = 0;
            }
            const float xv = in_lds ? srow[win] : row[win];
            top_idx[b * k + j] = win;
            top_val[b * k + j] = soft ? head_prob(xv, mx, sum) : xv;
        }
    }

    // last: the probabilities.  probs may alias x: every element is read (again, for a long row) by
    // the thread that then writes it, and the winners above were read before this barrier.
    if (probs) {
        __syncthreads();
        float *prow = probs + b * classes;
        for (uint32_t i = tid; i < classes; i += kHeadBlock) prow[i] = head_prob(in_lds ? srow[i] : row[i], mx, sum);
    }
}

__global__ __launch_bounds__(256) void widen_bf16_kernel(const uint16_t *src, float *dst, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        dst[i] = __uint_as_float((uint32_t)src[i] << 16);
}

int head_launch(rn_ctx *ctx, const float *x, float *probs, float *top_val, uint64_t *top_idx, uint64_t B,
                uint64_t classes, uint64_t k, int soft, const char *what)
{
    head_kernel<<<(unsigned)B, kHeadBlock, 0, ctx->stream>>>(x, probs, top_val, top_idx, (uint32_t)classes,
                                                             (uint32_t)k, soft);
    return rn_after_launch(ctx, what);
}

inline bool aligned_to(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

}  // namespace

extern "C" {

int rn_softmax_forward(rn_ctx *ctx, const float *logits, float *probs, uint64_t B, uint64_t classes)
{
    RN_ENTER(ctx);
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, logits, "logits is null");
    RN_REQUIRE(ctx, probs, "probs is null");
    RN_REQUIRE(ctx, aligned_to(logits, 3) && aligned_to(probs, 3), "logits / probs off a 4-byte boundary");
    RN_REQUIRE(ctx, classes >= 1 && classes <= 65536, "classes out of range [1, 65536]");
    RN_REQUIRE(ctx, B < (1ull << 31), "B too large");
    return head_launch(ctx, logits, probs, nullptr, nullptr, B, classes, 0, 1, "rn_softmax_forward");
}

int rn_topk_forward(rn_ctx *ctx, const float *x, float *values, uint64_t *indices, uint64_t B, uint64_t classes,
                    uint64_t k)
{
    RN_ENTER(ctx);
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, x, "x is null");
    RN_REQUIRE(ctx, values, "values is null");
    RN_REQUIRE(ctx, indices, "indices is null");
    RN_REQUIRE(ctx, aligned_to(x, 3) && aligned_to(values, 3), "x / values off a 4-byte boundary");
    RN_REQUIRE(ctx, aligned_to(indices, 7), "indices off an 8-byte boundary");
    RN_REQUIRE(ctx, classes >= 1 && classes <= 65536, "classes out of range [1, 65536]");
    RN_REQUIRE(ctx, k >= 1 && k <= 64 && k <= classes, "k out of range [1, min(classes, 64)]");
    RN_REQUIRE(ctx, B < (1ull << 31), "B too large");
    return head_launch(ctx, x, nullptr, values, indices, B, classes, k, 0, "rn_topk_forward");
}

int rn_softmax_topk_forward(rn_ctx *ctx, const float *logits, float *probs, float *topk_prob, uint64_t *topk_idx,
                            uint64_t B, uint64_t classes, uint64_t k)
{
    RN_ENTER(ctx);
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, logits, "logits is null");
    RN_REQUIRE(ctx, topk_prob, "topk_prob is null");
    RN_REQUIRE(ctx, topk_idx, "topk_idx is null");
    RN_REQUIRE(ctx, aligned_to(logits, 3) && aligned_to(probs, 3) && aligned_to(topk_prob, 3),
               "logits / probs / topk_prob off a 4-byte boundary");
    RN_REQUIRE(ctx, aligned_to(topk_idx, 7), "topk_idx off an 8-byte boundary");
    RN_REQUIRE(ctx, classes >= 1 && classes <= 65536, "classes out of range [1, 65536]");
    RN_REQUIRE(ctx, k >= 1 && k <= 64 && k <= classes, "k out of range [1, min(classes, 64)]");
    RN_REQUIRE(ctx, B < (1ull << 31), "B too large");
    return head_launch(ctx, logits, probs, topk_prob, topk_idx, B, classes, k, 1, "rn_softmax_topk_forward");
}

// library-internal (rn_private.h): bf16 values as fp32, exact; src on a 2-byte, dst on a 4-byte boundary
int rn_widen_bf16_forward(rn_ctx *ctx, const void *src_bf16, float *dst, uint64_t n)
{
    RN_ENTER(ctx);
    if (n == 0) return RN_OK;
    RN_REQUIRE(ctx, src_bf16 && dst, "null tensor");
    widen_bf16_kernel<<<rn_stream_grid(n, 256), 256, 0, ctx->stream>>>((const uint16_t *)src_bf16, dst, n);
    return rn_after_launch(ctx, "rn_widen_bf16_forward");
}

}  // extern "C"
