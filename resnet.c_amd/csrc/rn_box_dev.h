// Device code that more than one translation unit states: the softmax statistics of a row (rn_head.hip; the box
// head's class scores in rn_detect.hip are the same bits because they are this code), and the order, the selection,
// the sort, the decode and the IoU of the detector's launches (rn_rpn.hip, rn_detect.hip).  Everything sits in the
// unnamed namespace of the file that includes it, as it did when each file held its own copy.
#ifndef RN_BOX_DEV_H
#define RN_BOX_DEV_H

#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace {

// ---- the classifier head's softmax: one block of kHeadBlock threads per row (rn_head.hip's header) --------------
constexpr int kHeadBlock = 256;
constexpr int kHeadWaves = kHeadBlock / 64;
constexpr uint32_t kHeadLdsRow = 4096;

// the one expression of a probability
__device__ __forceinline__ float head_prob(float x, float mx, float sum) { return expf(x - mx) / sum; }

// Block-wide, from every thread's own maximum in mx: mx becomes the row's maximum and sum (0 on entry) the sum of
// expf(x - mx) in the one order: per thread in index order (i = tid, tid + 256, ...), a xor-shuffle tree inside the
// wave, then the wave sums in wave order.  red_v (kHeadWaves floats of LDS) is free again after the caller's next
// barrier.  A macro, not a function: inlined as a function the same statements reach head_kernel as the same 562
// instructions in another order, and that kernel's emitted code is held fixed (profiles/detect/isa_parent_against_this.txt).
#define RN_HEAD_SOFTMAX_STATS(row, classes, in_lds, srow, red_v, tid, lane, wave, mx, sum)                            \
    do {                                                                                                               \
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));                                \
        if (lane == 0) red_v[wave] = mx;                                                                               \
        __syncthreads();                                                                                               \
        mx = red_v[0];                                                                                                 \
        for (int w = 1; w < kHeadWaves; ++w) mx = fmaxf(mx, red_v[w]);                                                 \
        __syncthreads();                                                                                               \
        for (uint32_t i = tid; i < classes; i += kHeadBlock) sum += expf((in_lds ? srow[i] : row[i]) - mx);           \
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);                                        \
        if (lane == 0) red_v[wave] = sum;                                                                              \
        __syncthreads();                                                                                               \
        sum = red_v[0];                                                                                                \
        for (int w = 1; w < kHeadWaves; ++w) sum += red_v[w];                                                          \
    } while (0)

// ---- order, selection and sort (rn_rpn.hip's header) --------------------------------------------------------------
constexpr uint32_t kRpnBlock = 1024;  // select + decode and the merges: one block per segment / image
constexpr uint32_t kRpnMaxK = 4096;   // keys a selection holds in LDS (32 KiB)

struct sel_smem {
    uint64_t keys[kRpnMaxK];
    uint32_t hist[256];
    uint64_t prefix;
    uint32_t remaining, fill;
};

// the contract's min and max: a NaN first operand stays (torch.clamp's and numpy's rule)
__device__ __forceinline__ float rpn_min(float a, float b) { return a > b ? b : a; }
__device__ __forceinline__ float rpn_max(float a, float b) { return a < b ? b : a; }

__device__ __forceinline__ uint32_t rpn_mono(float v)
{
    uint32_t u = __float_as_uint(v);
    if (v != v) u = 0xFF800000u;   // a NaN ranks as -inf
    if (u == 0x80000000u) u = 0u;  // -0 == +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // never 0: -inf is 0x007FFFFF
}

// the value rpn_mono took (a NaN comes back as -inf, -0 as +0)
__device__ __forceinline__ float rpn_unmono(uint32_t m) { return __uint_as_float((m & 0x80000000u) ? (m & 0x7FFFFFFFu) : ~m); }

__device__ __forceinline__ uint64_t rpn_key(float v, uint32_t index) { return ((uint64_t)rpn_mono(v) << 32) | (uint32_t)~index; }

// Block-wide.  keys[0 .. want) hold `want` >= 1 unique nonzero keys in any order, want <= kRpnMaxK and every thread
// sees them (a barrier lies behind the last write); afterwards they are descending.  The bitonic network runs on the
// next power of two, padded with 0.
__device__ __forceinline__ void rpn_sort_desc(uint64_t *keys, uint32_t want)
{
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    uint32_t P = 2;
    while (P < want) P <<= 1;  // at most kRpnMaxK
    for (uint32_t i = want + tid; i < P; i += nt) keys[i] = 0;
    __syncthreads();
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < P / 2; t += nt) {
                const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t a = keys[lo], b = keys[hi];
                if ((a < b) == desc) keys[lo] = b, keys[hi] = a;
            }
            __syncthreads();
        }
    }
}

// Block-wide.  key_at(i), i < n, gives element i's key; keys are unique except for 0, which marks an absent element.
// want: 1 <= want <= min(number of nonzero keys, kRpnMaxK).  Afterwards s.keys[0 .. want) are the `want` greatest
// keys, descending.
template <typename KeyAt>
__device__ void rpn_select_sort(sel_smem &s, uint32_t n, uint32_t want, KeyAt key_at)
{
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    uint64_t kth = 0;  // want == n: every key is taken
    if (want < n) {
        uint64_t prefix = 0;
        uint32_t rem = want;
        for (int pass = 7; pass >= 0; --pass) {
            const int shift = pass * 8;
            if (tid < 256) s.hist[tid] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < n; i += nt) {
                const uint64_t key = key_at(i);
                if (pass == 7 || (key >> (shift + 8)) == prefix) atomicAdd(&s.hist[(uint32_t)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {  // wave 0: the digit whose bin holds the rem-th key from the top
                uint32_t c[4], tot = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) c[j] = s.hist[4 * tid + j], tot += c[j];
                uint32_t incl = tot;  // keys in this lane's bins and all higher ones
                for (uint32_t off = 1; off < 64; off <<= 1) {
                    const uint32_t v = __shfl_down(incl, off, 64);
                    if (tid + off < 64) incl += v;
                }
                uint32_t above = incl - tot;
                if (above < rem && rem <= incl) {  // exactly one lane
                    int d = 0;
                    bool found = false;
#pragma unroll
                    for (int j = 3; j >= 0; --j) {
                        if (found) continue;
                        if (rem <= above + c[j]) d = j, found = true;
                        else above += c[j];
                    }
                    s.prefix = (prefix << 8) | (uint64_t)(4 * tid + d);
                    s.remaining = rem - above;
                }
            }
            __syncthreads();
            prefix = s.prefix, rem = s.remaining;
        }
        kth = prefix;
    }
    if (tid == 0) s.fill = 0;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += nt) {
        const uint64_t key = key_at(i);
        if (key != 0 && key >= kth) {
            const uint32_t slot = atomicAdd(&s.fill, 1u);
            if (slot < kRpnMaxK) s.keys[slot] = key;
        }
    }
    __syncthreads();
    rpn_sort_desc(s.keys, want);
}

// ---- BoxCoder.decode_single + clip_boxes_to_image, the contract's "Decode" ----------------------------------
// (the arithmetic is a contract, operation by operation: no product of rpn_decode or rpn_iou is fused into an add)
struct decode_consts {
    float wx, wy, ww, wh, clip, img_w, img_h;
};

__device__ __forceinline__ void rpn_decode(const float a[4], const float d[4], const decode_consts &k, float out[4])
{
#pragma clang fp contract(off)
    const float wa = a[2] - a[0], ha = a[3] - a[1];
    const float cx = a[0] + 0.5f * wa, cy = a[1] + 0.5f * ha;
    const float dx = d[0] / k.wx, dy = d[1] / k.wy;
    const float dw = rpn_min(d[2] / k.ww, k.clip), dh = rpn_min(d[3] / k.wh, k.clip);
    const float pcx = dx * wa + cx, pcy = dy * ha + cy;
    const float pw = expf(dw) * wa, ph = expf(dh) * ha;
    const float hw = 0.5f * pw, hh = 0.5f * ph;
    out[0] = rpn_min(rpn_max(pcx - hw, 0.0f), k.img_w);
    out[1] = rpn_min(rpn_max(pcy - hh, 0.0f), k.img_h);
    out[2] = rpn_min(rpn_max(pcx + hw, 0.0f), k.img_w);
    out[3] = rpn_min(rpn_max(pcy + hh, 0.0f), k.img_h);
}

// the contract's IoU of the earlier box (x1, y1, x2, y2), whose area the caller formed as (x2 - x1) * (y2 - y1),
// and the later box (u1, v1, u2, v2); 0/0 is a NaN
__device__ __forceinline__ float rpn_iou(float x1, float y1, float x2, float y2, float area, float u1, float v1, float u2,
                                         float v2)
{
#pragma clang fp contract(off)
    const float area_c = (u2 - u1) * (v2 - v1);
    const float iw = (x2 < u2 ? x2 : u2) - (x1 > u1 ? x1 : u1), ih = (y2 < v2 ? y2 : v2) - (y1 > v1 ? y1 : v1);
    const float inter = (iw > 0.0f ? iw : 0.0f) * (ih > 0.0f ? ih : 0.0f);
    return inter / (area + area_c - inter);
}

}  // namespace

#endif
