// RoIAlign over a pyramid: torchvision's MultiScaleRoIAlign as ONE launch (rn_roi_align_forward_dt), every RoI
// choosing its level inside the kernel, and the level thresholds that choice reads (rn_roi_level_thresholds).  The
// reference classifies whole images only; nothing here has a counterpart in it.
#include <math.h>
#include <string.h>

#include "rn_conv_params.h"
#include "rn_internal.h"
#include "rn_private.h"

// The pooler's arithmetic is a contract, operation by operation (rn_hip.h): no product of this file is fused into
// an add, for the reason rn_seg.hip gives.
#pragma clang fp contract(off)

using rn_gemm::bf16_t;
using rn_gemm::u32x4;

namespace {

// ---- the kernel ---------------------------------------------------------------------------------------------
// One block: one RoI and a slab of `sl` 16-byte chunks of channels (gridDim.x slabs; the RoIs stride gridDim.y).
// An item is (bin, chunk of the slab), consecutive lanes on consecutive chunks: the four corners of a sample are
// four runs of sl * 16 bytes, each lane's loads (sixteen at S = 2, fewer where samples share pixels) independent of
// one another.  The bin's V values
// (4 fp32 / 8 bf16 channels) are summed in registers in the contract's order and go to LDS; the slab's nc * bins
// outputs are ONE contiguous run of dst, which the block then stores by rn_nhwc_to_nchw_dt's rule: 16 bytes
// wherever four consecutive outputs share an aligned 16 bytes, scalars only at the run's head and tail.
// LDS: output t of the run (t = channel * bins + bin) sits `sh` floats behind an aligned quad of dst (sh = 0..3, the
// run's misalignment); with u = t + sh it is stored at (u >> 2) + (u & 3) * Q -- four planes of Q quads.  The store
// phase reads plane e at consecutive quads on consecutive lanes (conflict free, no division); the item phase
// writes dwords whose planes rotate with the bin, Q = 8 (mod 32) keeping eight consecutive quads of the four
// planes on 32 distinct banks.  16 * Q bytes, at most kRoiLdsCap + 512.
constexpr uint32_t kRoiBlock = 256;
constexpr uint64_t kRoiLdsCap = 36 * 1024;  // bytes of outputs a block holds: 64 fp32 channels at 7 x 7, 32 at 14 x 14
constexpr int kRoiMaxLevels = 4;

struct roi_args {
    const uint4 *map[kRoiMaxLevels];  // image img_lo of every level
    uint32_t h[kRoiMaxLevels], w[kRoiMaxLevels];
    float scale[kRoiMaxLevels], thr[kRoiMaxLevels - 1];
    const float *rois;
    float *out;
    int32_t *levels;
    uint32_t n, K, C, cpp;            // levels, RoIs, channels, chunks of a pixel
    uint32_t images, img_lo, img_cnt; // valid image indices 0 .. images - 1; this launch holds img_lo .. + img_cnt
    uint32_t write_invalid;           // this launch writes the rows whose image index is invalid
    uint32_t PH, PW, bins, mul_pw, shr_pw;
    uint32_t sl, sl_log2, Q;
    uint32_t aligned;
};

template <typename T>
__device__ __forceinline__ void roi_unpack(const uint4 a, float (&v)[16 / sizeof(T)])
{
    const u32x4 u{a.x, a.y, a.z, a.w};
    rn_gemm::OutVec<T>::unpack(u, v);  // a bf16 value is widened exactly
}

// one axis of a sample, the contract's "One sample": the two indices (always inside [0, n)) and the two weights
__device__ __forceinline__ void roi_axis(float c, uint32_t n, uint32_t *lo, uint32_t *hi, float *l, float *hw)
{
    c = c > 0.0f ? c : 0.0f;  // max(c, 0); the caller has replaced a coordinate outside [-1, n] (a NaN too) by 0
    int i = (int)c;
    int j;
    if (i >= (int)n - 1) {
        i = j = (int)n - 1;
        c = (float)i;
    } else {
        j = i + 1;
    }
    i = i < 0 ? 0 : i, j = j < 0 ? 0 : j;  // unconditional: no RoI content indexes outside its map
    i = i > (int)n - 1 ? (int)n - 1 : i, j = j > (int)n - 1 ? (int)n - 1 : j;
    *lo = (uint32_t)i, *hi = (uint32_t)j;
    *l = c - (float)i;
    *hw = 1.0f - *l;
}

// NHWC: the store layout [K, PH, PW, C] of rn_roi_align_nhwc_forward_dt.  An item's V values are 16 (bf16 maps: 32)
// consecutive bytes of that layout, so the thread stores its acc[] itself: no tile, no barrier, the same values.
template <typename T, int S, bool NHWC>
__global__ __launch_bounds__(kRoiBlock) void roi_align_kernel(const roi_args p)
{
    constexpr int V = 16 / sizeof(T), UY = S <= 2 ? S : 1;  // the sample rows unrolled: a row's loads are in flight together
    extern __shared__ float tile[];  // 4 * Q floats
    const uint32_t c0 = blockIdx.x * p.sl * V;  // first channel of the slab
    const uint32_t nc = p.C - c0 < p.sl * V ? p.C - c0 : p.sl * V, nch = nc / V;
    const uint32_t len = nc * p.bins;
    for (uint32_t r = blockIdx.y; r < p.K; r += gridDim.y) {
        const float *roi = p.rois + (uint64_t)r * 5;
        const float bf = roi[0], x1 = roi[1], y1 = roi[2], x2 = roi[3], y2 = roi[4];
        // the image: an integer in [0, images), or the row is zeros and the level -1
        const bool integral = bf >= 0.0f && bf < 2147483648.0f && bf == truncf(bf);
        const uint32_t ib = integral ? (uint32_t)bf : 0u;
        const bool valid = integral && ib < p.images;
        const uint32_t il = ib - p.img_lo;  // wraps below the window
        const bool mine = valid ? il < p.img_cnt : p.write_invalid != 0;
        if (!mine) continue;  // uniform: the whole block skips the row, another launch writes it
        // the level: thresholds on the area in image pixels, no logarithm
        const float area = (x2 - x1) * (y2 - y1);
        uint32_t lvl = 0;
#pragma unroll
        for (int j = 0; j < kRoiMaxLevels - 1; ++j)
            if (j + 1 < (int)p.n && area >= p.thr[j]) ++lvl;
        const uint4 *map = p.map[0];
        uint32_t h = p.h[0], w = p.w[0];
        float scale = p.scale[0];
#pragma unroll
        for (int j = 1; j < kRoiMaxLevels; ++j)
            if (lvl == (uint32_t)j) map = p.map[j], h = p.h[j], w = p.w[j], scale = p.scale[j];
        if (blockIdx.x == 0 && threadIdx.x == 0 && p.levels) p.levels[r] = valid ? (int32_t)lvl : -1;

        // the RoI's extent on the level
        const float off = p.aligned ? 0.5f : 0.0f;
        const float x1s = x1 * scale - off, y1s = y1 * scale - off;
        const float x2s = x2 * scale - off, y2s = y2 * scale - off;
        float rw = x2s - x1s, rh = y2s - y1s;
        if (!p.aligned) rw = rw < 1.0f ? 1.0f : rw, rh = rh < 1.0f ? 1.0f : rh;
        const float bin_h = rh / (float)p.PH, bin_w = rw / (float)p.PW;
        const float fh = (float)h, fw = (float)w;
        const uint4 *img = map + (uint64_t)il * h * w * p.cpp + (c0 / V);

        float *run = p.out + ((uint64_t)r * p.C + c0) * p.bins;  // the slab's outputs: one run of len floats
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(run) >> 2) & 3;  // floats behind the aligned quad

        const uint32_t items = p.bins << p.sl_log2;
        for (uint32_t i = threadIdx.x; i < items; i += kRoiBlock) {
            const uint32_t b = i >> p.sl_log2, k = i & (p.sl - 1);
            if (k >= nch) continue;
            float acc[V];
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] = 0.0f;
            if (valid) {
                const uint32_t ph = rn_gemm::fast_div(b, (int)p.PW, p.mul_pw, p.shr_pw), pw = b - ph * p.PW;
                const uint4 *src = img + k;
                // the bin's 2 S columns (xl, xh of every sample column) and their weights, once
                uint32_t cx[2 * S];
                float lx[S], hx[S];
                bool x_in[S];
#pragma unroll
                for (int ix = 0; ix < S; ++ix) {
                    const float x = x1s + (float)pw * bin_w + ((float)ix + 0.5f) * bin_w / (float)S;
                    x_in[ix] = x >= -1.0f && x <= fw;  // false for a NaN coordinate
                    roi_axis(x_in[ix] ? x : 0.0f, w, &cx[2 * ix], &cx[2 * ix + 1], &lx[ix], &hx[ix]);
                }
                // Neighbouring samples of a bin mostly share pixels (a bin of the level a RoI is sent to is about a
                // pixel wide).  On fp32 maps a pixel is loaded once: a column that is one of the two before it, and
                // (S <= 2, where the registers allow it) a row that is one of the previous sample row's two, takes
                // the chunk already in registers.  Equal indices, equal values: the arithmetic and its order are
                // untouched.  On bf16 maps every corner is loaded: half the bytes per chunk and twice the values to
                // select made the shared form the slower one when both were measured (profiles/roi_align).
                uint4 pl[2 * S], pu[2 * S];  // the previous sample row's chunks at rows yl, yh (ROWS only)
                uint32_t pyl = 0, pyh = 0;
                constexpr bool COLS = sizeof(T) == 4, ROWS = COLS && S <= 2;
#pragma unroll UY
                for (int iy = 0; iy < S; ++iy) {
                    const float y = y1s + (float)ph * bin_h + ((float)iy + 0.5f) * bin_h / (float)S;
                    const bool y_in = y >= -1.0f && y <= fh;
                    uint32_t yl, yh;
                    float ly, hy;
                    roi_axis(y_in ? y : 0.0f, h, &yl, &yh, &ly, &hy);
                    const uint4 *row_l = src + (uint64_t)yl * w * p.cpp, *row_h = src + (uint64_t)yh * w * p.cpp;
                    const bool l_pl = ROWS && iy > 0 && yl == pyl, l_pu = ROWS && iy > 0 && yl == pyh;
                    const bool u_l = COLS && yh == yl, u_pl = ROWS && iy > 0 && yh == pyl, u_pu = ROWS && iy > 0 && yh == pyh;
                    uint4 ql[2 * S], qu[2 * S];
#pragma unroll
                    for (int j = 0; j < 2 * S; ++j) {
                        const bool c1 = COLS && j >= 1 && cx[j] == cx[j >= 1 ? j - 1 : 0];
                        const bool c2 = COLS && j >= 2 && cx[j] == cx[j >= 2 ? j - 2 : 0];
                        if (l_pl) ql[j] = pl[j];
                        else if (l_pu) ql[j] = pu[j];
                        else if (c1) ql[j] = ql[j >= 1 ? j - 1 : 0];
                        else if (c2) ql[j] = ql[j >= 2 ? j - 2 : 0];
                        else ql[j] = row_l[(uint64_t)cx[j] * p.cpp];
                        if (u_l) qu[j] = ql[j];
                        else if (u_pu) qu[j] = pu[j];
                        else if (u_pl) qu[j] = pl[j];
                        else if (c1) qu[j] = qu[j >= 1 ? j - 1 : 0];
                        else if (c2) qu[j] = qu[j >= 2 ? j - 2 : 0];
                        else qu[j] = row_h[(uint64_t)cx[j] * p.cpp];
                    }
#pragma unroll
                    for (int ix = 0; ix < S; ++ix) {
                        const bool in = y_in && x_in[ix];
                        float v1[V], v2[V], v3[V], v4[V];
                        roi_unpack<T>(ql[2 * ix], v1), roi_unpack<T>(ql[2 * ix + 1], v2);
                        roi_unpack<T>(qu[2 * ix], v3), roi_unpack<T>(qu[2 * ix + 1], v4);
                        const float w1 = hy * hx[ix], w2 = hy * lx[ix], w3 = ly * hx[ix], w4 = ly * lx[ix];
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            const float val = w1 * v1[e] + w2 * v2[e] + w3 * v3[e] + w4 * v4[e];
                            acc[e] = in ? acc[e] + val : acc[e];
                        }
                    }
                    if (ROWS) {
                        pyl = yl, pyh = yh;
#pragma unroll
                        for (int j = 0; j < 2 * S; ++j) pl[j] = ql[j], pu[j] = qu[j];
                    }
                }
            }
            if (NHWC) {
                float4 *dst = reinterpret_cast<float4 *>(p.out + ((uint64_t)r * p.bins + b) * p.C + c0 + k * V);
#pragma unroll
                for (int e = 0; e < V; e += 4)
                    dst[e / 4] = make_float4(acc[e] / (float)(S * S), acc[e + 1] / (float)(S * S), acc[e + 2] / (float)(S * S),
                                             acc[e + 3] / (float)(S * S));
                continue;
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint32_t u = (k * V + e) * p.bins + b + sh;
                tile[(u >> 2) + (u & 3) * p.Q] = acc[e] / (float)(S * S);
            }
        }
        if (NHWC) continue;  // nothing of the block is shared: the next RoI may start
        __syncthreads();
        const uint32_t quads = (len + sh + 3) >> 2;
        for (uint32_t q = threadIdx.x; q < quads; q += kRoiBlock) {
            const uint32_t t0 = 4 * q - sh;  // wraps below 0: those elements are outside the run
            float v[4];
            bool in[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                in[e] = t0 + e < len;
                v[e] = in[e] ? tile[q + e * p.Q] : 0.0f;
            }
            if (in[0] && in[3]) {  // the whole quad is inside: run + t0 is 16-byte aligned by construction
                *reinterpret_cast<float4 *>(run + t0) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (in[e]) run[(uint32_t)(t0 + e)] = v[e];
            }
        }
        __syncthreads();  // the next RoI of the block reuses the tile
    }
}

template <typename T, bool NHWC>
void roi_launch_s(int S, dim3 grid, size_t lds, hipStream_t stream, const roi_args &p)
{
    switch (S) {
    case 1: roi_align_kernel<T, 1, NHWC><<<grid, kRoiBlock, lds, stream>>>(p); break;
    case 2: roi_align_kernel<T, 2, NHWC><<<grid, kRoiBlock, lds, stream>>>(p); break;
    case 3: roi_align_kernel<T, 3, NHWC><<<grid, kRoiBlock, lds, stream>>>(p); break;
    default: roi_align_kernel<T, 4, NHWC><<<grid, kRoiBlock, lds, stream>>>(p); break;
    }
}

// the launch of either form, no checks
int roi_window(rn_ctx *ctx, bool nhwc, int dtype, uint64_t n_levels, const void *const *x_nhwc, const uint64_t *h,
               const uint64_t *w, const float *scales, const float *thr, uint64_t images, uint64_t img_lo, uint64_t img_cnt,
               int write_invalid, uint64_t C, const float *rois_dev, uint64_t K, uint64_t PH, uint64_t PW, int sampling_ratio,
               int aligned, float *out, int32_t *levels_out)
{
    const uint64_t V = 16 / rn_elem_size(dtype), bins = PH * PW, cpp = C / V;
    roi_args p;
    memset(&p, 0, sizeof(p));
    for (uint64_t i = 0; i < n_levels; ++i) {
        p.map[i] = (const uint4 *)x_nhwc[i], p.h[i] = (uint32_t)h[i], p.w[i] = (uint32_t)w[i], p.scale[i] = scales[i];
        if (i + 1 < n_levels) p.thr[i] = thr[i];
    }
    p.rois = rois_dev, p.out = out, p.levels = levels_out;
    p.n = (uint32_t)n_levels, p.K = (uint32_t)K, p.C = (uint32_t)C, p.cpp = (uint32_t)cpp;
    p.images = (uint32_t)images, p.img_lo = (uint32_t)img_lo, p.img_cnt = (uint32_t)img_cnt;
    p.write_invalid = write_invalid ? 1u : 0u;
    p.PH = (uint32_t)PH, p.PW = (uint32_t)PW, p.bins = (uint32_t)bins;
    rn_fast_div(p.PW, &p.mul_pw, &p.shr_pw);
    // the slab: the most chunks (a power of two, at most 64 channels of fp32 / bf16 lanes' worth) whose outputs fit
    uint32_t sl = 1, lg = 0;
    while (sl * 2 * V <= 64 && sl < cpp && (uint64_t)sl * 2 * V * bins * sizeof(float) <= kRoiLdsCap) sl *= 2, ++lg;
    p.sl = sl, p.sl_log2 = lg;
    uint32_t Q = (uint32_t)((sl * V * bins + 6) / 4 + 1);
    Q += (8 + 32 - Q % 32) % 32;  // Q = 8 (mod 32)
    p.Q = Q;
    p.aligned = aligned ? 1u : 0u;
    const size_t lds = nhwc ? 0 : (size_t)Q * 4 * sizeof(float);  // the NHWC form has no tile
    const dim3 grid((unsigned)rn_ceil_div(cpp, sl), (unsigned)(K < 65535 ? K : 65535));
    if (nhwc) {
        if (dtype == RN_DTYPE_BF16) roi_launch_s<bf16_t, true>(sampling_ratio, grid, lds, ctx->stream, p);
        else roi_launch_s<float, true>(sampling_ratio, grid, lds, ctx->stream, p);
        return rn_after_launch(ctx, "rn_roi_align_nhwc_forward_dt");
    }
    if (dtype == RN_DTYPE_BF16) roi_launch_s<bf16_t, false>(sampling_ratio, grid, lds, ctx->stream, p);
    else roi_launch_s<float, false>(sampling_ratio, grid, lds, ctx->stream, p);
    return rn_after_launch(ctx, "rn_roi_align_forward_dt");
}

#define ROI_REQUIRE(cond, msg)                                                            \
    do {                                                                                  \
        if (!(cond)) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, (msg));       \
    } while (0)
// both public forms: every check, then the launch.  fn: the entry point's name in a refusal
int roi_forward(rn_ctx *ctx, const char *fn, bool nhwc, int dtype, uint64_t n_levels, const void *const *x_nhwc,
                const uint64_t *h, const uint64_t *w, const float *scales, const float *thr, uint64_t B, uint64_t C,
                const float *rois_dev, uint64_t K, uint64_t PH, uint64_t PW, int sampling_ratio, int aligned, float *out,
                int32_t *levels_out)
{
    RN_ENTER(ctx);
    ROI_REQUIRE(dtype == RN_DTYPE_F32 || dtype == RN_DTYPE_BF16, "unknown dtype");
    ROI_REQUIRE(n_levels >= 1 && n_levels <= (uint64_t)kRoiMaxLevels, "n_levels must be 1..4");
    ROI_REQUIRE(x_nhwc && h && w && scales, "x_nhwc, h, w or scales is NULL");
    ROI_REQUIRE(n_levels == 1 || thr, "thr is NULL (n_levels - 1 thresholds)");
    ROI_REQUIRE(PH >= 1 && PH <= 32 && PW >= 1 && PW <= 32, "PH and PW must be 1..32");
    if (sampling_ratio <= 0)
        return rn_set_error(ctx, RN_ERR_UNSUPPORTED, "%s: sampling_ratio <= 0 (adaptive grids) is not carried", fn);
    ROI_REQUIRE(sampling_ratio <= 4, "sampling_ratio must be 1..4");
    ROI_REQUIRE(aligned == 0 || aligned == 1, "aligned must be 0 or 1");
    const uint64_t es = rn_elem_size(dtype), per = 16 / es;
    ROI_REQUIRE(C >= 1 && C < (1ull << 31) && C % per == 0, "C must be a multiple of 16 bytes (and below 2^31)");
    ROI_REQUIRE(B < (1ull << 31) && K < (1ull << 31), "B and K must be below 2^31");
    for (uint64_t i = 0; i < n_levels; ++i) {
        ROI_REQUIRE(h[i] >= 1 && w[i] >= 1, "h and w must be >= 1");
        ROI_REQUIRE(h[i] < (1ull << 31) && w[i] < (1ull << 31) && h[i] * w[i] < (1ull << 31) &&
                            B * h[i] * w[i] < (1ull << 31),
                   "B * h * w must be below 2^31");
        ROI_REQUIRE(scales[i] > 0.0f && isfinite(scales[i]), "every scale must be positive and finite");
    }
    if (K == 0 || B == 0) return RN_OK;
    ROI_REQUIRE(rois_dev, "rois_dev is NULL");
    ROI_REQUIRE(out, "out is NULL");
    ROI_REQUIRE((reinterpret_cast<uintptr_t>(rois_dev) & 3) == 0, "rois_dev is off a 4-byte boundary");
    if (nhwc) ROI_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "out is off a 16-byte boundary");
    ROI_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "out is off a 4-byte boundary");
    ROI_REQUIRE((reinterpret_cast<uintptr_t>(levels_out) & 3) == 0, "levels_out is off a 4-byte boundary");
    const uint64_t out_bytes = K * C * PH * PW * sizeof(float);
    for (uint64_t i = 0; i < n_levels; ++i) {
        ROI_REQUIRE(x_nhwc[i], "a level's map is NULL");
        ROI_REQUIRE((reinterpret_cast<uintptr_t>(x_nhwc[i]) & 15) == 0, "a level's map is off a 16-byte boundary");
        ROI_REQUIRE(!rn_overlap(out, out_bytes, x_nhwc[i], B * h[i] * w[i] * C * es), "out overlaps a level's map");
        ROI_REQUIRE(!levels_out || !rn_overlap(levels_out, K * 4, x_nhwc[i], B * h[i] * w[i] * C * es),
                   "levels_out overlaps a level's map");
    }
    ROI_REQUIRE(!rn_overlap(out, out_bytes, rois_dev, K * 5 * sizeof(float)), "out overlaps rois_dev");
    ROI_REQUIRE(!levels_out || !rn_overlap(levels_out, K * 4, rois_dev, K * 5 * sizeof(float)),
               "levels_out overlaps rois_dev");
    ROI_REQUIRE(!levels_out || !rn_overlap(levels_out, K * 4, out, out_bytes), "levels_out overlaps out");
    return roi_window(ctx, nhwc, dtype, n_levels, x_nhwc, h, w, scales, thr, B, 0, B, 1, C, rois_dev, K, PH, PW, sampling_ratio,
                      aligned, out, levels_out);
}
#undef ROI_REQUIRE


}  // namespace

extern "C" {

int rn_roi_level_thresholds(uint64_t n_levels, const float *scales, double canonical_scale, int canonical_level,
                            float *thr_out)
{
    if (n_levels < 1 || n_levels > (uint64_t)kRoiMaxLevels || !scales || (n_levels > 1 && !thr_out)) return RN_ERR_INVALID;
    if (!(canonical_scale > 0.0)) return RN_ERR_INVALID;
    for (uint64_t i = 0; i < n_levels; ++i)
        if (!(scales[i] > 0.0f) || !isfinite(scales[i])) return RN_ERR_INVALID;
    const double k_min = floor(-log2((double)scales[0]) + 0.5);  // torchvision's LevelMapper: k_min of the finest scale
    for (uint64_t j = 0; j + 1 < n_levels; ++j) {
        const double side = canonical_scale * exp2(k_min + 1.0 + (double)j - (double)canonical_level - 1e-6);
        const double t = side * side;
        float f = (float)t;
        if ((double)f < t) f = nextafterf(f, INFINITY);  // rounded up: area >= thr in fp32 only where it is in double
        thr_out[j] = f;
    }
    return RN_OK;
}

int rn_roi_align_window(rn_ctx *ctx, int dtype, uint64_t n_levels, const void *const *x_nhwc, const uint64_t *h,
                        const uint64_t *w, const float *scales, const float *thr, uint64_t images, uint64_t img_lo,
                        uint64_t img_cnt, int write_invalid, uint64_t C, const float *rois_dev, uint64_t K, uint64_t PH,
                        uint64_t PW, int sampling_ratio, int aligned, float *out, int32_t *levels_out)
{
    return roi_window(ctx, false, dtype, n_levels, x_nhwc, h, w, scales, thr, images, img_lo, img_cnt, write_invalid, C,
                      rois_dev, K, PH, PW, sampling_ratio, aligned, out, levels_out);
}

int rn_roi_align_nhwc_window(rn_ctx *ctx, int dtype, uint64_t n_levels, const void *const *x_nhwc, const uint64_t *h,
                             const uint64_t *w, const float *scales, const float *thr, uint64_t images, uint64_t img_lo,
                             uint64_t img_cnt, int write_invalid, uint64_t C, const float *rois_dev, uint64_t K, uint64_t PH,
                             uint64_t PW, int sampling_ratio, int aligned, float *out, int32_t *levels_out)
{
    return roi_window(ctx, true, dtype, n_levels, x_nhwc, h, w, scales, thr, images, img_lo, img_cnt, write_invalid, C,
                      rois_dev, K, PH, PW, sampling_ratio, aligned, out, levels_out);
}

int rn_roi_align_forward_dt(rn_ctx *ctx, int dtype, uint64_t n_levels, const void *const *x_nhwc, const uint64_t *h,
                            const uint64_t *w, const float *scales, const float *thr, uint64_t B, uint64_t C,
                            const float *rois_dev, uint64_t K, uint64_t PH, uint64_t PW, int sampling_ratio, int aligned,
                            float *out, int32_t *levels_out)
{
    return roi_forward(ctx, __func__, false, dtype, n_levels, x_nhwc, h, w, scales, thr, B, C, rois_dev, K, PH, PW,
                       sampling_ratio, aligned, out, levels_out);
}

int rn_roi_align_nhwc_forward_dt(rn_ctx *ctx, int dtype, uint64_t n_levels, const void *const *x_nhwc, const uint64_t *h,
                                 const uint64_t *w, const float *scales, const float *thr, uint64_t B, uint64_t C,
                                 const float *rois_dev, uint64_t K, uint64_t PH, uint64_t PW, int sampling_ratio, int aligned,
                                 float *out_nhwc, int32_t *levels_out)
{
    return roi_forward(ctx, __func__, true, dtype, n_levels, x_nhwc, h, w, scales, thr, B, C, rois_dev, K, PH, PW,
                       sampling_ratio, aligned, out_nhwc, levels_out);
}

}  // extern "C"
