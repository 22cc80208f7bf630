// Resize and centre-crop of decoded 8-bit RGB images of any size, PIL's bits (include/rn_hip.h,
// "resize and centre-crop"; the tables come from rn_resize_host.c).  One launch, no full-size
// intermediate: a block owns a band of R output rows of one image.  The source rows that band's
// vertical taps touch go through the horizontal pass -- crop columns only, rounded to 8 bits as PIL
// rounds them -- into LDS, `rows_cap` rows at a time; the vertical pass accumulates out of LDS into
// int32 registers, so a band that reads more rows than LDS holds (large reductions) simply takes
// more rounds: integer sums do not care in how many pieces they are added.  Thread t owns the bytes
// t, t + 256, ... of each of the band's rows (NCOL columns x R rows = RN_RS_ACC accumulators), which
// makes the vertical loop uniform across the block: bounds and coefficients are the same for every
// lane.  Source bytes are loaded one by one (images start at any byte), results stored one by one.
#include <stdlib.h>

#include "rn_internal.h"
#include "rn_resize.h"

namespace {

__device__ __forceinline__ uint32_t clip8(int32_t s)
{
    const int32_t v = s >> 22;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

template <int NCOL>
__global__ __launch_bounds__(256) void resize_crop_kernel(const uint8_t *__restrict__ src,
                                                          const uint32_t *__restrict__ tab, uint8_t *__restrict__ dst,
                                                          uint32_t b_base, uint32_t crop, uint32_t rows_cap)
{
    constexpr int R = RN_RS_ACC / NCOL;
    extern __shared__ uint8_t rows[];  // [rows_cap][crop * 3]: horizontal pass results
    const uint32_t tid = threadIdx.x;
    const uint32_t b = b_base + blockIdx.y;
    const uint32_t *d = tab + (uint64_t)b * RN_RS_DESC;
    const uint8_t *img = src + (((uint64_t)d[1] << 32) | d[0]);
    const int32_t *itab = reinterpret_cast<const int32_t *>(tab);
    const int32_t *hb = itab + d[4], *hk = itab + d[5], *vb = itab + d[7], *vk = itab + d[8];
    const uint32_t hks = d[6], vks = d[9], stride = d[10];
    const uint32_t crop3 = crop * 3;
    const uint32_t y0 = blockIdx.x * R;
    const uint32_t nrows = crop - y0 < (uint32_t)R ? crop - y0 : (uint32_t)R;
    // source rows of the band: bounds are monotone in the output row
    const int32_t r_lo = vb[2 * y0];
    const int32_t r_hi = vb[2 * (y0 + nrows - 1)] + vb[2 * (y0 + nrows - 1) + 1];
    const uint32_t step_r = 256 / crop, step_x = 256 - step_r * crop;

    int32_t acc[NCOL][R];
#pragma unroll
    for (int ci = 0; ci < NCOL; ++ci)
#pragma unroll
        for (int yr = 0; yr < R; ++yr) acc[ci][yr] = 0;

    for (int32_t c0 = r_lo; c0 < r_hi; c0 += (int32_t)rows_cap) {
        const int32_t c1 = c0 + (int32_t)rows_cap < r_hi ? c0 + (int32_t)rows_cap : r_hi;
        // horizontal pass of source rows [c0, c1): one pixel (three channels) per thread and step
        {
            const uint32_t nr = (uint32_t)(c1 - c0);
            uint32_t rr = tid / crop, x = tid - rr * crop;
            while (rr < nr) {
                const int32_t xmin = hb[2 * x], xmax = hb[2 * x + 1];
                const int32_t *k = hk + x * hks;
                const uint8_t *p = img + (uint64_t)(uint32_t)(c0 + (int32_t)rr) * stride + (uint32_t)xmin * 3;
                int32_t s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
                for (int32_t t = 0; t < xmax; ++t) {
                    const int32_t kk = k[t];
                    s0 += (int32_t)p[3 * t] * kk;
                    s1 += (int32_t)p[3 * t + 1] * kk;
                    s2 += (int32_t)p[3 * t + 2] * kk;
                }
                uint8_t *o = rows + rr * crop3 + x * 3;
                o[0] = (uint8_t)clip8(s0);
                o[1] = (uint8_t)clip8(s1);
                o[2] = (uint8_t)clip8(s2);
                rr += step_r;
                x += step_x;
                if (x >= crop) x -= crop, ++rr;
            }
        }
        __syncthreads();
        // vertical pass: the taps of every row of the band that fall into [c0, c1)
#pragma unroll
        for (int yr = 0; yr < R; ++yr) {
            if ((uint32_t)yr < nrows) {
                const int32_t ymin = vb[2 * (y0 + yr)], yend = ymin + vb[2 * (y0 + yr) + 1];
                const int32_t t0 = ymin > c0 ? ymin : c0, t1 = yend < c1 ? yend : c1;
                const int32_t *k = vk + (y0 + yr) * vks - ymin;
                for (int32_t r = t0; r < t1; ++r) {
                    const int32_t kk = k[r];
                    const uint8_t *row = rows + (uint32_t)(r - c0) * crop3;
#pragma unroll
                    for (int ci = 0; ci < NCOL; ++ci) {
                        const uint32_t xc = tid + 256 * ci;
                        if (xc < crop3) acc[ci][yr] += (int32_t)row[xc] * kk;
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int yr = 0; yr < R; ++yr) {
        if ((uint32_t)yr < nrows) {
            uint8_t *o = dst + ((uint64_t)b * crop + y0 + yr) * crop3;
#pragma unroll
            for (int ci = 0; ci < NCOL; ++ci) {
                const uint32_t xc = tid + 256 * ci;
                if (xc < crop3) o[xc] = (uint8_t)clip8((1 << 21) + acc[ci][yr]);
            }
        }
    }
}

template <int NCOL>
void launch(rn_ctx *ctx, const uint8_t *src, const void *tab, uint8_t *dst, uint64_t B, uint32_t crop)
{
    constexpr int R = RN_RS_ACC / NCOL;
    const uint32_t crop3 = crop * 3;
    // LDS: 32 rows of the horizontal pass (a band at scale 1.5 reads 15), fewer where a row is long: <= 64 KB
    uint32_t rows_cap = 65536 / crop3;
    if (rows_cap > 32) rows_cap = 32;
    for (uint64_t b0 = 0; b0 < B; b0 += 65535) {
        const uint64_t nb = (B - b0) < 65535 ? (B - b0) : 65535;
        resize_crop_kernel<NCOL><<<dim3((unsigned)rn_ceil_div(crop, R), (unsigned)nb), 256, rows_cap * crop3, ctx->stream>>>(
            src, (const uint32_t *)tab, dst, (uint32_t)b0, crop, rows_cap);
    }
}

}  // namespace

extern "C" {

int rn_image_u8_resize_crop_launch(rn_ctx *ctx, const uint8_t *packed_dev, const void *table_dev, uint64_t B,
                                   uint8_t *dst_dev, uint64_t crop)
{
    RN_ENTER(ctx);
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, packed_dev && table_dev && dst_dev, "null pointer");
    RN_REQUIRE(ctx, crop >= 1 && crop <= RN_RS_MAX_CROP, "crop must be 1..2048");
    RN_REQUIRE(ctx, B < (1ull << 31) / RN_RS_DESC, "batch too large");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(table_dev) & 15) == 0, "the table must be 16-byte aligned");
    const uint32_t ncol = (uint32_t)rn_ceil_div(crop * 3, 256);
    const uint32_t c = (uint32_t)crop;
    if (ncol <= 1) launch<1>(ctx, packed_dev, table_dev, dst_dev, B, c);
    else if (ncol <= 2) launch<2>(ctx, packed_dev, table_dev, dst_dev, B, c);
    else if (ncol <= 3) launch<3>(ctx, packed_dev, table_dev, dst_dev, B, c);
    else if (ncol <= 4) launch<4>(ctx, packed_dev, table_dev, dst_dev, B, c);
    else if (ncol <= 6) launch<6>(ctx, packed_dev, table_dev, dst_dev, B, c);
    else if (ncol <= 8) launch<8>(ctx, packed_dev, table_dev, dst_dev, B, c);
    else if (ncol <= 12) launch<12>(ctx, packed_dev, table_dev, dst_dev, B, c);
    else launch<24>(ctx, packed_dev, table_dev, dst_dev, B, c);
    return rn_after_launch(ctx, "rn_image_u8_resize_crop");
}

int rn_image_u8_resize_crop(rn_ctx *ctx, const uint8_t *packed_dev, const uint64_t *offsets, const uint64_t *heights,
                            const uint64_t *widths, uint64_t B, uint8_t *dst_dev, uint64_t resize, uint64_t crop)
{
    RN_ENTER(ctx);
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, packed_dev && offsets && heights && widths && dst_dev, "null pointer");
    RN_REQUIRE(ctx, B < (1ull << 31) / RN_RS_DESC, "batch too large");
    uint64_t bytes = 0;
    if (rn_image_u8_resize_crop_table(offsets, heights, widths, B, resize, crop, nullptr, 0, &bytes) != RN_OK)
        return rn_set_error(ctx, RN_ERR_INVALID,
                            "rn_image_u8_resize_crop: needs 1 <= crop <= resize, crop <= 2048, image sides 1..16384 "
                            "and at most 64 times their resized length");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    RN_HIP_TRY(ctx, hipStreamIsCapturing(ctx->stream, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return rn_set_error(ctx, RN_ERR_UNSUPPORTED, "rn_image_u8_resize_crop: uploads host tables, cannot be captured");
    void *host = malloc(bytes), *dev = nullptr;
    if (!host) return RN_ERR_NOMEM;
    int st = rn_image_u8_resize_crop_table(offsets, heights, widths, B, resize, crop, host, bytes, &bytes);
    if (st == RN_OK) st = rn_scratch(ctx, 5, bytes, &dev);
    if (st == RN_OK) st = rn_check_hip(ctx, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream), "table upload");
    // the table is pageable memory that is freed below: wait for the copy (what was queued before it as well)
    if (st == RN_OK) st = rn_check_hip(ctx, hipStreamSynchronize(ctx->stream), "table upload");
    free(host);
    if (st != RN_OK) return st;
    return rn_image_u8_resize_crop_launch(ctx, packed_dev, dev, B, dst_dev, crop);
}

}  // extern "C"
