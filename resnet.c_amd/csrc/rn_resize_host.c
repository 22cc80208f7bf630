/*
 * Host half of the device resize (rn_resize.hip): geometry of the preset and the integer coefficient
 * tables of PIL's 8-bit resample, in plain C doubles.  Built with -ffp-contract=off: a product and
 * a sum fused into one fma would move a tap boundary or a coefficient by one, and the contract is
 * PIL's bits (include/rn_hip.h, "resize and centre-crop").
 *
 * The table rn_image_u8_resize_crop_table builds, in 32-bit words:
 *   B descriptors of RN_RS_DESC words: byte offset of the image (lo, hi), H, W, then for the
 *   horizontal and the vertical axis (bounds index, coefficient index, ksize), row stride in bytes;
 *   then per distinct (H, W) of the batch the two axis tables: crop (xmin, xmax) pairs and crop rows
 *   of ksize coefficients.  Images of one size share their tables.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "rn_hip.h"
#include "rn_resize.h"

int rn_resize_crop_geometry(uint64_t H, uint64_t W, uint64_t resize, uint64_t crop, uint64_t *nh, uint64_t *nw,
                            uint64_t *top, uint64_t *left)
{
    uint64_t h, w, d;
    if (H == 0 || W == 0 || crop == 0 || crop > resize) return RN_ERR_INVALID;
    if (H > RN_RS_MAX_SIDE || W > RN_RS_MAX_SIDE || resize > RN_RS_MAX_SIDE) return RN_ERR_INVALID;
    if (W <= H) {
        w = resize;
        h = (uint64_t)((double)(resize * H) / (double)W);
    } else {
        w = (uint64_t)((double)(resize * W) / (double)H);
        h = resize;
    }
    if (h < crop || w < crop) return RN_ERR_INVALID;
    if (nh) *nh = h;
    if (nw) *nw = w;
    /* round((n - crop) / 2.0) with halves to even, as Python rounds */
    d = (w - crop) >> 1;
    if (left) *left = ((w - crop) & 1) && (d & 1) ? d + 1 : d;
    d = (h - crop) >> 1;
    if (top) *top = ((h - crop) & 1) && (d & 1) ? d + 1 : d;
    return RN_OK;
}

static uint64_t ksize_of(uint64_t in_size, uint64_t out_size)
{
    double fs = (double)in_size / (double)out_size;
    if (fs < 1.0) fs = 1.0;
    return (uint64_t)ceil(fs) * 2 + 1;
}

/* rows [first, first + count) of the axis in_size -> out_size; every row of ks ints written whole */
static void fill_axis(uint64_t in_size, uint64_t out_size, uint64_t first, uint64_t count, int32_t *bounds,
                      int32_t *kk, uint64_t ks, double *w)
{
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs, ss = 1.0 / fs;
    uint64_t i;
    for (i = 0; i < count; ++i) {
        const double center = ((double)(first + i) + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        int xmax = (int)(center + support + 0.5);
        int32_t *k = kk + i * ks;
        double ww = 0.0;
        int x;
        if (xmin < 0) xmin = 0;
        if (xmax > (int)in_size) xmax = (int)in_size;
        xmax -= xmin;
        for (x = 0; x < xmax; ++x) {
            double a = ((double)(x + xmin) - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w[x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[x];
        }
        for (x = 0; x < xmax; ++x) {
            if (ww != 0.0) w[x] /= ww;
            k[x] = (int32_t)(0.5 + w[x] * (double)(1 << 22));
        }
        for (; x < (int)ks; ++x) k[x] = 0;
        bounds[2 * i] = xmin;
        bounds[2 * i + 1] = xmax;
    }
}

int rn_resize_coefficients(uint64_t in_size, uint64_t out_size, uint64_t first, uint64_t count, int32_t *bounds_out,
                           int32_t *coeffs_out, uint64_t cap, uint64_t *ksize)
{
    uint64_t ks;
    double *w;
    if (in_size == 0 || out_size == 0 || in_size > RN_RS_MAX_SIDE || out_size > RN_RS_MAX_SIDE) return RN_ERR_INVALID;
    if (first + count > out_size) return RN_ERR_INVALID;
    ks = ksize_of(in_size, out_size);
    if (ksize) *ksize = ks;
    if (count * ks > cap || (count && (!bounds_out || !coeffs_out))) return RN_ERR_INVALID;
    w = (double *)malloc(ks * sizeof(double));
    if (!w) return RN_ERR_NOMEM;
    fill_axis(in_size, out_size, first, count, bounds_out, coeffs_out, ks, w);
    free(w);
    return RN_OK;
}

int rn_image_u8_resize_crop_table(const uint64_t *offsets, const uint64_t *heights, const uint64_t *widths, uint64_t B,
                                  uint64_t resize, uint64_t crop, void *table, uint64_t cap, uint64_t *bytes)
{
    uint32_t *t = (uint32_t *)table;
    uint64_t words = B * RN_RS_DESC, i, j;
    double w[2 * RN_RS_MAX_SCALE + 3];
    int pass;
    if (bytes) *bytes = 0;
    if (B == 0) return RN_OK;
    if (!offsets || !heights || !widths) return RN_ERR_INVALID;
    if (crop == 0 || crop > resize || crop > RN_RS_MAX_CROP || resize > RN_RS_MAX_SIDE) return RN_ERR_INVALID;
    /* pass 0 checks every image and sizes the table, pass 1 fills it */
    for (pass = 0; pass < 2; ++pass) {
        words = B * RN_RS_DESC;
        for (i = 0; i < B; ++i) {
            const uint64_t H = heights[i], W = widths[i];
            uint64_t nh, nw, top, left, ksh, ksv;
            if (rn_resize_crop_geometry(H, W, resize, crop, &nh, &nw, &top, &left) != RN_OK) return RN_ERR_INVALID;
            if (H > RN_RS_MAX_SCALE * nh || W > RN_RS_MAX_SCALE * nw) return RN_ERR_INVALID;
            ksh = ksize_of(W, nw);
            ksv = ksize_of(H, nh);
            for (j = 0; j < i; ++j)
                if (heights[j] == H && widths[j] == W) break;
            if (pass) {
                uint32_t *d = t + i * RN_RS_DESC;
                d[0] = (uint32_t)offsets[i];
                d[1] = (uint32_t)(offsets[i] >> 32);
                d[2] = (uint32_t)H;
                d[3] = (uint32_t)W;
                d[10] = (uint32_t)(W * 3);
                d[11] = 0;
                if (j < i) {
                    memcpy(d + 4, t + j * RN_RS_DESC + 4, 6 * sizeof(uint32_t));
                } else {
                    d[4] = (uint32_t)words;
                    d[5] = (uint32_t)(words + 2 * crop);
                    d[6] = (uint32_t)ksh;
                    d[7] = (uint32_t)(words + crop * (2 + ksh));
                    d[8] = (uint32_t)(words + crop * (2 + ksh) + 2 * crop);
                    d[9] = (uint32_t)ksv;
                    fill_axis(W, nw, left, crop, (int32_t *)t + d[4], (int32_t *)t + d[5], ksh, w);
                    fill_axis(H, nh, top, crop, (int32_t *)t + d[7], (int32_t *)t + d[8], ksv, w);
                }
            }
            if (j == i) words += crop * (4 + ksh + ksv);
        }
        if (words >= (1ull << 31)) return RN_ERR_INVALID; /* indices are 32-bit words */
        if (bytes) *bytes = words * 4;
        if (!table || words * 4 > cap) return table ? RN_ERR_INVALID : RN_OK;
    }
    return RN_OK;
}
