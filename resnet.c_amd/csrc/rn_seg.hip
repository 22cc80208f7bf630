// Semantic segmentation: the bilinear upsample of per-pixel class scores with an optional fused argmax
// (rn_upsample_bilinear_forward), the channel concat with a per-image broadcast source
// (rn_concat_channels_forward_dt), and torchvision's FCNHead and DeepLabHead as the two kinds of one object over the
// library's own convolutions (rn_seg_head_*).  The reference classifies whole images only; nothing here has a
// counterpart in it.
#include <stdlib.h>
#include <string.h>

#include "rn_conv_params.h"
#include "rn_internal.h"
#include "rn_private.h"

// The upsample's arithmetic is a contract, operation by operation (rn_hip.h): no product of this file is fused into
// an add.  (HIP's __fmul_rn / __fadd_rn are plain operators in a header compiled with contraction on: after
// inlining they fuse like any other, so the kernel writes plain operators under this pragma instead.)
#pragma clang fp contract(off)

namespace {

// ---- the upsample kernel ----------------------------------------------------------------------------------
// One block: kSegTY output rows x kSegTX output columns of one image, 256 threads = 16 rows of 16 lanes, every
// lane a run of four consecutive output X (lanes adjacent along W).  The source pixels the tile reads -- rows
// y0(first row) .. y1(last row), columns likewise, all `classes` channels -- are staged in LDS once, pixel-major
// with an odd pitch (classes | 1), from 16-byte loads along the channels.  A tile whose footprint does not fit
// the LDS the launch was given (shrinking, or identity on a large map) reads the source from global memory
// instead: the same arithmetic, merely correct.  A thread then walks the channels: four outputs per channel from
// the contract's fp32 operations, none fused; the running maximum and its index stay in registers; scores go to
// the channel's NCHW plane.
// Stores follow rn_nhwc_to_nchw_dt's rule: 16 bytes wherever four consecutive outputs share an aligned 16 bytes of
// dst, whatever W and the address of dst are.  The thread's run is fixed (the argmax needs that), so an aligned
// quad that starts s = 1..3 floats into the run takes its last s values from the next lane (one __shfl_down per
// value); the run's first s values then belong to the previous lane's quad.  Scalars remain at the ends of a
// tile row: where no previous lane or no full quad exists.  Labels do the same with bytes and 4-byte words.
constexpr int kSegTX = 64, kSegTY = 16;
constexpr uint32_t kSegLdsCap = 32 * 1024;  // bytes of LDS a launch asks for at most

// the contract's source coordinate of output o: index pair and the weight of the second
__device__ inline void seg_coord(uint32_t o, float scale, uint32_t n_in, uint32_t *i0, uint32_t *i1, float *l1)
{
    const float c = (float)o + 0.5f;
    float s = scale * c - 0.5f;
    s = s > 0.0f ? s : 0.0f;
    uint32_t a = (uint32_t)(int)s;
    if (a > n_in - 1) a = n_in - 1;
    *i0 = a;
    *i1 = a + 1 < n_in ? a + 1 : n_in - 1;
    *l1 = s - (float)a;
}

struct seg_args {
    const float *src;
    float *scores;
    uint8_t *labels;
    uint32_t h, w, classes, cs, H, W, tiles_x;
    float scale_h, scale_w;
    uint32_t lds_floats;
};

// the channel walk of one thread.  v: element (row 0, column 0, channel 0) of what the offsets index (the LDS
// tile or the image in global memory); oy / ox: float offsets of the two rows and of the 2 x 4 columns
template <bool SCORES, bool LABELS, typename O>  // O: uint32_t inside the LDS tile, uint64_t inside an image
__device__ inline void seg_walk(const seg_args &p, const float *v, O oy0, O oy1, float a0, float a1,
                                const O (&ox0)[4], const O (&ox1)[4], const float (&b0)[4],
                                const float (&b1)[4], uint64_t img, uint32_t Y, bool row_ok, uint32_t X0, uint32_t Xend,
                                uint32_t q)
{
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t arg[4] = {0, 0, 0, 0};
    const bool nb_ok = q < 15;  // lane + 1 holds the next run of the same tile row
    const uint64_t HW = (uint64_t)p.H * p.W;
    for (uint32_t c = 0; c < p.classes; ++c) {
        const float *r0 = v + oy0 + c, *r1 = v + oy1 + c;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float top = b0[e] * r0[ox0[e]] + b1[e] * r0[ox1[e]];
            const float bot = b0[e] * r1[ox0[e]] + b1[e] * r1[ox1[e]];
            o[e] = a0 * top + a1 * bot;
            if (LABELS) {
                if (c == 0) best[e] = o[e];
                else if (o[e] > best[e]) best[e] = o[e], arg[e] = c;
            }
        }
        if (SCORES) {
            float *row = p.scores + (img * p.classes + c) * HW + (uint64_t)Y * p.W;  // (c, Y, 0)
            const uint32_t s = (0u - (uint32_t)(reinterpret_cast<uintptr_t>(row + X0) >> 2)) & 3;  // floats to the aligned quad
            const float n0 = __shfl_down(o[0], 1), n1 = __shfl_down(o[1], 1), n2 = __shfl_down(o[2], 1);
            if (row_ok) {
                if (s == 0) {
                    if (X0 + 3 < Xend) {
                        *reinterpret_cast<float4 *>(row + X0) = make_float4(o[0], o[1], o[2], o[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (X0 + e < Xend) row[X0 + e] = o[e];
                    }
                } else {
                    const bool prev_full = q > 0 && X0 + s - 1 < Xend;  // the previous lane's quad ends at X0 + s - 1
                    const bool full = nb_ok && X0 + s + 3 < Xend;
#pragma unroll
                    for (int e = 0; e < 3; ++e)
                        if (!prev_full && (uint32_t)e < s && X0 + e < Xend) row[X0 + e] = o[e];
                    if (full) {
                        float4 t;
                        if (s == 1) t = make_float4(o[1], o[2], o[3], n0);
                        else if (s == 2) t = make_float4(o[2], o[3], n0, n1);
                        else t = make_float4(o[3], n0, n1, n2);
                        *reinterpret_cast<float4 *>(row + X0 + s) = t;
                    } else {
#pragma unroll
                        for (int e = 1; e < 4; ++e)
                            if ((uint32_t)e >= s && X0 + e < Xend) row[X0 + e] = o[e];
                    }
                }
            }
        }
    }
    if (LABELS) {
        uint8_t *row = p.labels + img * HW + (uint64_t)Y * p.W;
        const uint32_t s = (0u - (uint32_t)reinterpret_cast<uintptr_t>(row + X0)) & 3;  // bytes to the aligned word
        const uint32_t mine = arg[0] | arg[1] << 8 | arg[2] << 16 | arg[3] << 24;
        const uint32_t next = __shfl_down(mine, 1);
        if (row_ok) {
            const bool prev_full = q > 0 && X0 + s - 1 < Xend;
            const bool full = (s == 0 || nb_ok) && X0 + s + 3 < Xend;
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (!prev_full && (uint32_t)e < s && X0 + e < Xend) row[X0 + e] = (uint8_t)arg[e];
            if (full) {
                const uint64_t both = (uint64_t)next << 32 | mine;
                *reinterpret_cast<uint32_t *>(row + X0 + s) = (uint32_t)(both >> (8 * s));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((uint32_t)e >= s && X0 + e < Xend) row[X0 + e] = (uint8_t)arg[e];
            }
        }
    }
}

template <bool SCORES, bool LABELS>
__global__ __launch_bounds__(256) void upsample_bilinear_kernel(const seg_args p)
{
    extern __shared__ float tile[];  // [rows][cols][classes | 1] of the tile's source pixels
    const uint32_t q = threadIdx.x & 15, r = threadIdx.x >> 4;
    const uint32_t by = blockIdx.x / p.tiles_x, bx = blockIdx.x - by * p.tiles_x;
    const uint64_t img = blockIdx.y;
    const uint32_t Xt = bx * kSegTX, Yt = by * kSegTY;
    const uint32_t Xend = p.W - Xt < (uint32_t)kSegTX ? p.W : Xt + kSegTX;
    const uint32_t Yend = p.H - Yt < (uint32_t)kSegTY ? p.H : Yt + kSegTY;
    // the tile's footprint in the source: the coordinate is monotonic in the output index
    uint32_t ys, ye, xs, xe, u;
    float f;
    seg_coord(Yt, p.scale_h, p.h, &ys, &u, &f);
    seg_coord(Yend - 1, p.scale_h, p.h, &u, &ye, &f);
    seg_coord(Xt, p.scale_w, p.w, &xs, &u, &f);
    seg_coord(Xend - 1, p.scale_w, p.w, &u, &xe, &f);
    const uint32_t nr = ye - ys + 1, nc = xe - xs + 1, pitch = p.classes | 1;
    const bool staged = (uint64_t)nr * nc * pitch <= (uint64_t)p.lds_floats;  // the same for the whole block
    const float *image = p.src + img * p.h * p.w * p.cs;
    if (staged) {
        const uint32_t c4 = (p.classes + 3) / 4, items = nr * nc * c4;  // 4 * c4 <= cs: cs % 4 == 0, cs >= classes
        for (uint32_t i = threadIdx.x; i < items; i += 256) {
            const uint32_t pix = i / c4, k = i - pix * c4, pr = pix / nc, pc = pix - pr * nc;
            const float4 t = *reinterpret_cast<const float4 *>(image + ((uint64_t)(ys + pr) * p.w + xs + pc) * p.cs + 4 * k);
            const float e[4] = {t.x, t.y, t.z, t.w};
            float *d = tile + pix * pitch + 4 * k;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * k + j < p.classes) d[j] = e[j];
        }
        __syncthreads();
    }
    // rows and columns past the image repeat its last ones: every lane computes (the shuffles want all of them)
    // and reads inside the footprint; their stores are dropped
    const uint32_t Y = Yt + r, X0 = Xt + 4 * q;
    const bool row_ok = Y < Yend;
    uint32_t y0, y1, x0[4], x1[4];
    float a0, a1, b0[4], b1[4];
    seg_coord(row_ok ? Y : Yend - 1, p.scale_h, p.h, &y0, &y1, &a1);
    a0 = 1.0f - a1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        seg_coord(X0 + e < Xend ? X0 + e : Xend - 1, p.scale_w, p.w, &x0[e], &x1[e], &b1[e]);
        b0[e] = 1.0f - b1[e];
    }
    if (staged) {
        const uint32_t rs = nc * pitch;  // floats from a row of the tile to the next
        uint32_t ox0[4], ox1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ox0[e] = (x0[e] - xs) * pitch, ox1[e] = (x1[e] - xs) * pitch;
        seg_walk<SCORES, LABELS, uint32_t>(p, tile, (y0 - ys) * rs, (y1 - ys) * rs, a0, a1, ox0, ox1, b0, b1, img, Y,
                                           row_ok, X0, Xend, q);
    } else {
        const uint64_t rs = (uint64_t)p.w * p.cs;
        uint64_t ox0[4], ox1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ox0[e] = (uint64_t)x0[e] * p.cs, ox1[e] = (uint64_t)x1[e] * p.cs;
        seg_walk<SCORES, LABELS, uint64_t>(p, image, y0 * rs, y1 * rs, a0, a1, ox0, ox1, b0, b1, img, Y, row_ok, X0, Xend,
                                           q);
    }
}

// source rows (columns) a tile of `t` outputs can touch at this scale, with room for the rounding of the coordinate;
// an estimate only: the kernel measures its footprint and stages it when it fits what the launch was given
uint64_t seg_span(float scale, uint64_t t, uint64_t n_in)
{
    const uint64_t s = (uint64_t)(scale * (float)(t - 1)) + 3;
    return s < n_in ? s : n_in;
}

// ---- the channel concat -----------------------------------------------------------------------------------
// A copy, bound by HBM: one thread moves one 16-byte chunk per trip, consecutive threads consecutive chunks of
// the destination, so a wave stores 1 KiB in a row and loads runs of a source's pixel (the 256 fp32 channels of
// an ASPP branch are one such KiB).  256 threads, no LDS, a dozen registers: every CU holds its eight blocks,
// and the grid is at most the 2048 blocks that fill the chip (rn_stream_grid); a thread then strides on.  A
// chunk is (pixel, chunk k of the destination pixel); the stride is a fixed (pixels, chunks) pair, so a trip adds
// it with one carry: no division in the loop but the image of a broadcast chunk, and 64-bit offsets only where an
// address is formed (B * pixels * channels passes 2^31; B * pixels and the chunks of a pixel do not).
struct concat_args {
    const uint4 *src[8];
    const uint4 *per_image;
    uint4 *dst;
    uint32_t end[8];  // chunk of a destination pixel where source i ends (sources past n_src: where the last ends)
    uint32_t cpp, pc;  // chunks of a destination pixel, of them the broadcast's (the last ones)
    uint32_t pixels, total_pix;
    uint32_t mul_cpp, shr_cpp, mul_px, shr_px;
    uint32_t step_pix, step_k;  // the grid's threads as (pixels, chunks)
};

__global__ __launch_bounds__(256) void concat_channels_kernel(const concat_args p)
{
    const uint32_t gid = blockIdx.x * 256 + threadIdx.x;  // < 2^19
    uint32_t pix = rn_gemm::fast_div(gid, (int)p.cpp, p.mul_cpp, p.shr_cpp), k = gid - pix * p.cpp;
    while (pix < p.total_pix) {
        const uint4 *from = nullptr;
        uint32_t lo = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (k >= lo && k < p.end[j]) from = p.src[j] + ((uint64_t)pix * (p.end[j] - lo) + (k - lo));
            lo = p.end[j];
        }
        if (!from) {  // the broadcast: image pix / pixels
            const uint32_t b = rn_gemm::fast_div(pix, (int)p.pixels, p.mul_px, p.shr_px);
            from = p.per_image + ((uint64_t)b * p.pc + (k - lo));
        }
        p.dst[(uint64_t)pix * p.cpp + k] = *from;
        pix += p.step_pix, k += p.step_k;
        if (k >= p.cpp) k -= p.cpp, ++pix;
    }
}

bool seg_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace

struct rn_seg_head {
    rn_ctx *ctx;
    uint64_t cin, mid, classes;
    // what the two convolutions run with: mid rounded up to a multiple of 64 (the bf16 contraction's K granule; the
    // added channels have zero weights, scale 0 and shift 0, so they hold ReLU(0) = 0 and meet zero columns of the
    // 1x1 panel: exact zeros added to every sum) and classes rounded up to a multiple of 4 (16-byte coarse pixels)
    uint64_t midp, cpad;
    int dtype, finalized;
    float *raw[7];     // the state dict's tensors on the device, fp32, padded to midp / cpad
    int is_set[7];
    void *packed1, *packed2;
    float *scale, *shift;
    void *mid_t;       // [cap, h, w, mid] of the storage type
    float *coarse;     // [cap, h, w, cpad] fp32
    uint64_t cap_pix;  // pixels (images x h x w) the two scratch tensors hold
    struct seg_deeplab *dl;  // NULL: the FCN kind, everything above; else the DeepLab kind, which uses of the above
                             // ctx, cin, classes, cpad, dtype, finalized, coarse and cap_pix
};

// The DeepLab kind: torchvision's DeepLabHead(in, classes) = ASPP(in, rates, a) + Conv3x3(a, a) + BN + ReLU +
// Conv1x1(a, classes).  n + 4 convolutions with a batch-norm ("units": 0 the 1x1 branch, 1..n the dilated 3x3
// branches, n + 1 the pooled branch's 1x1, n + 2 the projection, n + 3 the 3x3) and the classifier.
constexpr int kDlMaxRates = 4, kDlMaxUnits = kDlMaxRates + 4, kDlMaxTensors = 5 * kDlMaxUnits + 2;

struct seg_tensor {
    char key[64];
    uint64_t numel, padded;  // elements of the state dict's tensor, and of its device copy (classifier rows: cpad)
    float *raw;
    int is_set;
};

struct seg_unit {
    uint64_t cin, k, dilation;
    void *packed;
    void *center;       // dilated branches: the centre tap weight[:, :, 1, 1] packed as a 1x1 panel
    float *raw_center;  // its fp32 [a, cin] source until finalize
    float *scale, *shift;
};

struct seg_deeplab {
    uint64_t a, n, rates[kDlMaxRates];
    int center_tap;  // rn_seg_head_set_center_tap
    int n_units, n_tensors;
    seg_unit unit[kDlMaxUnits];
    seg_tensor tensor[kDlMaxTensors];  // unit u: 5u + {weight, bn weight, bn bias, running_mean, running_var}; then
                                       // the classifier's weight and bias
    void *packed_cls;
    // scratch: per coarse pixel the n + 1 branch tensors [cap_pix, a] each, the concat [cap_pix, (n + 2) a]; per image
    // the pooled map [cap_img, cin] and the pooled branch [cap_img, a].  The projected tensor and the 3x3's output
    // live in branch 0's and branch 1's tensors, which are dead behind the concat.
    void *branch[kDlMaxRates + 1], *cat, *pool_in, *pool_out;
    uint64_t cap_img;
};

namespace {

const char *const kSegKeys[7] = {"classifier.0.weight",       "classifier.1.weight",      "classifier.1.bias",
                                 "classifier.1.running_mean", "classifier.1.running_var", "classifier.4.weight",
                                 "classifier.4.bias"};

uint64_t seg_key_numel(const rn_seg_head *hd, int i)
{
    if (i == 0) return hd->mid * hd->cin * 9;
    if (i <= 4) return hd->mid;
    return i == 5 ? hd->classes * hd->mid : hd->classes;
}

uint64_t seg_elem(const rn_seg_head *hd) { return hd->dtype == RN_DTYPE_BF16 ? 2 : 4; }

// ---- the DeepLab kind ----
const char *const kDlBranchOps[kDlMaxRates + 1] = {"aspp_conv0", "aspp_conv1", "aspp_conv2", "aspp_conv3", "aspp_conv4"};

// Whether dilated branch u of a forward on an h x w map runs as the 1x1 contraction on its centre tap.  With
// rate >= h and rate >= w every other tap of every output pixel lies outside the image, so the 3x3 sums the centre
// tap's products in channel order among zeros, and so does the 1x1 -- the same bits as long as both routes round
// that sum at the same places.  bf16 tensors: every candidate of both adds one K tile after the other into one
// accumulator; the plan holds for every width.  fp32 tensors: a contraction of 32 or more K tiles (K >= 1024)
// folds its sum in eight chunks whose ends are multiples of 2 * ceil(K tiles / 16) (choose_four_wave and
// split_chunked_tail of rn_conv.hip).  The 3x3 has nine times the K tiles of the 1x1, so from in_channels = 128 on
// its chunk ends cut the centre tap's range elsewhere than the 1x1 does (in = 128: tiles 16..19 of 36 fold at 18, the
// 1x1's four tiles not at all; in = 2048: tiles 256..319 of 576 fold once, at 288, the 1x1's 64 tiles at every
// eighth): the same products, added in another association.  Only in = 64 (18 and 2 tiles, neither chunked) keeps
// the bits in fp32, and only there does an fp32 head take the plan ("DeepLabV3 head").
bool dl_center_route(const rn_seg_head *hd, int u, uint64_t h, uint64_t w)
{
    const seg_deeplab *dl = hd->dl;
    if (!dl->center_tap || u < 1 || (uint64_t)u > dl->n) return false;
    if (dl->unit[u].dilation < h || dl->unit[u].dilation < w) return false;
    return hd->dtype == RN_DTYPE_BF16 || 9 * hd->cin / 32 < 32;
}

void dl_free(rn_ctx *ctx, void **p)
{
    if (*p) rn_free(ctx, *p);
    *p = NULL;
}

void dl_free_scratch(rn_seg_head *hd)
{
    seg_deeplab *dl = hd->dl;
    for (uint64_t i = 0; i <= dl->n; ++i) dl_free(hd->ctx, &dl->branch[i]);
    dl_free(hd->ctx, &dl->cat), dl_free(hd->ctx, &dl->pool_in), dl_free(hd->ctx, &dl->pool_out);
    dl_free(hd->ctx, (void **)&hd->coarse);
    hd->cap_pix = dl->cap_img = 0;
}

int dl_set_tensor(rn_seg_head *hd, const char *key, const float *host_data, uint64_t numel)
{
    rn_ctx *ctx = hd->ctx;
    seg_deeplab *dl = hd->dl;
    int i = 0;
    while (i < dl->n_tensors && strcmp(key, dl->tensor[i].key) != 0) ++i;
    if (i == dl->n_tensors) return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head_set_tensor: unknown key '%s'", key);
    seg_tensor *t = &dl->tensor[i];
    if (numel != t->numel)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head_set_tensor: %s has %llu elements, not %llu", key,
                            (unsigned long long)t->numel, (unsigned long long)numel);
    // only the classifier is padded (classes -> cpad rows of zeros: its weight and its bias)
    float *padded = (float *)calloc(t->padded, sizeof(float));
    if (!padded) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_seg_head_set_tensor: out of host memory");
    memcpy(padded, host_data, numel * sizeof(float));
    int st = t->raw ? RN_OK : rn_malloc(ctx, (void **)&t->raw, t->padded * sizeof(float));
    if (st == RN_OK) st = rn_ctx_upload_sync(ctx, t->raw, padded, t->padded * sizeof(float));
    free(padded);
    RN_TRY(st);
    const int u = i / 5;
    if (i % 5 == 0 && u >= 1 && (uint64_t)u <= dl->n) {  // a dilated branch's weight [a, in, 3, 3]: its centre tap too
        seg_unit *un = &dl->unit[u];
        const uint64_t rows = dl->a * un->cin;
        float *center = (float *)malloc(rows * sizeof(float));
        if (!center) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_seg_head_set_tensor: out of host memory");
        for (uint64_t r = 0; r < rows; ++r) center[r] = host_data[r * 9 + 4];
        st = un->raw_center ? RN_OK : rn_malloc(ctx, (void **)&un->raw_center, rows * sizeof(float));
        if (st == RN_OK) st = rn_ctx_upload_sync(ctx, un->raw_center, center, rows * sizeof(float));
        free(center);
        RN_TRY(st);
    }
    t->is_set = 1;
    return RN_OK;
}

int dl_finalize(rn_seg_head *hd)
{
    rn_ctx *ctx = hd->ctx;
    seg_deeplab *dl = hd->dl;
    for (int i = 0; i < dl->n_tensors; ++i)
        if (!dl->tensor[i].is_set)
            return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head_finalize: %s is not set", dl->tensor[i].key);
    const uint64_t es = seg_elem(hd);
    for (int u = 0; u < dl->n_units; ++u) {
        seg_unit *un = &dl->unit[u];
        seg_tensor *t = &dl->tensor[5 * u];
        RN_TRY(rn_malloc(ctx, (void **)&un->scale, dl->a * sizeof(float)));
        RN_TRY(rn_malloc(ctx, (void **)&un->shift, dl->a * sizeof(float)));
        RN_TRY(rn_malloc(ctx, &un->packed, rn_conv2d_packed_weight_numel_dt(hd->dtype, un->cin, dl->a, un->k) * es));
        RN_TRY(rn_batchnorm2d_fold(ctx, t[1].raw, t[2].raw, t[3].raw, t[4].raw, un->scale, un->shift, dl->a));
        RN_TRY(rn_conv2d_pack_weight_dt(ctx, hd->dtype, t[0].raw, un->packed, un->cin, dl->a, un->k));
        if (un->raw_center) {
            RN_TRY(rn_malloc(ctx, &un->center, rn_conv2d_packed_weight_numel_dt(hd->dtype, un->cin, dl->a, 1) * es));
            RN_TRY(rn_conv2d_pack_weight_dt(ctx, hd->dtype, un->raw_center, un->center, un->cin, dl->a, 1));
        }
    }
    seg_tensor *cls = &dl->tensor[5 * dl->n_units];
    RN_TRY(rn_malloc(ctx, &dl->packed_cls, rn_conv2d_packed_weight_numel_dt(hd->dtype, dl->a, hd->cpad, 1) * es));
    RN_TRY(rn_conv2d_pack_weight_dt(ctx, hd->dtype, cls->raw, dl->packed_cls, dl->a, hd->cpad, 1));
    RN_TRY(rn_sync(ctx));
    for (int i = 0; i < dl->n_tensors - 1; ++i) dl_free(ctx, (void **)&dl->tensor[i].raw);  // the bias stays: a shift
    for (int u = 0; u < dl->n_units; ++u) dl_free(ctx, (void **)&dl->unit[u].raw_center);
    hd->finalized = 1;
    return RN_OK;
}

// launch `step` of a DeepLab forward (the order of rn_hip.h): B images whose scratch starts img0 images into the
// head's tensors
int dl_step(rn_seg_head *hd, rn_ctx *ctx, int step, const void *x, uint64_t img0, uint64_t B, uint64_t h, uint64_t w,
            uint64_t H, uint64_t W, float *scores_nchw, uint8_t *labels)
{
    seg_deeplab *dl = hd->dl;
    const uint64_t es = seg_elem(hd), n = dl->n, a = dl->a, pix0 = img0 * h * w;
    const int dt = hd->dtype;
    void *br[kDlMaxRates + 1];
    for (uint64_t i = 0; i <= n; ++i) br[i] = (char *)dl->branch[i] + pix0 * a * es;
    void *cat = (char *)dl->cat + pix0 * (n + 2) * a * es;
    void *pool_in = (char *)dl->pool_in + img0 * hd->cin * es, *pool_out = (char *)dl->pool_out + img0 * a * es;
    void *proj = br[0], *mid = br[1];
    float *coarse = hd->coarse + pix0 * hd->cpad;
    rn_epilogue ep;
    ep.residual = NULL;
    if (pix0 + B * h * w > hd->cap_pix || img0 + B > dl->cap_img)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head: scratch not reserved");
    const uint64_t s = (uint64_t)step;
    if (s <= n) {  // the branches
        const seg_unit *un = &dl->unit[s];
        ep.scale = un->scale, ep.shift = un->shift, ep.relu = 1;
        if (s == 0 || dl_center_route(hd, (int)s, h, w))
            return rn_conv2d_nhwc_forward_dt(ctx, dt, dt, x, br[s], s == 0 ? un->packed : un->center, 1, 1, 0, h, w, B,
                                             hd->cin, a, h, w, &ep);
        return rn_conv2d_dilated_nhwc_forward_dt(ctx, dt, dt, x, br[s], un->packed, 3, 1, un->dilation, un->dilation, h,
                                                 w, B, hd->cin, a, h, w, 1, &ep);
    }
    if (s == n + 1) return rn_global_avgpool_nhwc_forward_dt(ctx, dt, x, pool_in, B, hd->cin, h, w);
    if (s == n + 2) {  // the pooled branch: B "pixels"
        const seg_unit *un = &dl->unit[n + 1];
        ep.scale = un->scale, ep.shift = un->shift, ep.relu = 1;
        return rn_conv2d_nhwc_forward_dt(ctx, dt, dt, pool_in, pool_out, un->packed, 1, 1, 0, 1, 1, B, hd->cin, a, 1, 1,
                                         &ep);
    }
    if (s == n + 3) {
        uint64_t ch[kDlMaxRates + 1];
        for (uint64_t i = 0; i <= n; ++i) ch[i] = a;
        return rn_concat_channels_forward_dt(ctx, dt, n + 1, br, ch, pool_out, a, cat, B, h * w);
    }
    if (s == n + 4 || s == n + 5) {
        const seg_unit *un = &dl->unit[s - 2];
        const uint64_t k = un->k;
        ep.scale = un->scale, ep.shift = un->shift, ep.relu = 1;
        return rn_conv2d_nhwc_forward_dt(ctx, dt, dt, s == n + 4 ? cat : proj, s == n + 4 ? proj : mid, un->packed, k, 1,
                                         k / 2, h, w, B, un->cin, a, h, w, &ep);
    }
    if (s == n + 6) {
        ep.scale = NULL, ep.shift = dl->tensor[dl->n_tensors - 1].raw, ep.relu = 0;
        return rn_conv2d_nhwc_forward_dt(ctx, dt, RN_DTYPE_F32, mid, coarse, dl->packed_cls, 1, 1, 0, h, w, B, a, hd->cpad,
                                         h, w, &ep);
    }
    return rn_upsample_bilinear_forward(ctx, coarse, B, h, w, hd->classes, hd->cpad, H, W, scores_nchw, labels);
}

}  // namespace

extern "C" {

int rn_upsample_bilinear_forward(rn_ctx *ctx, const float *src_nhwc, uint64_t B, uint64_t h, uint64_t w,
                                 uint64_t classes, uint64_t src_channels, uint64_t H, uint64_t W, float *scores_nchw,
                                 uint8_t *labels)
{
    RN_ENTER(ctx);
    if (B == 0) return RN_OK;
    RN_REQUIRE(ctx, src_nhwc, "src_nhwc is NULL");
    RN_REQUIRE(ctx, scores_nchw || labels, "both outputs (scores_nchw, labels) are NULL");
    RN_REQUIRE(ctx, classes >= 1 && classes <= 256, "classes must be 1..256");
    RN_REQUIRE(ctx, src_channels >= classes && src_channels <= 256 && src_channels % 4 == 0,
               "src_channels must be a multiple of 4, >= classes and <= 256");
    RN_REQUIRE(ctx, h >= 1 && w >= 1 && H >= 1 && W >= 1, "h, w, H, W must be >= 1");
    RN_REQUIRE(ctx, h < (1ull << 31) && w < (1ull << 31) && h * w < (1ull << 31) && H < (1ull << 31) &&
                        W < (1ull << 31) && H * W < (1ull << 31),
               "h * w and H * W must be below 2^31");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(src_nhwc) & 15) == 0, "src_nhwc must be 16-byte aligned");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(scores_nchw) & 3) == 0, "scores_nchw must be 4-byte aligned");
    seg_args p;
    p.h = (uint32_t)h, p.w = (uint32_t)w, p.classes = (uint32_t)classes, p.cs = (uint32_t)src_channels;
    p.H = (uint32_t)H, p.W = (uint32_t)W;
    p.scale_h = (float)h / (float)H, p.scale_w = (float)w / (float)W;
    const uint64_t tx = rn_ceil_div(W, kSegTX), ty = rn_ceil_div(H, kSegTY);
    p.tiles_x = (uint32_t)tx;
    const uint64_t want = seg_span(p.scale_h, kSegTY, h) * seg_span(p.scale_w, kSegTX, w) * (classes | 1) * sizeof(float);
    const uint32_t lds = want <= kSegLdsCap ? (uint32_t)want : 0;  // 0: every tile reads global memory
    p.lds_floats = lds / 4;
    // gridDim.y is limited to 65535: walk the batch in slabs
    for (uint64_t b0 = 0; b0 < B; b0 += 65535) {
        const uint64_t nb = (B - b0) < 65535 ? (B - b0) : 65535;
        const dim3 grid((unsigned)(tx * ty), (unsigned)nb);
        p.src = src_nhwc + b0 * h * w * src_channels;
        p.scores = scores_nchw ? scores_nchw + b0 * classes * H * W : NULL;
        p.labels = labels ? labels + b0 * H * W : NULL;
        if (scores_nchw && labels)
            upsample_bilinear_kernel<true, true><<<grid, 256, lds, ctx->stream>>>(p);
        else if (scores_nchw)
            upsample_bilinear_kernel<true, false><<<grid, 256, lds, ctx->stream>>>(p);
        else
            upsample_bilinear_kernel<false, true><<<grid, 256, lds, ctx->stream>>>(p);
    }
    return rn_after_launch(ctx, "rn_upsample_bilinear_forward");
}

int rn_concat_channels_forward_dt(rn_ctx *ctx, int dtype, uint64_t n_src, const void *const *srcs,
                                  const uint64_t *channels, const void *per_image, uint64_t per_image_channels, void *dst,
                                  uint64_t B, uint64_t pixels)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, dtype == RN_DTYPE_F32 || dtype == RN_DTYPE_BF16, "unknown dtype");
    RN_REQUIRE(ctx, n_src >= 1 && n_src <= 8, "n_src must be 1..8");
    RN_REQUIRE(ctx, srcs && channels && dst, "srcs, channels or dst is NULL");
    RN_REQUIRE(ctx, (per_image != NULL) == (per_image_channels != 0),
               "per_image and per_image_channels: a pointer with channels, or NULL with 0");
    RN_REQUIRE(ctx, B < (1ull << 31) && pixels < (1ull << 31) && B * pixels < (1ull << 31), "B * pixels must be below 2^31");
    const uint64_t es = dtype == RN_DTYPE_BF16 ? 2 : 4, per = 16 / es;  // elements of a 16-byte chunk
    concat_args p{};
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_src; ++i) {
        RN_REQUIRE(ctx, srcs[i], "a source is NULL");
        RN_REQUIRE(ctx, channels[i] >= 1 && channels[i] < (1ull << 31), "a channel count is 0 (or 2^31 and above)");
        RN_REQUIRE(ctx, channels[i] % per == 0, "a source's channels are no multiple of 16 bytes");
        RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(srcs[i]) & 15) == 0, "a source is off a 16-byte boundary");
        total += channels[i];
        p.src[i] = (const uint4 *)srcs[i];
        p.end[i] = (uint32_t)(total / per);
    }
    RN_REQUIRE(ctx, per_image_channels % per == 0 && per_image_channels < (1ull << 31),
               "per_image_channels is no multiple of 16 bytes");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(per_image) & 15) == 0, "per_image is off a 16-byte boundary");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(dst) & 15) == 0, "dst is off a 16-byte boundary");
    total += per_image_channels;
    RN_REQUIRE(ctx, total / per < (1ull << 31), "a destination pixel must be below 2^31 chunks of 16 bytes");
    if (B == 0 || pixels == 0) return RN_OK;
    const uint64_t npix = B * pixels, dst_bytes = npix * total * es;
    for (uint64_t i = 0; i < n_src; ++i)
        RN_REQUIRE(ctx, !seg_overlap(dst, dst_bytes, srcs[i], npix * channels[i] * es), "dst overlaps a source");
    RN_REQUIRE(ctx, !per_image || !seg_overlap(dst, dst_bytes, per_image, B * per_image_channels * es),
               "dst overlaps per_image");
    for (uint64_t i = n_src; i < 8; ++i) p.end[i] = p.end[n_src - 1];
    p.per_image = (const uint4 *)per_image, p.dst = (uint4 *)dst;
    p.cpp = (uint32_t)(total / per), p.pc = (uint32_t)(per_image_channels / per);
    p.pixels = (uint32_t)pixels, p.total_pix = (uint32_t)npix;
    rn_fast_div(p.cpp, &p.mul_cpp, &p.shr_cpp);
    rn_fast_div(p.pixels, &p.mul_px, &p.shr_px);
    const unsigned grid = rn_stream_grid(npix * p.cpp, 256);
    p.step_pix = (uint32_t)((uint64_t)grid * 256 / p.cpp), p.step_k = (uint32_t)((uint64_t)grid * 256 % p.cpp);
    concat_channels_kernel<<<grid, 256, 0, ctx->stream>>>(p);
    return rn_after_launch(ctx, "rn_concat_channels_forward_dt");
}

// ---- the head ---------------------------------------------------------------------------------------------

int rn_seg_head_create(rn_ctx *ctx, rn_seg_head **out, uint64_t in_channels, uint64_t mid_channels, uint64_t classes)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    RN_REQUIRE(ctx, in_channels >= 64 && in_channels % 64 == 0 && in_channels <= 8192,
               "in_channels must be a multiple of 64 (at most 8192)");
    RN_REQUIRE(ctx, mid_channels >= 1 && mid_channels <= 8192, "mid_channels must be 1..8192");
    RN_REQUIRE(ctx, classes >= 1 && classes <= 256, "classes must be 1..256");
    rn_seg_head *hd = (rn_seg_head *)calloc(1, sizeof(*hd));
    if (!hd) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_seg_head_create: out of host memory");
    hd->ctx = ctx;
    hd->cin = in_channels, hd->mid = mid_channels, hd->classes = classes;
    hd->midp = (mid_channels + 63) / 64 * 64, hd->cpad = (classes + 3) / 4 * 4;
    hd->dtype = RN_DTYPE_F32;
    *out = hd;
    return RN_OK;
}

int rn_seg_head_create_deeplab(rn_ctx *ctx, rn_seg_head **out, uint64_t in_channels, uint64_t aspp_channels,
                               uint64_t classes, uint64_t n_rates, const uint64_t *rates)
{
    static const char *const bn[4] = {"weight", "bias", "running_mean", "running_var"};
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    RN_REQUIRE(ctx, in_channels >= 64 && in_channels % 64 == 0 && in_channels <= 8192,
               "in_channels must be a multiple of 64 (at most 8192)");
    RN_REQUIRE(ctx, aspp_channels >= 64 && aspp_channels % 64 == 0 && aspp_channels <= 1024,
               "aspp_channels must be a multiple of 64 (at most 1024)");
    RN_REQUIRE(ctx, classes >= 1 && classes <= 256, "classes must be 1..256");
    RN_REQUIRE(ctx, n_rates >= 1 && n_rates <= (uint64_t)kDlMaxRates && rates, "n_rates must be 1..4 (and rates not NULL)");
    for (uint64_t i = 0; i < n_rates; ++i)
        RN_REQUIRE(ctx, rates[i] >= 1 && rates[i] <= RN_CONV_MAX_DILATION, "a rate must be 1..RN_CONV_MAX_DILATION");
    rn_seg_head *hd = (rn_seg_head *)calloc(1, sizeof(*hd));
    seg_deeplab *dl = (seg_deeplab *)calloc(1, sizeof(*dl));
    if (!hd || !dl) {
        free(hd), free(dl);
        return rn_set_error(ctx, RN_ERR_NOMEM, "rn_seg_head_create_deeplab: out of host memory");
    }
    hd->ctx = ctx, hd->dl = dl;
    hd->cin = in_channels, hd->classes = classes, hd->cpad = (classes + 3) / 4 * 4;
    hd->mid = hd->midp = aspp_channels;
    hd->dtype = RN_DTYPE_F32;
    const uint64_t n = n_rates, a = aspp_channels;
    dl->a = a, dl->n = n, dl->center_tap = 1;
    dl->n_units = (int)n + 4, dl->n_tensors = 5 * dl->n_units + 2;
    for (int u = 0; u < dl->n_units; ++u) {
        seg_unit *un = &dl->unit[u];
        seg_tensor *t = &dl->tensor[5 * u];
        char conv[48], norm[48];
        const uint64_t v = (uint64_t)u;
        un->cin = v <= n + 1 ? in_channels : v == n + 2 ? (n + 2) * a : a;
        un->k = (v >= 1 && v <= n) || v == n + 3 ? 3 : 1;
        un->dilation = v >= 1 && v <= n ? rates[v - 1] : 1;
        if (v >= 1 && v <= n) dl->rates[v - 1] = rates[v - 1];
        // the pooled branch's Sequential starts with the pool: its convolution is .1, its batch-norm .2
        if (v <= n + 1) {
            snprintf(conv, sizeof(conv), "classifier.0.convs.%d.%d", u, v <= n ? 0 : 1);
            snprintf(norm, sizeof(norm), "classifier.0.convs.%d.%d", u, v <= n ? 1 : 2);
        } else {
            snprintf(conv, sizeof(conv), "%s", v == n + 2 ? "classifier.0.project.0" : "classifier.1");
            snprintf(norm, sizeof(norm), "%s", v == n + 2 ? "classifier.0.project.1" : "classifier.2");
        }
        snprintf(t[0].key, sizeof(t[0].key), "%s.weight", conv);
        t[0].numel = t[0].padded = a * un->cin * un->k * un->k;
        for (int j = 0; j < 4; ++j) {
            snprintf(t[1 + j].key, sizeof(t[1 + j].key), "%s.%s", norm, bn[j]);
            t[1 + j].numel = t[1 + j].padded = a;
        }
    }
    seg_tensor *cls = &dl->tensor[5 * dl->n_units];
    snprintf(cls[0].key, sizeof(cls[0].key), "classifier.4.weight");
    snprintf(cls[1].key, sizeof(cls[1].key), "classifier.4.bias");
    cls[0].numel = classes * a, cls[0].padded = hd->cpad * a;
    cls[1].numel = classes, cls[1].padded = hd->cpad;
    *out = hd;
    return RN_OK;
}

int rn_seg_head_set_center_tap(rn_seg_head *hd, int on)
{
    if (!hd) return RN_ERR_INVALID;
    RN_REQUIRE(hd->ctx, hd->dl, "not a DeepLab head");
    RN_REQUIRE(hd->ctx, on == 0 || on == 1, "on must be 0 or 1");
    hd->dl->center_tap = on;
    return RN_OK;
}

int rn_seg_head_set_dtype(rn_seg_head *hd, int dtype)
{
    if (!hd) return RN_ERR_INVALID;
    RN_REQUIRE(hd->ctx, !hd->finalized, "the head is finalized");
    RN_REQUIRE(hd->ctx, dtype == RN_DTYPE_F32 || dtype == RN_DTYPE_BF16, "unknown dtype");
    hd->dtype = dtype;
    return RN_OK;
}

int rn_seg_head_set_tensor(rn_seg_head *hd, const char *key, const float *host_data, uint64_t numel)
{
    if (!hd) return RN_ERR_INVALID;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, key && host_data, "key or host_data is NULL");
    RN_REQUIRE(ctx, !hd->finalized, "the head is finalized");
    if (hd->dl) return dl_set_tensor(hd, key, host_data, numel);
    int i = 0;
    while (i < 7 && strcmp(key, kSegKeys[i]) != 0) ++i;
    if (i == 7) return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head_set_tensor: unknown key '%s'", key);
    if (numel != seg_key_numel(hd, i))
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head_set_tensor: %s has %llu elements, not %llu", key,
                            (unsigned long long)seg_key_numel(hd, i), (unsigned long long)numel);
    // padded on the host: rows of `len` values become rows of `pitch`, `rows` rows become `prows`; everything added
    // is zero but the running variance of an added mid channel (1: scale = 0 / sqrt(1 + eps) = 0, shift = 0)
    const uint64_t rows = i == 0 ? hd->mid : i <= 4 ? 1 : hd->classes, prows = i == 0 ? hd->midp : i <= 4 ? 1 : hd->cpad;
    const uint64_t len = i == 0 ? hd->cin * 9 : i <= 5 ? hd->mid : 1, pitch = i == 0 ? len : i <= 5 ? hd->midp : 1;
    float *padded = (float *)calloc(prows * pitch, sizeof(float));
    if (!padded) return rn_set_error(ctx, RN_ERR_NOMEM, "rn_seg_head_set_tensor: out of host memory");
    for (uint64_t r = 0; r < rows; ++r) memcpy(padded + r * pitch, host_data + r * len, len * sizeof(float));
    if (i == 4)
        for (uint64_t c = hd->mid; c < hd->midp; ++c) padded[c] = 1.0f;
    int st = hd->raw[i] ? RN_OK : rn_malloc(ctx, (void **)&hd->raw[i], prows * pitch * sizeof(float));
    if (st == RN_OK) st = rn_ctx_upload_sync(ctx, hd->raw[i], padded, prows * pitch * sizeof(float));
    free(padded);
    RN_TRY(st);
    hd->is_set[i] = 1;
    return RN_OK;
}

int rn_seg_head_finalize(rn_seg_head *hd)
{
    if (!hd) return RN_ERR_INVALID;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    if (hd->finalized) return RN_OK;
    if (hd->dl) return dl_finalize(hd);
    for (int i = 0; i < 7; ++i)
        if (!hd->is_set[i]) return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head_finalize: %s is not set", kSegKeys[i]);
    const uint64_t es = seg_elem(hd);
    RN_TRY(rn_malloc(ctx, (void **)&hd->scale, hd->midp * sizeof(float)));
    RN_TRY(rn_malloc(ctx, (void **)&hd->shift, hd->midp * sizeof(float)));
    RN_TRY(rn_malloc(ctx, &hd->packed1, rn_conv2d_packed_weight_numel_dt(hd->dtype, hd->cin, hd->midp, 3) * es));
    RN_TRY(rn_malloc(ctx, &hd->packed2, rn_conv2d_packed_weight_numel_dt(hd->dtype, hd->midp, hd->cpad, 1) * es));
    RN_TRY(rn_batchnorm2d_fold(ctx, hd->raw[1], hd->raw[2], hd->raw[3], hd->raw[4], hd->scale, hd->shift, hd->midp));
    RN_TRY(rn_conv2d_pack_weight_dt(ctx, hd->dtype, hd->raw[0], hd->packed1, hd->cin, hd->midp, 3));
    RN_TRY(rn_conv2d_pack_weight_dt(ctx, hd->dtype, hd->raw[5], hd->packed2, hd->midp, hd->cpad, 1));
    RN_TRY(rn_sync(ctx));
    for (int i = 0; i < 6; ++i) {  // the bias (raw[6]) stays: it is the 1x1 convolution's shift
        RN_TRY(rn_free(ctx, hd->raw[i]));
        hd->raw[i] = NULL;
    }
    hd->finalized = 1;
    return RN_OK;
}

int rn_seg_head_destroy(rn_seg_head *hd)
{
    if (!hd) return RN_OK;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    RN_TRY(rn_sync(ctx));
    if (hd->dl) {
        seg_deeplab *dl = hd->dl;
        dl_free_scratch(hd);
        for (int i = 0; i < dl->n_tensors; ++i) dl_free(ctx, (void **)&dl->tensor[i].raw);
        for (int u = 0; u < dl->n_units; ++u) {
            seg_unit *un = &dl->unit[u];
            dl_free(ctx, &un->packed), dl_free(ctx, &un->center), dl_free(ctx, (void **)&un->raw_center);
            dl_free(ctx, (void **)&un->scale), dl_free(ctx, (void **)&un->shift);
        }
        dl_free(ctx, &dl->packed_cls);
        free(dl);
        free(hd);
        return RN_OK;
    }
    void *bufs[6] = {hd->packed1, hd->packed2, hd->scale, hd->shift, hd->mid_t, hd->coarse};
    for (int i = 0; i < 7; ++i)
        if (hd->raw[i]) rn_free(ctx, hd->raw[i]);
    for (int i = 0; i < 6; ++i)
        if (bufs[i]) rn_free(ctx, bufs[i]);
    free(hd);
    return RN_OK;
}

// library-internal (rn_private.h): what the model driver asks of a head and queues of it
int rn_seg_head_matches(const rn_seg_head *hd, uint64_t in_channels, int dtype, const char **why)
{
    const char *w = NULL;
    if (!hd) w = "the head is NULL";
    else if (!hd->finalized) w = "the head is not finalized";
    else if (hd->cin != in_channels) w = "the head's in_channels is not the width of the model's layer4";
    else if (hd->dtype != dtype) w = "the head's storage type (dtype) is not the model's";
    if (why) *why = w;
    return w == NULL;
}

void rn_seg_head_dims(const rn_seg_head *hd, uint64_t dims[4])
{
    dims[0] = hd->cin, dims[1] = hd->midp, dims[2] = hd->classes, dims[3] = hd->cpad;
}

// launch `step` of a forward of B images on an h x w map to H x W: its profile name, FLOPs and bytes; returns the
// number of launches (3 for the FCN kind, n + 8 for the DeepLab kind); step outside 0 .. that - 1 only counts
int rn_seg_head_plan(const rn_seg_head *hd, uint64_t B, uint64_t h, uint64_t w, uint64_t H, uint64_t W, int want_scores,
                     int want_labels, int step, const char **name, double *flops, double *bytes)
{
    const double es = (double)seg_elem(hd), P = (double)(B * h * w), cin = (double)hd->cin, cpad = (double)hd->cpad;
    const double up = 4.0 * P * cpad +
                      (double)(B * H * W) * ((want_scores ? 4.0 * (double)hd->classes : 0.0) + (want_labels ? 1.0 : 0.0));
    const int count = hd->dl ? (int)hd->dl->n + 8 : 3;
    const char *nm = NULL;
    double f = 0.0, by = 0.0;
    if (step < 0 || step >= count) return count;
    if (!hd->dl) {
        const double mid = (double)hd->midp;
        if (step == 0) nm = "seg_conv1", f = 2.0 * P * 9.0 * cin * mid, by = es * (P * (cin + mid) + 9.0 * cin * mid);
        else if (step == 1) nm = "seg_conv2", f = 2.0 * P * mid * cpad, by = P * (es * mid + 4.0 * cpad) + es * (mid * cpad);
        else nm = "seg_upsample", by = up;
    } else {
        const uint64_t n = hd->dl->n, s = (uint64_t)step;
        const double a = (double)hd->dl->a, cat = (double)(n + 2) * a;
        if (s <= n) {  // the FLOPs of the route that runs
            const double taps = s == 0 || dl_center_route(hd, step, h, w) ? 1.0 : 9.0;
            nm = kDlBranchOps[s], f = 2.0 * P * taps * cin * a, by = es * (P * (cin + a) + taps * cin * a);
        } else if (s == n + 1) nm = "aspp_pool", by = es * (double)B * cin * (double)(h * w + 1);
        else if (s == n + 2) nm = "aspp_pool_conv", f = 2.0 * (double)B * cin * a, by = es * ((double)B * (cin + a) + cin * a);
        else if (s == n + 3) nm = "aspp_concat", by = es * (2.0 * P * cat - P * a + (double)B * a);
        else if (s == n + 4) nm = "aspp_project", f = 2.0 * P * cat * a, by = es * (P * (cat + a) + cat * a);
        else if (s == n + 5) nm = "seg_conv1", f = 2.0 * P * 9.0 * a * a, by = es * (P * 2.0 * a + 9.0 * a * a);
        else if (s == n + 6) nm = "seg_conv2", f = 2.0 * P * a * cpad, by = P * (es * a + 4.0 * cpad) + es * (a * cpad);
        else nm = "seg_upsample", by = up;
    }
    if (name) *name = nm;
    if (flops) *flops = f;
    if (bytes) *bytes = by;
    return count;
}

// the scratch for `images` images of `pixels` coarse pixels (h x w) each; it grows like the model's logits buffer:
// never on a stream that is being captured, never while a captured graph of the context may hold it
int rn_seg_head_reserve(rn_seg_head *hd, uint64_t images, uint64_t pixels)
{
    rn_ctx *ctx = hd->ctx;
    seg_deeplab *dl = hd->dl;
    uint64_t pix = images * pixels;
    if (pix <= hd->cap_pix && (!dl || images <= dl->cap_img)) return RN_OK;
    if (rn_ctx_is_capturing(ctx))
        return rn_set_error(ctx, RN_ERR_UNSUPPORTED, "rn_seg_head: the scratch cannot grow on a stream that is being captured");
    if (hd->cap_pix > 0 && ctx->graphs_live > 0)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head: the scratch cannot grow while a captured graph lives");
    RN_TRY(rn_sync(ctx));
    if (dl) {
        const uint64_t es = seg_elem(hd);
        if (pix < hd->cap_pix) pix = hd->cap_pix;
        if (images < dl->cap_img) images = dl->cap_img;
        dl_free_scratch(hd);
        for (uint64_t i = 0; i <= dl->n; ++i) RN_TRY(rn_malloc(ctx, &dl->branch[i], pix * dl->a * es));
        RN_TRY(rn_malloc(ctx, &dl->cat, pix * (dl->n + 2) * dl->a * es));
        RN_TRY(rn_malloc(ctx, &dl->pool_in, images * hd->cin * es));
        RN_TRY(rn_malloc(ctx, &dl->pool_out, images * dl->a * es));
        RN_TRY(rn_malloc(ctx, (void **)&hd->coarse, pix * hd->cpad * sizeof(float)));
        hd->cap_pix = pix, dl->cap_img = images;
        return RN_OK;
    }
    if (hd->mid_t) RN_TRY(rn_free(ctx, hd->mid_t));
    hd->mid_t = NULL;
    if (hd->coarse) RN_TRY(rn_free(ctx, hd->coarse));
    hd->coarse = NULL;
    hd->cap_pix = 0;
    RN_TRY(rn_malloc(ctx, &hd->mid_t, pix * hd->midp * seg_elem(hd)));
    RN_TRY(rn_malloc(ctx, (void **)&hd->coarse, pix * hd->cpad * sizeof(float)));
    hd->cap_pix = pix;
    return RN_OK;
}

// one of the head's launches on `ctx` (the head's own context, or the context of the model's stream the images
// run on): B images whose scratch starts `img0` images (img0 * h * w coarse pixels) into the head's tensors
int rn_seg_head_step(rn_seg_head *hd, rn_ctx *ctx, int step, const void *x_nhwc, uint64_t img0, uint64_t B, uint64_t h,
                     uint64_t w, uint64_t H, uint64_t W, float *scores_nchw, uint8_t *labels)
{
    if (hd->dl) return dl_step(hd, ctx, step, x_nhwc, img0, B, h, w, H, W, scores_nchw, labels);
    const uint64_t pix0 = img0 * h * w;
    void *mid = (char *)hd->mid_t + pix0 * hd->midp * seg_elem(hd);
    float *coarse = hd->coarse + pix0 * hd->cpad;
    rn_epilogue ep;
    ep.residual = NULL;
    if (pix0 + B * h * w > hd->cap_pix) return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head: scratch not reserved");
    if (step == 0) {
        ep.scale = hd->scale, ep.shift = hd->shift, ep.relu = 1;
        return rn_conv2d_nhwc_forward_dt(ctx, hd->dtype, hd->dtype, x_nhwc, mid, hd->packed1, 3, 1, 1, h, w, B, hd->cin,
                                         hd->midp, h, w, &ep);
    }
    if (step == 1) {
        ep.scale = NULL, ep.shift = hd->raw[6], ep.relu = 0;
        return rn_conv2d_nhwc_forward_dt(ctx, hd->dtype, RN_DTYPE_F32, mid, coarse, hd->packed2, 1, 1, 0, h, w, B,
                                         hd->midp, hd->cpad, h, w, &ep);
    }
    return rn_upsample_bilinear_forward(ctx, coarse, B, h, w, hd->classes, hd->cpad, H, W, scores_nchw, labels);
}

int rn_seg_head_forward(rn_seg_head *hd, const void *x_nhwc, uint64_t B, uint64_t h, uint64_t w, uint64_t H, uint64_t W,
                        float *scores_nchw, uint8_t *labels)
{
    if (!hd) return RN_ERR_INVALID;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, hd->finalized, "the head is not finalized");
    RN_REQUIRE(ctx, x_nhwc, "x_nhwc is NULL");
    RN_REQUIRE(ctx, scores_nchw || labels, "both outputs (scores_nchw, labels) are NULL");
    RN_REQUIRE(ctx, h >= 1 && w >= 1 && H >= 1 && W >= 1, "h, w, H, W must be >= 1");
    RN_REQUIRE(ctx, h < (1ull << 31) && w < (1ull << 31) && B * h * w < (1ull << 31), "B * h * w must be below 2^31");
    if (B == 0) return RN_OK;
    const int saved_layout = ctx->layout;
    RN_TRY(rn_seg_head_reserve(hd, B, h * w));
    ctx->layout = RN_LAYOUT_NHWC;
    int st = RN_OK;
    const int steps = rn_seg_head_plan(hd, B, h, w, H, W, scores_nchw != NULL, labels != NULL, -1, NULL, NULL, NULL);
    for (int step = 0; step < steps && st == RN_OK; ++step)
        st = rn_seg_head_step(hd, ctx, step, x_nhwc, 0, B, h, w, H, W, scores_nchw, labels);
    ctx->layout = saved_layout;
    return st;
}

}  // extern "C"

