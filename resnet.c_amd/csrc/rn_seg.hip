// Semantic segmentation: the bilinear upsample of per-pixel class scores with an optional fused argmax
// (rn_upsample_bilinear_forward), the channel concat with a per-image broadcast source
// (rn_concat_channels_forward_dt), and torchvision's FCNHead and DeepLabHead as one object (rn_seg_head_*): a table
// of convolution units and a list of launches over the library's own convolutions, which the two create functions
// fill differently.  The reference classifies whole images only; nothing here has a counterpart in it.
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

}  // namespace

// ---- the head's tables --------------------------------------------------------------------------------------
// A head is a table of convolution "units", the state dict's tensors they are made of, a list of scratch tensors
// and the list of a forward's launches.  Its create function fills the four; nothing else knows a kind of head.
//   FCNHead(in, classes): Conv3x3(in, mid) + BN + ReLU, Conv1x1(mid, classes).  2 units, 3 launches.
//   DeepLabHead(in, classes) = ASPP(in, rates, a) + Conv3x3(a, a) + BN + ReLU + Conv1x1(a, classes).  n + 5 units
//   (the 1x1 branch, the n dilated 3x3 branches, the pooled branch's 1x1, the projection, the 3x3, the
//   classifier), n + 8 launches.
constexpr int kSegMaxRates = 4, kSegMaxUnits = kSegMaxRates + 5;
constexpr int kSegMaxBufs = kSegMaxRates + 5, kSegMaxSteps = kSegMaxRates + 8;

// A k x k convolution of cin -> cout channels, both as they run (padded).  bn: a batch-norm folded into scale and
// shift and a ReLU follow, the output is of the storage type; parameters first .. first + 4 are the weight and the
// batch-norm's weight, bias, running_mean and running_var.  Otherwise (the classifier) it carries a bias, which is
// its shift, has no ReLU and an fp32 output; parameters first and first + 1.
struct seg_unit {
    uint64_t cin, cout, k;
    uint64_t dilation;  // 0: a plain convolution, padding k / 2; else a dilated 3x3 branch of ASPP, padding = dilation
    int bn, first;
    rn_stage_unit dev;  // center: a dilated branch's centre tap weight[:, :, 1, 1] packed as a 1x1 panel
};

struct seg_buf {  // a scratch tensor: [cap_img, channels] or [cap_pix, channels], fp32 or of the storage type
    int per_image, f32;
    uint64_t channels;
    void *ptr;
};

// A launch of a forward.  src, dst: scratch tensors; src -1 is the input map.  SEG_CONV: unit u (on a per-image src:
// B "pixels").  SEG_POOL: the global average of src.  SEG_CONCAT: scratch tensors 0 .. u - 1 side by side, then the
// per-image src at every pixel of its image.  SEG_UPSAMPLE: src to the caller's scores and labels.
enum { SEG_CONV, SEG_POOL, SEG_CONCAT, SEG_UPSAMPLE };

struct seg_step {
    int kind, u, src, dst;
    const char *name;  // of its profile record
};

struct rn_seg_head {
    rn_ctx *ctx;
    uint64_t cin, classes;
    uint64_t midp, cpad;  // the classifier's channels as it runs (seg_add_unit)
    int dtype, finalized;
    int center_tap;  // rn_seg_head_set_center_tap
    int n_units, n_bufs, n_steps;
    seg_unit unit[kSegMaxUnits];
    rn_params params;  // 5 per unit with a batch-norm, 2 of the classifier: at most 5 * (kSegMaxUnits - 1) + 2
    seg_buf buf[kSegMaxBufs];
    seg_step step[kSegMaxSteps];
    uint64_t cap[2];  // coarse pixels (images x h x w) and images the scratch tensors hold
};
enum { kSegPix, kSegImg };
static_assert(5 * (kSegMaxUnits - 1) + 2 <= RN_PARAMS_MAX, "the parameter table holds a DeepLab head of kSegMaxRates rates");

namespace {

void seg_add_tensor(rn_seg_head *hd, const char *module, const char *name, uint64_t rows, uint64_t len, uint64_t prows,
                    uint64_t pitch, float fill)
{
    char key[RN_PARAM_KEY];
    snprintf(key, sizeof(key), "%s.%s", module, name);
    rn_params_add(&hd->params, key, NULL, rows, len, prows, pitch, fill);
}

// The unit `conv` (+ batch-norm `norm`, or NULL: + bias) of the state dict: cin -> cout channels there.  It runs
// with cin rounded up to a multiple of 64 (the bf16 contraction's K granule; only a 1x1 is ever given such a cin)
// and cout to one of 64 with a batch-norm (the next unit's cin) or of 4 without (16-byte coarse pixels).  The
// added rows and columns of the weight are zero, and so is the bias; an added channel of the batch-norm has
// variance 1 and zeros otherwise (scale = 0 / sqrt(1 + eps) = 0, shift = 0), so it holds ReLU(0) = 0 and meets
// zero columns of the next panel: exact zeros added to every sum.  Returns the unit's index.
int seg_add_unit(rn_seg_head *hd, const char *conv, const char *norm, uint64_t cin, uint64_t cout, uint64_t k,
                 uint64_t dilation)
{
    static const char *const bn[4] = {"weight", "bias", "running_mean", "running_var"};
    seg_unit *un = &hd->unit[hd->n_units];
    un->cin = (cin + 63) / 64 * 64, un->cout = norm ? (cout + 63) / 64 * 64 : (cout + 3) / 4 * 4;
    un->k = k, un->dilation = dilation, un->bn = norm != NULL, un->first = hd->params.n;
    seg_add_tensor(hd, conv, "weight", cout, cin * k * k, un->cout, un->cin * k * k, 0.0f);
    if (!norm) seg_add_tensor(hd, conv, "bias", 1, cout, 1, un->cout, 0.0f);
    for (int j = 0; norm && j < 4; ++j) seg_add_tensor(hd, norm, bn[j], 1, cout, 1, un->cout, j == 3 ? 1.0f : 0.0f);
    return hd->n_units++;
}

int seg_add_buf(rn_seg_head *hd, int per_image, uint64_t channels, int f32)
{
    seg_buf *b = &hd->buf[hd->n_bufs];
    b->per_image = per_image, b->channels = channels, b->f32 = f32;
    return hd->n_bufs++;
}

void seg_add_step(rn_seg_head *hd, int kind, int u, int src, int dst, const char *name)
{
    seg_step *s = &hd->step[hd->n_steps++];
    s->kind = kind, s->u = u, s->src = src, s->dst = dst, s->name = name;
}

int seg_new(rn_ctx *ctx, rn_seg_head **out, uint64_t in_channels, uint64_t classes, const char *who)
{
    rn_seg_head *hd = (rn_seg_head *)calloc(1, sizeof(*hd));
    if (!hd) return rn_set_error(ctx, RN_ERR_NOMEM, "%s: out of host memory", who);
    hd->ctx = ctx, hd->cin = in_channels, hd->classes = classes, hd->dtype = RN_DTYPE_F32, hd->center_tap = 1;
    *out = hd;
    return RN_OK;
}

// what every head ends with: the classifier on scratch tensor `from` (mid channels in the state dict), the upsample
void seg_add_classifier(rn_seg_head *hd, int from, uint64_t mid)
{
    const int u = seg_add_unit(hd, "classifier.4", NULL, mid, hd->classes, 1, 0);
    hd->midp = hd->unit[u].cin, hd->cpad = hd->unit[u].cout;
    const int coarse = seg_add_buf(hd, 0, hd->cpad, 1);
    seg_add_step(hd, SEG_CONV, u, from, coarse, "seg_conv2");
    seg_add_step(hd, SEG_UPSAMPLE, 0, coarse, -1, "seg_upsample");
}

// Whether dilated branch `un` of a forward on an h x w map runs as the 1x1 contraction on its centre tap.  With
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
bool dl_center_route(const rn_seg_head *hd, const seg_unit *un, uint64_t h, uint64_t w)
{
    if (!hd->center_tap || !un->dilation) return false;
    if (un->dilation < h || un->dilation < w) return false;
    return hd->dtype == RN_DTYPE_BF16 || 9 * hd->cin / 32 < 32;
}

// whether every scratch tensor holds `pix` coarse pixels or `images` images, whichever it is made of
bool seg_fits(const rn_seg_head *hd, uint64_t pix, uint64_t images)
{
    for (int i = 0; i < hd->n_bufs; ++i)
        if (hd->buf[i].per_image ? images > hd->cap[kSegImg] : pix > hd->cap[kSegPix]) return false;
    return true;
}

// the scratch tensors for `pix` coarse pixels and `images` images; returns how many
int seg_scratch(rn_seg_head *hd, uint64_t pix, uint64_t images, rn_scratch_item *list)
{
    for (int i = 0; i < hd->n_bufs; ++i) {
        seg_buf *b = &hd->buf[i];
        list[i] = {&b->ptr, (b->per_image ? images : pix) * b->channels * (b->f32 ? 4 : rn_elem_size(hd->dtype))};
    }
    return hd->n_bufs;
}

// where the B images of a launch whose scratch starts img0 images (pix0 coarse pixels) in begin in scratch tensor i
void *seg_at(const rn_seg_head *hd, int i, uint64_t img0, uint64_t pix0)
{
    const seg_buf *b = &hd->buf[i];
    const uint64_t es = b->f32 ? 4 : rn_elem_size(hd->dtype);
    return (char *)b->ptr + (b->per_image ? img0 : pix0) * b->channels * es;
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
    const uint64_t es = rn_elem_size(dtype), per = 16 / es;  // elements of a 16-byte chunk
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
        RN_REQUIRE(ctx, !rn_overlap(dst, dst_bytes, srcs[i], npix * channels[i] * es), "dst overlaps a source");
    RN_REQUIRE(ctx, !per_image || !rn_overlap(dst, dst_bytes, per_image, B * per_image_channels * es),
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
    RN_TRY(seg_new(ctx, out, in_channels, classes, __func__));
    rn_seg_head *hd = *out;
    const int u = seg_add_unit(hd, "classifier.0", "classifier.1", in_channels, mid_channels, 3, 0);
    const int mid = seg_add_buf(hd, 0, hd->unit[u].cout, 0);
    seg_add_step(hd, SEG_CONV, u, -1, mid, "seg_conv1");
    seg_add_classifier(hd, mid, mid_channels);
    return RN_OK;
}

int rn_seg_head_create_deeplab(rn_ctx *ctx, rn_seg_head **out, uint64_t in_channels, uint64_t aspp_channels,
                               uint64_t classes, uint64_t n_rates, const uint64_t *rates)
{
    static const char *const branch_ops[kSegMaxRates + 1] = {"aspp_conv0", "aspp_conv1", "aspp_conv2", "aspp_conv3",
                                                             "aspp_conv4"};
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, out, "out is NULL");
    *out = NULL;
    RN_REQUIRE(ctx, in_channels >= 64 && in_channels % 64 == 0 && in_channels <= 8192,
               "in_channels must be a multiple of 64 (at most 8192)");
    RN_REQUIRE(ctx, aspp_channels >= 64 && aspp_channels % 64 == 0 && aspp_channels <= 1024,
               "aspp_channels must be a multiple of 64 (at most 1024)");
    RN_REQUIRE(ctx, classes >= 1 && classes <= 256, "classes must be 1..256");
    RN_REQUIRE(ctx, n_rates >= 1 && n_rates <= (uint64_t)kSegMaxRates && rates, "n_rates must be 1..4 (and rates not NULL)");
    for (uint64_t i = 0; i < n_rates; ++i)
        RN_REQUIRE(ctx, rates[i] >= 1 && rates[i] <= RN_CONV_MAX_DILATION, "a rate must be 1..RN_CONV_MAX_DILATION");
    RN_TRY(seg_new(ctx, out, in_channels, classes, __func__));
    rn_seg_head *hd = *out;
    const int n = (int)n_rates;
    const uint64_t a = aspp_channels;
    // scratch: per coarse pixel the n + 1 branch tensors (0 .. n: what the concat reads) and the concat; per image
    // the pooled map and the pooled branch.  The projected tensor and the 3x3's output live in branch 0's and branch
    // 1's tensors, which are dead behind the concat.
    for (int i = 0; i <= n; ++i) seg_add_buf(hd, 0, a, 0);
    const int cat = seg_add_buf(hd, 0, (n_rates + 2) * a, 0);
    const int pool_in = seg_add_buf(hd, 1, in_channels, 0), pool_out = seg_add_buf(hd, 1, a, 0);
    for (int i = 0; i <= n; ++i) {  // convs.0 is the 1x1 branch, convs.1 .. n the dilated ones
        char conv[48], norm[48];
        snprintf(conv, sizeof(conv), "classifier.0.convs.%d.0", i);
        snprintf(norm, sizeof(norm), "classifier.0.convs.%d.1", i);
        const int u = seg_add_unit(hd, conv, norm, in_channels, a, i ? 3 : 1, i ? rates[i - 1] : 0);
        seg_add_step(hd, SEG_CONV, u, -1, i, branch_ops[i]);
    }
    // the pooled branch's Sequential starts with the pool: its convolution is .1, its batch-norm .2
    char conv[48], norm[48];
    snprintf(conv, sizeof(conv), "classifier.0.convs.%d.1", n + 1);
    snprintf(norm, sizeof(norm), "classifier.0.convs.%d.2", n + 1);
    seg_add_step(hd, SEG_POOL, 0, -1, pool_in, "aspp_pool");
    seg_add_step(hd, SEG_CONV, seg_add_unit(hd, conv, norm, in_channels, a, 1, 0), pool_in, pool_out, "aspp_pool_conv");
    seg_add_step(hd, SEG_CONCAT, n + 1, pool_out, cat, "aspp_concat");
    const int project = seg_add_unit(hd, "classifier.0.project.0", "classifier.0.project.1", (n_rates + 2) * a, a, 1, 0);
    seg_add_step(hd, SEG_CONV, project, cat, 0, "aspp_project");
    seg_add_step(hd, SEG_CONV, seg_add_unit(hd, "classifier.1", "classifier.2", a, a, 3, 0), 0, 1, "seg_conv1");
    seg_add_classifier(hd, 1, a);
    return RN_OK;
}

int rn_seg_head_set_center_tap(rn_seg_head *hd, int on)
{
    if (!hd) return RN_ERR_INVALID;
    int dilated = 0;
    for (int u = 0; u < hd->n_units; ++u) dilated |= hd->unit[u].dilation != 0;
    RN_REQUIRE(hd->ctx, dilated, "not a DeepLab head");
    RN_REQUIRE(hd->ctx, on == 0 || on == 1, "on must be 0 or 1");
    hd->center_tap = on;
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
    return rn_stage_set_tensor(hd->ctx, __func__, "the head", hd->finalized, &hd->params, key, host_data, numel);
}

// unit `un` on the device: its parameters as they are stored (seg_add_unit's padding), packed; a dilated branch's
// centre tap, cut from the weight [cout, cin, 3, 3] (a branch is never padded), as a second panel
static int seg_pack_unit(rn_seg_head *hd, seg_unit *un)
{
    const rn_params *t = &hd->params;
    const rn_params_entry *e = &t->p[un->first];
    const uint64_t n = e->prows * e->pitch, taps = un->cout * un->cin;
    float *buf = (float *)malloc((n + 4 * un->cout + (un->dilation ? taps : 0)) * sizeof(float));
    if (!buf) return rn_set_error(hd->ctx, RN_ERR_NOMEM, "rn_seg_head_finalize: out of host memory");
    float *vec = buf + n, *tap = vec + 4 * un->cout;
    const float *bn[4];
    rn_params_write(t, un->first, buf);
    for (int j = 0; j < (un->bn ? 4 : 1); ++j) rn_params_write(t, un->first + 1 + j, vec + j * un->cout), bn[j] = vec + j * un->cout;
    int st = rn_stage_pack(hd->ctx, hd->dtype, buf, un->cin, un->cout, un->k, un->bn ? NULL : vec, un->bn ? bn : NULL, &un->dev);
    if (st == RN_OK && un->dilation) {
        rn_stage_unit c = {};
        for (uint64_t i = 0; i < taps; ++i) tap[i] = e->host[i * 9 + 4];
        st = rn_stage_pack(hd->ctx, hd->dtype, tap, un->cin, un->cout, 1, NULL, NULL, &c);
        un->dev.center = c.packed;
    }
    free(buf);
    return st;
}

int rn_seg_head_finalize(rn_seg_head *hd)
{
    if (!hd) return RN_ERR_INVALID;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    if (hd->finalized) return RN_OK;
    RN_TRY(rn_stage_all_set(ctx, __func__, &hd->params));
    for (int u = 0; u < hd->n_units; ++u) RN_TRY(seg_pack_unit(hd, &hd->unit[u]));
    rn_params_free(&hd->params);
    hd->finalized = 1;
    return RN_OK;
}

int rn_seg_head_destroy(rn_seg_head *hd)
{
    if (!hd) return RN_OK;
    rn_ctx *ctx = hd->ctx;
    RN_ENTER(ctx);
    RN_TRY(rn_sync(ctx));
    rn_scratch_item list[kSegMaxBufs];
    rn_stage_free_list(ctx, list, seg_scratch(hd, 0, 0, list));
    rn_params_free(&hd->params);
    for (int u = 0; u < hd->n_units; ++u) rn_stage_unit_free(ctx, &hd->unit[u].dev);
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
// number of launches; step outside 0 .. that - 1 only counts.  Every count is an integer far below 2^53, so the
// doubles are exact whatever the order of their products.
int rn_seg_head_plan(const rn_seg_head *hd, uint64_t B, uint64_t h, uint64_t w, uint64_t H, uint64_t W, int want_scores,
                     int want_labels, int step, const char **name, double *flops, double *bytes)
{
    if (step < 0 || step >= hd->n_steps) return hd->n_steps;
    const seg_step *s = &hd->step[step];
    const double es = (double)rn_elem_size(hd->dtype), nb = (double)B, P = (double)(B * h * w);
    double f = 0.0, by = 0.0;
    switch (s->kind) {
    case SEG_CONV: {  // the FLOPs of the route that runs
        const seg_unit *un = &hd->unit[s->u];
        const double M = s->src >= 0 && hd->buf[s->src].per_image ? nb : P, cin = (double)un->cin, cout = (double)un->cout;
        const double taps = dl_center_route(hd, un, h, w) ? 1.0 : (double)(un->k * un->k);
        f = 2.0 * M * taps * cin * cout, by = M * (es * cin + (un->bn ? es : 4.0) * cout) + es * taps * cin * cout;
        break;
    }
    case SEG_POOL: by = es * nb * (double)hd->buf[s->dst].channels * (double)(h * w + 1); break;
    case SEG_CONCAT: {
        const double cat = (double)hd->buf[s->dst].channels, a = (double)hd->buf[s->src].channels;
        by = es * (2.0 * P * cat - P * a + nb * a);
        break;
    }
    default:
        by = 4.0 * P * (double)hd->cpad +
             (double)(B * H * W) * ((want_scores ? 4.0 * (double)hd->classes : 0.0) + (want_labels ? 1.0 : 0.0));
        break;
    }
    if (name) *name = s->name;
    if (flops) *flops = f;
    if (bytes) *bytes = by;
    return hd->n_steps;
}

// the scratch for `images` images of `pixels` coarse pixels (h x w) each; it never shrinks (rn_stage_grow's rule)
int rn_seg_head_reserve(rn_seg_head *hd, uint64_t images, uint64_t pixels)
{
    const uint64_t pix = images * pixels;
    if (seg_fits(hd, pix, images)) return RN_OK;
    const uint64_t want[2] = {pix > hd->cap[kSegPix] ? pix : hd->cap[kSegPix], images > hd->cap[kSegImg] ? images : hd->cap[kSegImg]};
    rn_scratch_item list[kSegMaxBufs];
    return rn_stage_grow(hd->ctx, "rn_seg_head", list, seg_scratch(hd, want[kSegPix], want[kSegImg], list), hd->cap, want, 2);
}

// one of the head's launches on `ctx` (the head's own context, or the context of the model's stream the images
// run on): B images whose scratch starts `img0` images (img0 * h * w coarse pixels) into the head's tensors
int rn_seg_head_step(rn_seg_head *hd, rn_ctx *ctx, int step, const void *x_nhwc, uint64_t img0, uint64_t B, uint64_t h,
                     uint64_t w, uint64_t H, uint64_t W, float *scores_nchw, uint8_t *labels)
{
    const uint64_t pix0 = img0 * h * w;
    const int dt = hd->dtype;
    RN_REQUIRE(ctx, step >= 0 && step < hd->n_steps, "no such step");
    if (!seg_fits(hd, pix0 + B * h * w, img0 + B)) return rn_set_error(ctx, RN_ERR_INVALID, "rn_seg_head: scratch not reserved");
    const seg_step *s = &hd->step[step];
    const bool per_image = s->src >= 0 && hd->buf[s->src].per_image;
    const void *src = s->src < 0 ? x_nhwc : seg_at(hd, s->src, img0, pix0);
    void *dst = s->dst < 0 ? NULL : seg_at(hd, s->dst, img0, pix0);
    switch (s->kind) {
    case SEG_CONV: {
        const seg_unit *un = &hd->unit[s->u];
        const uint64_t uh = per_image ? 1 : h, uw = per_image ? 1 : w;
        rn_epilogue ep;
        ep.scale = un->dev.scale, ep.shift = un->dev.shift, ep.residual = NULL, ep.relu = un->bn;
        if (un->dilation && !dl_center_route(hd, un, h, w))
            return rn_conv2d_dilated_nhwc_forward_dt(ctx, dt, dt, src, dst, un->dev.packed, 3, 1, un->dilation, un->dilation, h,
                                                     w, B, un->cin, un->cout, h, w, 1, &ep);
        const uint64_t k = un->dilation ? 1 : un->k;  // a dilated branch gets here on its centre tap
        return rn_conv2d_nhwc_forward_dt(ctx, dt, un->bn ? dt : RN_DTYPE_F32, src, dst, un->dilation ? un->dev.center : un->dev.packed,
                                         k, 1, k / 2, uh, uw, B, un->cin, un->cout, uh, uw, &ep);
    }
    case SEG_POOL: return rn_global_avgpool_nhwc_forward_dt(ctx, dt, src, dst, B, hd->buf[s->dst].channels, h, w);
    case SEG_CONCAT: {
        const void *srcs[kSegMaxRates + 1];
        uint64_t ch[kSegMaxRates + 1];
        for (int i = 0; i < s->u; ++i) srcs[i] = seg_at(hd, i, img0, pix0), ch[i] = hd->buf[i].channels;
        return rn_concat_channels_forward_dt(ctx, dt, (uint64_t)s->u, srcs, ch, src, hd->buf[s->src].channels, dst, B, h * w);
    }
    default:
        return rn_upsample_bilinear_forward(ctx, (const float *)src, B, h, w, hd->classes, hd->cpad, H, W, scores_nchw,
                                            labels);
    }
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
    for (int step = 0; step < hd->n_steps && st == RN_OK; ++step)
        st = rn_seg_head_step(hd, ctx, step, x_nhwc, 0, B, h, w, H, W, scores_nchw, labels);
    ctx->layout = saved_layout;
    return st;
}

}  // extern "C"

