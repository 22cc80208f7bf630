// Grouped k x k convolution (torch's groups argument): ResNeXt's conv2.
//
// weight [Cout][Cin/G][k][k]; output channel o belongs to group o / (Cout/G) and reads the input
// channels [g*Cg, (g+1)*Cg), Cg = Cin/G, only.  A per-group GEMM has N = 4..64 and K = 36..576: too
// narrow for a 32x32 MFMA tile.  The fast path (fp32, NHWC, k = 3, Cin == Cout, Cin % 32 == 0, Cg a
// divisor or a multiple of 32) therefore works on SUPER-GROUPS: 32 consecutive output channels and the
// KC = max(32, Cg) consecutive input channels they read.
//
//  * the weight is packed block-diagonally per super-group, with zeros where an input channel of the
//    slice belongs to another group than the output channel (waste 32/Cg for Cg < 32, none above), in
//    the order the kernel consumes it: [super-group][K slice of 32 channels][tap][MFMA step][lane];
//  * grid = (M tiles of 256 output pixels) x (C/32 super-groups), the super-groups of one M tile
//    adjacent in launch order: they read disjoint 128-byte channel slices of the same pixels;
//  * a block of 4 waves keeps the 36 KB weight slice of its (super-group, K slice) in LDS -- one
//    conflict-free ds_read_b32 per MFMA step, shared by the wave's two 32-pixel row tiles -- and
//    fetches its A operands straight from global memory: lane (i, h) of v_mfma_f32_32x32x2_f32 owns
//    pixel i and, per tap, the float4s 2j + h (j = 0..3) of the pixel's 128-byte slice, prefetched
//    one tap ahead;
//  * the K order of an output element is fixed -- (K slice, tap, step) with the pair of channels
//    (8j + e, 8j + 4 + e) inside step 4j + e -- whatever the batch size, the position in the batch or
//    the stream split;
//  * epilogue from the accumulators: scale, shift, residual, ReLU (rn_epilogue), 128-byte row pieces
//    per half wave; the NCHW drop-in route has the same kernel write NCHW.
//
// Non-finite inputs: the zeros of the block-diagonal pack are multiplied like any weight, so a NaN or
// an infinity in one group's input surfaces in the other groups of its 32-channel super-group (never
// outside it).  The direct kernel reads a group's own channels only.
//
// Everything else (other k, Cin != Cout, other Cg, operands off a 16-byte boundary) runs the direct
// kernel: one thread per output element, the reference's loop order (ops.cu:30-45) restricted to the
// group's channels, one fp32 fmaf chain.
//
// bf16 storage: no grouped kernel of its own.  rn_conv2d_grouped_pack_weight_dt(BF16) expands the
// weight to the dense [Cout][Cin][k][k] form with zeros outside the groups and packs the panel of the
// dense bf16 contraction; the forward is rn_conv2d_nhwc_forward_dt on it (correct for every Cg,
// wasteful by G; a non-finite input surfaces in every output channel of its pixel neighbourhood).
#include "rn_conv_params.h"
#include "rn_private.h"

using rn_gemm::f32x16;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SG = 32;           // channels of a super-group
constexpr int TAPS = 9;          // the fast path is 3x3
constexpr int BM = 256;          // output pixels per block: 4 waves x 2 row tiles of 32
constexpr int SLICE = TAPS * SG * SG;  // floats of one (super-group, K slice) weight image

struct GroupParams {
    const float *in;
    const float *w;  // packed, see pack_kernel
    float *out;
    const float *scale, *shift, *residual;
    int relu;
    int H, W, C, Ho, Wo, stride, pad;
    int M, HoWo;
    int kc;   // input channels a super-group reads: max(32, Cg)
    int sgs;  // super-groups: C / 32
    int out_nchw;
    unsigned mul_hw, shr_hw, mul_w, shr_w;
    int dil;  // dilation (>= 1): kernel row kh reads input row ih0 + kh * dil, columns alike
};

// packed index of weight (o, channel cl of the super-group's input slice, tap)
__host__ __device__ inline uint64_t packed_index(int o, int cl, int tap, int nq)
{
    const int sg = o / SG, n = o % SG, q = cl / SG, r = cl % SG;
    const int j = r / 8, h = (r % 8) / 4, e = r % 4, s = 4 * j + e;
    return ((((uint64_t)(sg * nq + q) * TAPS + tap) * 16 + s) * 2 + h) * SG + n;
}

// DIL: p.dil > 1 (a flag of the instantiation: the undilated launches keep their row setup as it was)
template <bool DIL>
__global__ __launch_bounds__(256) void conv_group_kernel(const GroupParams p)
{
    __shared__ __attribute__((aligned(16))) float wl[SLICE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int sg = (int)(blockIdx.x % (unsigned)p.sgs);
    const int m0 = (int)(blockIdx.x / (unsigned)p.sgs) * BM + wave * 64;
    const int nq = p.kc / SG;
    const int cin0 = (sg * SG / p.kc) * p.kc;  // first input channel of the super-group's slice

    // per row tile: element offset of tap (0, 0) of this lane's pixel, and the taps inside the image
    long long a_off[2];
    int a_mask[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = m0 + mt * 32 + i;
        a_off[mt] = 0;
        a_mask[mt] = 0;
        if (m < p.M) {
            const auto [b, oh, ow] = rn_gemm::row_of(m, p);
            const int ih0 = oh * p.stride - p.pad, iw0 = ow * p.stride - p.pad;
            a_off[mt] = ((long long)(b * p.H + ih0) * p.W + iw0) * p.C + cin0 + 4 * h;
            if constexpr (!DIL) {
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw)
                        if (ih0 + kh >= 0 && ih0 + kh < p.H && iw0 + kw >= 0 && iw0 + kw < p.W)
                            a_mask[mt] |= 1 << (kh * 3 + kw);
            } else {
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw)
                        if (ih0 + kh * p.dil >= 0 && ih0 + kh * p.dil < p.H && iw0 + kw * p.dil >= 0 &&
                            iw0 + kw * p.dil < p.W)
                            a_mask[mt] |= 1 << (kh * 3 + kw);
            }
        }
    }

    f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;

    for (int q = 0; q < nq; ++q) {
        if (q > 0) __syncthreads();  // every wave is done with the previous slice
        {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(p.w + (size_t)(sg * nq + q) * SLICE);
            f32x4 *dst = reinterpret_cast<f32x4 *>(wl);
#pragma unroll
            for (int v = 0; v < SLICE / 4 / 256; ++v) dst[v * 256 + t] = src[v * 256 + t];
        }
        __syncthreads();

        f32x4 a[2][2][4];  // [buffer][row tile][float4 j]
        auto load_tap = [&](int tap, f32x4 (&dstv)[2][4]) {
            const int kh = tap / 3, kw = tap % 3;
            const long long toff = (long long)(kh * p.W + kw) * (DIL ? p.dil : 1) * p.C + q * SG;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const bool ok = (a_mask[mt] >> tap) & 1;
                const float *src = p.in + a_off[mt] + toff;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    dstv[mt][j] = ok ? *reinterpret_cast<const f32x4 *>(src + 8 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        load_tap(0, a[0]);
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
            if (tap + 1 < TAPS) load_tap(tap + 1, a[(tap + 1) & 1]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float b = wl[tap * (SG * SG) + (4 * j + e) * 64 + lane];
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tap & 1][mt][j][e], b, acc[mt], 0, 0, 0);
                }
        }
    }

    // accumulator register r of lane (n, h) is row (r/4)*8 + 4*h + r%4, column n of the 32x32 tile
    const int oc = sg * SG + i;
    const float sc = p.scale ? p.scale[oc] : 1.f;
    const float sh = p.shift ? p.shift[oc] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + mt * 32 + (r / 4) * 8 + 4 * h + (r % 4);
            if (m >= p.M) continue;
            float v = acc[mt][r];
            if (p.scale)
                v = fmaf(v, sc, sh);
            else if (p.shift)
                v += sh;
            const size_t nhwc = (size_t)m * p.C + oc;
            if (p.residual) v += p.residual[nhwc];
            if (p.relu) v = fmaxf(v, 0.f);
            if (p.out_nchw) {
                const int b = m / p.HoWo, rem = m - b * p.HoWo;
                p.out[((size_t)b * p.C + oc) * p.HoWo + rem] = v;
            } else {
                p.out[nhwc] = v;
            }
        }
}

// any shape: one thread per output element, ic -> kh -> kw over the group's channels, one fmaf chain
struct GroupDirectParams {
    const float *in;
    const float *w;
    float *out;
    const float *scale, *shift, *residual;
    int relu;
    int k, stride, pad, dil, Ho, Wo, Cin, Cout, H, W, groups;
    int nhwc;      // activation layout
    int w_packed;  // 0: OIHW [Cout][Cin/G][k][k]; 1: the super-group pack of the fast path
    uint64_t total;
};

__global__ __launch_bounds__(256) void conv_group_direct_kernel(const GroupDirectParams p)
{
    const uint64_t gstride = (uint64_t)gridDim.x * 256;
    const int cg = p.Cin / p.groups, og = p.Cout / p.groups;
    const int kc = cg > SG ? cg : SG, nq = kc / SG;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < p.total; idx += gstride) {
        int oc, oh, ow;
        uint64_t b;
        if (p.nhwc) {
            oc = (int)(idx % (uint64_t)p.Cout);
            uint64_t q = idx / (uint64_t)p.Cout;
            ow = (int)(q % (uint64_t)p.Wo);
            q /= (uint64_t)p.Wo;
            oh = (int)(q % (uint64_t)p.Ho);
            b = q / (uint64_t)p.Ho;
        } else {
            ow = (int)(idx % (uint64_t)p.Wo);
            uint64_t q = idx / (uint64_t)p.Wo;
            oh = (int)(q % (uint64_t)p.Ho);
            q /= (uint64_t)p.Ho;
            oc = (int)(q % (uint64_t)p.Cout);
            b = q / (uint64_t)p.Cout;
        }
        const int c0 = (oc / og) * cg;  // the group's first input channel
        const int slice0 = (oc / SG * SG / kc) * kc;
        const int ih0 = oh * p.stride - p.pad, iw0 = ow * p.stride - p.pad;
        float sum = 0.f;
        for (int ic = 0; ic < cg; ++ic) {
            for (int kh = 0; kh < p.k; ++kh) {
                const int ih = ih0 + kh * p.dil;
                if (ih < 0 || ih >= p.H) continue;
                for (int kw = 0; kw < p.k; ++kw) {
                    const int iw = iw0 + kw * p.dil;
                    if (iw < 0 || iw >= p.W) continue;
                    const uint64_t ii = p.nhwc ? (((b * p.H + ih) * p.W + iw) * p.Cin + c0 + ic)
                                               : (((b * p.Cin + c0 + ic) * p.H + ih) * p.W + iw);
                    const uint64_t wi = p.w_packed ? packed_index(oc, c0 + ic - slice0, kh * 3 + kw, nq)
                                                   : (((uint64_t)oc * cg + ic) * p.k + kh) * p.k + kw;
                    sum = fmaf(p.in[ii], p.w[wi], sum);
                }
            }
        }
        if (p.scale) {
            sum = fmaf(sum, p.scale[oc], p.shift ? p.shift[oc] : 0.f);
        } else if (p.shift) {
            sum += p.shift[oc];
        }
        if (p.residual) sum += p.residual[idx];
        if (p.relu) sum = fmaxf(sum, 0.f);
        p.out[idx] = sum;
    }
}

// OIHW [Cout][Cg][3][3] -> the super-group pack; one thread per packed element
__global__ __launch_bounds__(256) void group_pack_kernel(const float *w, float *packed, int C, int cg, uint64_t total)
{
    const int kc = cg > SG ? cg : SG, nq = kc / SG;
    const uint64_t gstride = (uint64_t)gridDim.x * 256;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += gstride) {
        uint64_t r = idx;
        const int n = (int)(r % SG); r /= SG;
        const int h = (int)(r % 2); r /= 2;
        const int s = (int)(r % 16); r /= 16;
        const int tap = (int)(r % TAPS); r /= TAPS;
        const int q = (int)(r % (uint64_t)nq);
        const int sg = (int)(r / (uint64_t)nq);
        const int o = sg * SG + n;
        const int cl = q * SG + 8 * (s / 4) + 4 * h + (s % 4);
        const int c = (sg * SG / kc) * kc + cl;  // input channel
        float v = 0.f;
        if (c / cg == o / cg && c < C) v = w[((uint64_t)o * cg + (c - (o / cg) * cg)) * TAPS + tap];
        packed[idx] = v;
    }
}

// OIHW [Cout][Cg][k][k] -> dense OIHW [Cout][Cin][k][k], zeros outside the groups
__global__ __launch_bounds__(256) void group_expand_kernel(const float *w, float *dense, int Cin, int Cout, int groups,
                                                           int kk, uint64_t total)
{
    const int cg = Cin / groups, og = Cout / groups;
    const uint64_t gstride = (uint64_t)gridDim.x * 256;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += gstride) {
        const int tap = (int)(idx % (uint64_t)kk);
        const int c = (int)(idx / (uint64_t)kk % (uint64_t)Cin);
        const int o = (int)(idx / (uint64_t)kk / (uint64_t)Cin);
        const int g = o / og;
        dense[idx] = c / cg == g ? w[((uint64_t)o * cg + (c - g * cg)) * kk + tap] : 0.f;
    }
}

bool shape_ok(uint64_t Cin, uint64_t Cout, uint64_t groups)
{
    return groups >= 1 && Cin >= 1 && Cout >= 1 && Cin % groups == 0 && Cout % groups == 0;
}

// shapes of the super-group kernel (alignment is checked per call)
bool fast_shape(uint64_t Cin, uint64_t Cout, uint64_t k, uint64_t groups)
{
    if (!shape_ok(Cin, Cout, groups) || k != 3 || Cin != Cout || Cin % SG != 0) return false;
    const uint64_t cg = Cin / groups;
    return SG % cg == 0 || cg % SG == 0;
}

uint64_t packed_numel(uint64_t Cin, uint64_t Cout, uint64_t k, uint64_t groups)
{
    const uint64_t cg = Cin / groups;
    if (fast_shape(Cin, Cout, k, groups)) return Cout * TAPS * (cg > SG ? cg : (uint64_t)SG);
    return Cout * cg * k * k;  // the OIHW weight as it is: the direct kernel reads it
}

bool aligned16(const void *a, const void *b, const void *c, const rn_epilogue *ep)
{
    uintptr_t x = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c);
    if (ep)
        x |= reinterpret_cast<uintptr_t>(ep->scale) | reinterpret_cast<uintptr_t>(ep->shift) |
             reinterpret_cast<uintptr_t>(ep->residual);
    return (x & 15) == 0;
}

int check_args(rn_ctx *ctx, const void *inp, const void *out, const void *weight, uint64_t k, uint64_t stride,
               uint64_t pad, uint64_t dil, uint64_t h_out, uint64_t w_out, uint64_t B, uint64_t Cin, uint64_t Cout,
               uint64_t H, uint64_t W, uint64_t groups)
{
    RN_REQUIRE(ctx, inp && out && weight, "null tensor");
    RN_REQUIRE(ctx, inp != out, "conv2d cannot run in place");
    RN_REQUIRE(ctx, k >= 1 && stride >= 1, "kernel_size and stride must be >= 1");
    RN_REQUIRE(ctx, k < (1u << 12) && stride < (1u << 12) && pad < (1u << 12), "dimension too large");
    RN_REQUIRE(ctx, shape_ok(Cin, Cout, groups), "groups must divide in_channels and out_channels");
    RN_REQUIRE(ctx, groups >= 2, "groups == 1 is rn_conv2d_forward / rn_conv2d_nhwc_forward");
    const uint64_t span = dil * (k - 1) + 1;  // the (dilated) kernel's extent
    RN_REQUIRE(ctx, H + 2 * pad >= span && W + 2 * pad >= span && h_out == (H + 2 * pad - span) / stride + 1 &&
                        w_out == (W + 2 * pad - span) / stride + 1,
               "h_out / w_out do not match the input");
    RN_REQUIRE(ctx, B * H * W * Cin < (1ull << 29) && B * h_out * w_out * Cout < (1ull << 29) &&
                        Cout * (Cin / groups < 32 ? 32 : Cin / groups) * k * k < (1ull << 29),
               "tensor has 2^29 or more elements");
    return RN_OK;
}

int launch_fast(rn_ctx *ctx, const float *inp, float *out, const float *packed, uint64_t stride, uint64_t pad,
                uint64_t dil, uint64_t h_out, uint64_t w_out, uint64_t B, uint64_t C, uint64_t H, uint64_t W, uint64_t groups,
                const rn_epilogue *ep, int out_nchw, const char *what)
{
    GroupParams p;
    const uint64_t cg = C / groups;
    p.in = inp;
    p.w = packed;
    p.out = out;
    p.scale = ep ? ep->scale : nullptr;
    p.shift = ep ? ep->shift : nullptr;
    p.residual = ep ? static_cast<const float *>(ep->residual) : nullptr;
    p.relu = ep ? ep->relu : 0;
    p.H = (int)H;
    p.W = (int)W;
    p.C = (int)C;
    p.Ho = (int)h_out;
    p.Wo = (int)w_out;
    p.stride = (int)stride;
    p.pad = (int)pad;
    p.dil = (int)dil;
    p.M = (int)(B * h_out * w_out);
    p.HoWo = (int)(h_out * w_out);
    p.kc = (int)(cg > SG ? cg : (uint64_t)SG);
    p.sgs = (int)(C / SG);
    p.out_nchw = out_nchw;
    rn_fast_div((unsigned)p.HoWo, &p.mul_hw, &p.shr_hw);
    rn_fast_div((unsigned)p.Wo, &p.mul_w, &p.shr_w);
    const uint64_t blocks = rn_ceil_div((uint64_t)p.M, BM) * (uint64_t)p.sgs;
    if (dil != 1)
        conv_group_kernel<true><<<(unsigned)blocks, 256, 0, ctx->stream>>>(p);
    else
        conv_group_kernel<false><<<(unsigned)blocks, 256, 0, ctx->stream>>>(p);
    return rn_after_launch(ctx, what);
}

int launch_group_direct(rn_ctx *ctx, const float *inp, float *out, const float *w, uint64_t k, uint64_t stride,
                        uint64_t pad, uint64_t dil, uint64_t h_out, uint64_t w_out, uint64_t B, uint64_t Cin, uint64_t Cout,
                        uint64_t H, uint64_t W, uint64_t groups, int nhwc, int w_packed, const rn_epilogue *ep,
                        const char *what)
{
    GroupDirectParams p;
    p.in = inp;
    p.w = w;
    p.out = out;
    p.scale = ep ? ep->scale : nullptr;
    p.shift = ep ? ep->shift : nullptr;
    p.residual = ep ? static_cast<const float *>(ep->residual) : nullptr;
    p.relu = ep ? ep->relu : 0;
    p.k = (int)k;
    p.stride = (int)stride;
    p.pad = (int)pad;
    p.dil = (int)dil;
    p.Ho = (int)h_out;
    p.Wo = (int)w_out;
    p.Cin = (int)Cin;
    p.Cout = (int)Cout;
    p.H = (int)H;
    p.W = (int)W;
    p.groups = (int)groups;
    p.nhwc = nhwc;
    p.w_packed = w_packed;
    p.total = B * Cout * h_out * w_out;
    conv_group_direct_kernel<<<rn_stream_grid(p.total, 256), 256, 0, ctx->stream>>>(p);
    return rn_after_launch(ctx, what);
}

}  // namespace

extern "C" {

uint64_t rn_conv2d_grouped_packed_weight_numel_dt(int dtype, uint64_t in_channels, uint64_t out_channels,
                                                  uint64_t kernel_size, uint64_t groups)
{
    if (!shape_ok(in_channels, out_channels, groups)) return 0;
    if (dtype == RN_DTYPE_BF16)  // the dense panel, zeros outside the groups
        return rn_conv2d_packed_weight_numel_dt(dtype, in_channels, out_channels, kernel_size);
    return dtype == RN_DTYPE_F32 ? packed_numel(in_channels, out_channels, kernel_size, groups) : 0;
}

int rn_conv2d_grouped_pack_weight_dt(rn_ctx *ctx, int dtype, const float *weight_oihw, void *packed,
                                     uint64_t in_channels, uint64_t out_channels, uint64_t kernel_size,
                                     uint64_t groups)
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, weight_oihw && packed, "null tensor");
    RN_REQUIRE(ctx, dtype == RN_DTYPE_F32 || dtype == RN_DTYPE_BF16, "unknown dtype");
    RN_REQUIRE(ctx, shape_ok(in_channels, out_channels, groups) && groups >= 2 && kernel_size >= 1 && kernel_size <= 15,
               "groups (>= 2) must divide in_channels and out_channels; kernel_size 1..15");
    RN_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(weight_oihw) & 3) == 0 && (reinterpret_cast<uintptr_t>(packed) & 3) == 0,
               "misaligned tensor");
    const uint64_t kk = kernel_size * kernel_size, cg = in_channels / groups;
    if (dtype == RN_DTYPE_BF16) {
        const uint64_t dn = out_channels * in_channels * kk;
        RN_REQUIRE(ctx, dn < (1ull << 31), "weight too large");
        void *dense = nullptr;
        RN_TRY(rn_malloc(ctx, &dense, dn * sizeof(float)));
        group_expand_kernel<<<rn_stream_grid(dn, 256), 256, 0, ctx->stream>>>(
            weight_oihw, (float *)dense, (int)in_channels, (int)out_channels, (int)groups, (int)kk, dn);
        int st = rn_after_launch(ctx, "rn_conv2d_grouped_pack_weight_dt(expand)");
        if (st == RN_OK)
            st = rn_conv2d_pack_weight_dt(ctx, dtype, (const float *)dense, packed, in_channels, out_channels, kernel_size);
        if (st == RN_OK) st = rn_sync(ctx);  // the dense copy is freed below
        rn_free(ctx, dense);
        return st;
    }
    const uint64_t pn = packed_numel(in_channels, out_channels, kernel_size, groups);
    RN_REQUIRE(ctx, pn < (1ull << 31), "weight too large");
    if (fast_shape(in_channels, out_channels, kernel_size, groups)) {
        group_pack_kernel<<<rn_stream_grid(pn, 256), 256, 0, ctx->stream>>>(weight_oihw, (float *)packed,
                                                                            (int)in_channels, (int)cg, pn);
        return rn_after_launch(ctx, "rn_conv2d_grouped_pack_weight_dt");
    }
    return rn_memcpy_d2d(ctx, packed, weight_oihw, pn * sizeof(float));
}

int rn_conv2d_grouped_nhwc_forward_dt(rn_ctx *ctx, int dtype, int out_dtype, const void *inp, void *out,
                                      const void *packed_weight, uint64_t kernel_size, uint64_t stride,
                                      uint64_t padding, uint64_t h_out, uint64_t w_out, uint64_t B,
                                      uint64_t in_channels, uint64_t out_channels, uint64_t H, uint64_t W,
                                      uint64_t groups, const rn_epilogue *epilogue)
{
    return rn_conv_group_nhwc_forward_dt(ctx, dtype, out_dtype, inp, out, packed_weight, kernel_size, stride, padding,
                                         1, h_out, w_out, B, in_channels, out_channels, H, W, groups, epilogue);
}

// library-internal (rn_private.h): the entry point above with a dilation the caller has validated
int rn_conv_group_nhwc_forward_dt(rn_ctx *ctx, int dtype, int out_dtype, const void *inp, void *out,
                                  const void *packed_weight, uint64_t kernel_size, uint64_t stride, uint64_t padding,
                                  uint64_t dilation, uint64_t h_out, uint64_t w_out, uint64_t B, uint64_t in_channels,
                                  uint64_t out_channels, uint64_t H, uint64_t W, uint64_t groups,
                                  const rn_epilogue *epilogue)
{
    RN_ENTER(ctx);
    if (B * out_channels * h_out * w_out == 0) return RN_OK;
    RN_TRY(check_args(ctx, inp, out, packed_weight, kernel_size, stride, padding, dilation, h_out, w_out, B,
                      in_channels, out_channels, H, W, groups));
    if (dtype == RN_DTYPE_BF16)  // dense panel with zeros outside the groups: the dense contraction
        return rn_conv_dense_nhwc_forward_dt(ctx, dtype, out_dtype, inp, out, packed_weight, kernel_size, stride,
                                             padding, dilation, h_out, w_out, B, in_channels, out_channels, H, W,
                                             epilogue);
    RN_REQUIRE(ctx, dtype == RN_DTYPE_F32 && out_dtype == RN_DTYPE_F32, "fp32 input implies fp32 output");
    const rn_epilogue none = {nullptr, nullptr, nullptr, 0};
    const rn_epilogue *ep = epilogue ? epilogue : &none;
    RN_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(inp) | reinterpret_cast<uintptr_t>(out) |
                      reinterpret_cast<uintptr_t>(packed_weight) | reinterpret_cast<uintptr_t>(ep->scale) |
                      reinterpret_cast<uintptr_t>(ep->shift) | reinterpret_cast<uintptr_t>(ep->residual)) & 3) == 0,
               "misaligned tensor (fp32 tensors sit on 4-byte boundaries)");
    const bool fs = fast_shape(in_channels, out_channels, kernel_size, groups);
    if (fs && aligned16(inp, out, packed_weight, epilogue))
        return launch_fast(ctx, (const float *)inp, (float *)out, (const float *)packed_weight, stride, padding,
                           dilation, h_out, w_out, B, in_channels, H, W, groups, epilogue, 0, "rn_conv2d_grouped_nhwc_forward_dt");
    return launch_group_direct(ctx, (const float *)inp, (float *)out, (const float *)packed_weight, kernel_size, stride,
                               padding, dilation, h_out, w_out, B, in_channels, out_channels, H, W, groups, 1, fs ? 1 : 0,
                               epilogue, "rn_conv2d_grouped_nhwc_forward_dt(direct)");
}

int rn_conv2d_grouped_forward(rn_ctx *ctx, const float *inp, float *out, const float *weight, uint64_t kernel_size,
                              uint64_t stride, uint64_t padding, uint64_t h_out, uint64_t w_out, uint64_t B,
                              uint64_t in_channels, uint64_t out_channels, uint64_t H, uint64_t W, uint64_t groups)
{
    return rn_conv_group_forward(ctx, inp, out, weight, kernel_size, stride, padding, 1, h_out, w_out, B, in_channels,
                                 out_channels, H, W, groups);
}

// library-internal (rn_private.h): the entry point above with a dilation the caller has validated
int rn_conv_group_forward(rn_ctx *ctx, const float *inp, float *out, const float *weight, uint64_t kernel_size,
                          uint64_t stride, uint64_t padding, uint64_t dilation, uint64_t h_out, uint64_t w_out,
                          uint64_t B, uint64_t in_channels, uint64_t out_channels, uint64_t H, uint64_t W,
                          uint64_t groups)
{
    RN_ENTER(ctx);  // on a deferred context: runs what is recorded, then this call at once
    if (B * out_channels * h_out * w_out == 0) return RN_OK;
    RN_TRY(check_args(ctx, inp, out, weight, kernel_size, stride, padding, dilation, h_out, w_out, B, in_channels,
                      out_channels, H, W, groups));
    RN_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(inp) | reinterpret_cast<uintptr_t>(out) |
                      reinterpret_cast<uintptr_t>(weight)) & 3) == 0,
               "misaligned tensor (fp32 tensors sit on 4-byte boundaries)");
    const int nhwc = ctx->layout == RN_LAYOUT_NHWC;
    // as for the dense entry points: the matrix-core path when every operand sits on a 16-byte boundary
    const bool fast = fast_shape(in_channels, out_channels, kernel_size, groups) && aligned16(inp, out, weight, nullptr);
    if (!fast)  // exact reference order; OIHW weights as given
        return launch_group_direct(ctx, inp, out, weight, kernel_size, stride, padding, dilation, h_out, w_out, B, in_channels,
                                   out_channels, H, W, groups, nhwc, 0, nullptr, "rn_conv2d_grouped_forward(direct)");
    void *wp = nullptr;
    const uint64_t pn = packed_numel(in_channels, out_channels, kernel_size, groups);
    RN_TRY(rn_scratch(ctx, 1, pn * sizeof(float), &wp));
    group_pack_kernel<<<rn_stream_grid(pn, 256), 256, 0, ctx->stream>>>(weight, (float *)wp, (int)in_channels,
                                                                        (int)(in_channels / groups), pn);
    RN_TRY(rn_after_launch(ctx, "rn_conv2d_grouped_forward(pack)"));
    if (nhwc)
        return launch_fast(ctx, inp, out, (const float *)wp, stride, padding, dilation, h_out, w_out, B, in_channels, H, W, groups,
                           nullptr, 0, "rn_conv2d_grouped_forward(nhwc)");
    void *xin = nullptr;
    RN_TRY(rn_scratch(ctx, 2, B * H * W * in_channels * sizeof(float), &xin));
    RN_TRY(rn_nchw_to_nhwc(ctx, inp, (float *)xin, B, in_channels, H, W));
    return launch_fast(ctx, (const float *)xin, out, (const float *)wp, stride, padding, dilation, h_out, w_out, B, in_channels, H,
                       W, groups, nullptr, 1, "rn_conv2d_grouped_forward");
}

}  // extern "C"
