// Network input from a decoder's bytes: 8-bit interleaved RGB [B,H,W,3] -> the first tensor of the
// forward, [B,H+2b,W+2b,Cpad] in the model dtype, normalised on the way.  It writes what
// rn_nchw_to_nhwc_pad_dt writes when it is fed the host-normalised fp32 NCHW image, bit for bit:
//     x = ((float)px / 255.0f - mean[c]) / std[c]
// in fp32 with correctly rounded divisions (the compiler's IEEE sequence; no product and sum that
// could contract into an fma), then the same float -> bf16 conversion.  The reference normalises on
// the host (preprocess.py) and uploads fp32; this is a quarter of those bytes.
#include "rn_internal.h"

namespace {

typedef __bf16 bf16_t;

// the 3 x 256 possible results of one (mean, std): every block fills its own copy in LDS (three
// entries a thread), after which an element costs one LDS read instead of two divisions
__device__ __forceinline__ float normalise(uint32_t px, float mean, float std)
{
    return ((float)px / 255.0f - mean) / std;
}

struct norm_t {
    float mean[3], std[3];
};

__device__ __forceinline__ void fill_table(float *tab, const norm_t &nm)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) tab[c * 256 + threadIdx.x] = normalise(threadIdx.x, nm.mean[c], nm.std[c]);
    __syncthreads();
}

// any shape and alignment: one element per thread and step
template <typename T>
__global__ __launch_bounds__(256) void image_u8_border_kernel(const uint8_t *__restrict__ src, T *__restrict__ dst,
                                                              uint32_t H, uint32_t W, uint32_t Cpad,
                                                              uint32_t border, uint64_t total, norm_t nm)
{
    __shared__ float tab[768];
    fill_table(tab, nm);
    const uint64_t gstride = (uint64_t)gridDim.x * 256;
    const uint32_t Hp = H + 2 * border, Wp = W + 2 * border;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += gstride) {
        const uint32_t c = (uint32_t)(i % Cpad);
        uint64_t p = i / Cpad;
        const uint32_t wp = (uint32_t)(p % Wp);
        p /= Wp;
        const uint32_t hp = (uint32_t)(p % Hp);
        const uint64_t b = p / Hp;
        const uint32_t h = hp - border, w = wp - border;  // wrap = out of range
        float v = 0.f;
        if (c < 3 && h < H && w < W) v = tab[c * 256 + src[((b * H + h) * W + w) * 3 + c]];
        dst[i] = (T)v;
    }
}

template <typename T, int N>
struct out16;
template <>
struct out16<float, 4> {
    float v[4];
    __device__ void set(int e, float x) { v[e] = x; }
    __device__ uint4 bits() const { return __builtin_bit_cast(uint4, *this); }
};
template <>
struct out16<bf16_t, 8> {
    bf16_t v[8];
    __device__ void set(int e, float x) { v[e] = (bf16_t)x; }
    __device__ uint4 bits() const { return __builtin_bit_cast(uint4, *this); }
};

// The fast form: one 16-byte store per thread and step (NE = 4 fp32 or 8 bf16 elements, which lie in
// at most two rows of the padded image), the bytes behind it from aligned dword loads of the image.
// In the byte image the pixels of a row, and with border 0 the rows too, follow each other, so the
// elements of a store that are not border or pad channel come from one run of source bytes that
// starts at s0 = 3 * ((hp - border) * W + (wp - border)) [+ channel, CPAD 3] of the store's first
// element, whether that element itself is inside or not: ND dwords from s0 / 4 on are loaded (indices
// clamped into the image: a clamped dword only feeds elements that are border), shifted down by
// s0 % 4 bytes with v_alignbyte, and element e takes byte e (CPAD 3) or 3 * (e / 4) + e % 4 (CPAD 4)
// of the result.  Needs: H * W * 3 % 4 == 0 and a 4-byte aligned image (dword loads), the padded
// image a whole number of 16-byte stores, border == 0 or >= 3 (so that no store has an inside
// element in each of two rows) and W + 2b >= 4 (a store's pixels wrap into the next row once).  Divisions by CPAD and W + 2b are multiply-high, as in rn_layout.hip.
template <typename T, int NE, int CPAD>
__global__ __launch_bounds__(256) void image_u8_border_x16_kernel(
    const uint8_t *__restrict__ src, uint4 *__restrict__ dst, uint32_t H, uint32_t W, uint32_t border,
    uint32_t Wp, uint32_t n16, uint32_t steps, uint32_t mul_w, uint32_t shr_w, norm_t nm)
{
    __shared__ float tab[768];
    fill_table(tab, nm);
    constexpr int NB = CPAD == 3 ? NE : 3 * (NE / 4);  // source bytes behind one store
    constexpr int ND = (NB + 3 + 3) / 4;               // dwords that hold them at any byte offset
    const uint64_t b = blockIdx.y;
    const int32_t nd = (int32_t)(H * W * 3 / 4);
    const uint32_t *img = reinterpret_cast<const uint32_t *>(src + b * H * W * 3);
    uint32_t i = blockIdx.x * (256 * steps) + threadIdx.x;
    for (uint32_t s = 0; s < steps && i < n16; ++s, i += 256) {
        const uint32_t idx0 = NE * i;
        const uint32_t pix0 = CPAD == 4 ? idx0 / 4 : __umulhi(idx0, 0xAAAAAAABu) >> 1;
        const uint32_t c0 = idx0 - pix0 * CPAD;  // 0 when CPAD is 4
        const uint32_t hp0 = __umulhi(pix0, mul_w) >> shr_w;
        const uint32_t wp0 = pix0 - hp0 * Wp;
        const int32_t s0 = 3 * ((int32_t)(hp0 - border) * (int32_t)W + (int32_t)(wp0 - border)) + (int32_t)c0;
        const int32_t q = s0 >> 2;
        uint32_t d[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            int32_t j = q + k;
            j = j < 0 ? 0 : (j >= nd ? nd - 1 : j);
            d[k] = img[j];
        }
        uint32_t r[ND - 1];
#pragma unroll
        for (int k = 0; k < ND - 1; ++k) r[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], (uint32_t)s0 & 3u);
        out16<T, NE> o;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            uint32_t c, dp;
            if (CPAD == 4) {
                c = e & 3, dp = e >> 2;
            } else {
                const uint32_t ce = c0 + e;  // < 3 + NE
                dp = (ce * 11) >> 5;         // ce / 3 for ce < 32
                c = ce - 3 * dp;
            }
            uint32_t wp = wp0 + dp, hp = hp0;
            if (wp >= Wp) wp -= Wp, hp += 1;
            const uint32_t h = hp - border, w = wp - border;  // wrap = out of range
            const int byte = CPAD == 4 ? 3 * (e >> 2) + ((e & 3) < 3 ? (e & 3) : 2) : e;  // pad channel: any
            float v = 0.f;
            if (c < 3 && h < H && w < W) v = tab[c * 256 + ((r[byte >> 2] >> (8 * (byte & 3))) & 255u)];
            o.set(e, v);
        }
        dst[b * n16 + i] = o.bits();
    }
}

void magic_div(uint32_t d, uint32_t *mul, uint32_t *shr)
{
    uint32_t lg = 0;
    while ((1u << lg) < d) ++lg;
    const uint32_t p = 31 + lg;
    *mul = (uint32_t)(((1ull << p) + d - 1) / d);
    *shr = p - 32;
}

template <typename T, int NE, int CPAD>
void launch_x16(rn_ctx *ctx, const uint8_t *img, void *dst, uint64_t B, uint64_t H, uint64_t W, uint64_t border,
                const norm_t &nm)
{
    const uint64_t Wp = W + 2 * border;
    const uint32_t n16 = (uint32_t)((H + 2 * border) * Wp * CPAD / NE);
    // a block's table costs three elements a thread: with a batch to spread over the CUs a thread
    // takes four stores, a lone image stays as wide as it can be
    const uint32_t steps = B * n16 >= 4u * 256u * 2048u ? 4 : 1;
    uint32_t mw = 0, sw = 0;
    magic_div((uint32_t)Wp, &mw, &sw);
    for (uint64_t b0 = 0; b0 < B; b0 += 65535) {
        const uint64_t nb = (B - b0) < 65535 ? (B - b0) : 65535;
        image_u8_border_x16_kernel<T, NE, CPAD>
            <<<dim3((unsigned)rn_ceil_div(n16, 256 * steps), (unsigned)nb), 256, 0, ctx->stream>>>(
                img + b0 * H * W * 3, (uint4 *)dst + b0 * n16, (uint32_t)H, (uint32_t)W, (uint32_t)border,
                (uint32_t)Wp, n16, steps, mw, sw, nm);
    }
}

}  // namespace

extern "C" {

int rn_image_u8_to_nhwc_pad_dt(rn_ctx *ctx, int dtype, const uint8_t *img, void *dst, uint64_t B, uint64_t H,
                               uint64_t W, uint64_t Cpad, uint64_t border, const float mean[3],
                               const float std[3])
{
    RN_ENTER(ctx);
    RN_REQUIRE(ctx, dtype == RN_DTYPE_F32 || dtype == RN_DTYPE_BF16, "unknown dtype");
    RN_REQUIRE(ctx, Cpad == 3 || Cpad == 4, "Cpad must be 3 or 4");
    RN_REQUIRE(ctx, mean && std, "null mean or std");
    RN_REQUIRE(ctx, H < (1u << 20) && W < (1u << 20) && border < (1u << 10), "dimension too large");
    const uint64_t per_img = (H + 2 * border) * (W + 2 * border) * Cpad;
    const uint64_t total = B * per_img;
    if (total == 0) return RN_OK;
    RN_REQUIRE(ctx, (img || H * W == 0) && dst && (const void *)img != dst, "null or aliased tensor");
    norm_t nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = mean[c], nm.std[c] = std[c];
    const uint64_t ne = dtype == RN_DTYPE_BF16 ? 8 : 4;
    const bool fast = H * W > 0 && (H * W * 3) % 4 == 0 && H * W * 3 < (1ull << 30) && per_img < (1ull << 31) &&
                      per_img % ne == 0 && (border == 0 || border >= 3) && W + 2 * border >= 4 &&
                      (reinterpret_cast<uintptr_t>(img) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    if (fast && dtype == RN_DTYPE_BF16 && Cpad == 4)
        launch_x16<bf16_t, 8, 4>(ctx, img, dst, B, H, W, border, nm);
    else if (fast && dtype == RN_DTYPE_BF16)
        launch_x16<bf16_t, 8, 3>(ctx, img, dst, B, H, W, border, nm);
    else if (fast && Cpad == 4)
        launch_x16<float, 4, 4>(ctx, img, dst, B, H, W, border, nm);
    else if (fast)
        launch_x16<float, 4, 3>(ctx, img, dst, B, H, W, border, nm);
    else if (dtype == RN_DTYPE_BF16)
        image_u8_border_kernel<bf16_t><<<rn_stream_grid(total, 256), 256, 0, ctx->stream>>>(
            img, (bf16_t *)dst, (uint32_t)H, (uint32_t)W, (uint32_t)Cpad, (uint32_t)border, total, nm);
    else
        image_u8_border_kernel<float><<<rn_stream_grid(total, 256), 256, 0, ctx->stream>>>(
            img, (float *)dst, (uint32_t)H, (uint32_t)W, (uint32_t)Cpad, (uint32_t)border, total, nm);
    return rn_after_launch(ctx, "rn_image_u8_to_nhwc_pad_dt");
}

}  // extern "C"
