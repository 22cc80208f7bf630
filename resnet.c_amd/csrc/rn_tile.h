// Device-side pieces every contraction kernel uses (rn_conv.hip, rn_conv_wide.hip, rn_chain.hip,
// rn_conv_group.hip, rn_conv_nchw.hip, rn_stem.hip), included through rn_conv_params.h.  Each of them is
// part of the bit contract between the kernels -- the same k order, the -0.0 neutral shift, one rounding to
// bf16, out-of-range offsets that land as zeros -- and is defined here once.
//
// Index arithmetic, descriptors and the register epilogues are __forceinline__ functions that take and return
// values.  Four pieces are macros (RN_SWZ, RN_STAGE_ACC, RN_EPILOGUE_ROW, RN_WITH_RES_RELU): hipcc's instruction
// order depends on more than the expression -- an out-parameter, an array passed by reference or an extra
// closure reordered or lengthened some kernel -- and every kernel's instruction sequence is held to what the
// written-out text compiled to (tools/isa_text_compare.py --mnemonics, profiles/shared_device_header).  Before
// turning one of them into a function, or changing the signature of a function here, run that comparison.
#ifndef RN_TILE_H
#define RN_TILE_H

#ifdef __HIPCC__

#include <type_traits>

namespace rn_gemm {

// ---- tile order ----

// XCD-aware order: the hardware deals consecutive workgroups round-robin to the 8 XCDs (block v runs on
// XCD v & 7, as its (v >> 3)-th).  The deal gives XCD x a contiguous range of the `total` logical
// indices -- q + 1 of them for the first r = total % 8 XCDs, q = total / 8 for the others -- so that
// neighbours in the logical order share an L2.  Every logical index below `total` is produced by exactly one
// v below `total`, for any total: a bijection.
__device__ __forceinline__ unsigned xcd_deal(unsigned total, unsigned v)
{
    const unsigned q = total >> 3, r = total & 7, xcd = v & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (v >> 3);
}

// nsteps steps over `total` persistent blocks as contiguous ranges, the remainder one each to the first
// blocks: the range of block `logical` (its xcd_deal index, or blockIdx.x where the order does not matter)
__device__ __forceinline__ void dealt_range(unsigned nsteps, unsigned total, unsigned logical, int *count, int *first)
{
    const unsigned base = nsteps / total, rem = nsteps % total;
    *count = (int)(base + (logical < rem ? 1u : 0u));
    *first = (int)(logical * base + min(logical, rem));
}

// ---- index arithmetic ----

// n / d for 0 <= n < 2^31 by the magic numbers of the host's rn_fast_div (rn_conv_params.h), which leaves
// d == 1 (fc, 1x1 outputs) to the kernel: this is that special case
__device__ __forceinline__ unsigned fast_div(unsigned n, int d, unsigned mul, unsigned shr)
{
    return d == 1 ? n : __umulhi(n, mul) >> shr;
}

// output row m -> (image, output row, output column); P: GemmParams, GroupParams
struct OutRow { int b, oh, ow; };
template <typename P>
__device__ __forceinline__ OutRow row_of(int m, const P &p)
{
    const int b = (int)fast_div((unsigned)m, p.HoWo, p.mul_hw, p.shr_hw);
    const int rem = m - b * p.HoWo;
    const int oh = (int)fast_div((unsigned)rem, p.Wo, p.mul_w, p.shr_w);
    return {b, oh, rem - oh * p.Wo};
}

// K tile -> (tap, 128-byte segment of the tap's channels), tap -> (kernel row, kernel column); by value: the
// kernels keep both in scalar registers
struct TapSeg { unsigned tap; int seg; };
struct TapRowCol { int kh, kw; };
template <typename P>
__device__ __forceinline__ TapSeg tap_of(unsigned kt, const P &p)
{
    const unsigned tap = fast_div(kt, p.cseg, p.mul_cs, p.shr_cs);
    return {tap, (int)(kt - tap * (unsigned)p.cseg)};
}
template <typename P>
__device__ __forceinline__ TapRowCol tap_row_col(unsigned tap, const P &p)
{
    const unsigned ukh = fast_div(tap, p.KW, p.mul_kw, p.shr_kw);
    return {(int)ukh, (int)(tap - ukh * (unsigned)p.KW)};
}

// LDS operand image: rows of 128 bytes = eight 16-byte chunks; logical chunk c of row `row` lies in physical
// chunk RN_SWZ(c, row) (and the other way round: an involution), which makes the ds_write_b128 of a staging
// pass, the lane-linear image of an LDS-DMA piece and the ds_read_b128 fragment reads bank-conflict free.
// The swizzle of rows r + 32 i is that of r.  (A macro: as an inline function the fp32 chain kernels came out of
// hipcc six instructions shorter and reordered.)
#define RN_SWZ(chunk, row) ((chunk) ^ (((row) >> 1) & 7))

// ---- buffer descriptors ----

// A byte offset no tensor we accept reaches (>= num_records): the descriptor's range check answers a load
// there with zeros and drops a store, so padding, ragged rows and absent tensors cost a select on the
// offset instead of a branch around the memory operation
constexpr int kOob = (int)0x80000000;
// fourth descriptor word: raw buffer, no swizzle, 32-bit offsets
constexpr int kRawBuffer = 0x00020000;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *ptr, int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(ptr), 0, bytes, kRawBuffer);
}

// ---- diagnostic stamps ----

// Time stamps (100 MHz wall clock) of a block's phases, 16 slots per block; off unless a debug buffer was
// attached to the context.  Nothing but tools/conv_stamps.py reads that buffer.
__device__ __forceinline__ void stamp(unsigned long long *buf, int slot)
{
    if (buf && threadIdx.x == 0) buf[(size_t)blockIdx.x * 16 + slot] = wall_clock64();
}
// ... and of the shader clock (s_memtime), to read the clock the chip holds inside the K loop
__device__ __forceinline__ void stamp_cycles(unsigned long long *buf, int slot)
{
    if (buf && threadIdx.x == 0) buf[(size_t)blockIdx.x * 16 + slot] = __builtin_amdgcn_s_memtime();
}

// ---- tile epilogue (4-wave and 8-wave kernels) ----

typedef float f32x2 __attribute__((ext_vector_type(2)));

// EPT consecutive output elements of one row: load (residual) / store as one 16-byte access
template <typename TO>
struct OutVec;
template <>
struct OutVec<float> {
    static constexpr int EPT = 4;
    static __device__ __forceinline__ void unpack(const u32x4 &x, float (&v)[4])
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(x[j]);
    }
    static __device__ __forceinline__ u32x4 pack(const float (&v)[4])
    {
        return u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    }
    static __device__ __forceinline__ float load1(const void *base, size_t idx) { return static_cast<const float *>(base)[idx]; }
    static __device__ __forceinline__ void store1(void *base, size_t idx, float v) { static_cast<float *>(base)[idx] = v; }
};
template <>
struct OutVec<bf16_t> {
    static constexpr int EPT = 8;
    static __device__ __forceinline__ void unpack(const u32x4 &r, float (&v)[8])
    {
        const bf16x8 x = __builtin_bit_cast(bf16x8, r);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)x[j];
    }
    static __device__ __forceinline__ u32x4 pack(const float (&v)[8])
    {
        bf16x8 x;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (bf16_t)v[j];  // round to nearest even
        return __builtin_bit_cast(u32x4, x);
    }
    static __device__ __forceinline__ float load1(const void *base, size_t idx) { return (float)static_cast<const bf16_t *>(base)[idx]; }
    static __device__ __forceinline__ void store1(void *base, size_t idx, float v) { static_cast<bf16_t *>(base)[idx] = (bf16_t)v; }
};

// One 32x32 MFMA accumulator into the staged fp32 C tile (row pitch BN floats).  C/D map: col = lane & 31,
// row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); dst points at (row 4 * (lane >> 5), col lane & 31) of the
// fragment.  One ds_write_b32 per register puts 32 consecutive columns of two rows, conflict-free.
// (A macro for the reason given at RN_EPILOGUE_ROW: as a function the 224x256 kernel came out reordered.)
#define RN_STAGE_ACC(dst, acc, BN)                                                                  \
    {                                                                                               \
        float *dst_ = (dst);                                                                        \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) dst_[((e & 3) + 8 * (e >> 2)) * (BN)] = (acc)[e]; \
    }

// One epilogue row of a thread, up to the store: declares float v[EPT] and fills it from 16 bytes of the staged
// tile (crow) as y = fma(v, sc, sh) (+ the residual vector resv), ReLU.  EPT is the caller's constant
// OutVec<TO>::EPT.  Two outputs per instruction: v_pk_fma_f32 / v_pk_add_f32 give the IEEE results of fmaf
// and +.  An absent shift is -0.0, not 0.0: the neutral addend that keeps a -0.0 sum -0.0.  The caller rounds
// once, OutVec<TO>::pack(v), and stores.
// A macro, not a function: as a function -- by value, by reference, by pointer, with or without the store -- the
// body came out of hipcc in another instruction order in every 8-wave kernel (profiles/shared_device_header).
#define RN_EPILOGUE_ROW(TO, RES, RELU, crow, resv, sc, sh, v)                                                     \
    float v[EPT], v##_res[EPT];                                                                                   \
    if constexpr (RES) rn_gemm::OutVec<TO>::unpack(resv, v##_res);                                                \
    _Pragma("unroll") for (int j4 = 0; j4 < EPT / 4; ++j4)                                                        \
    {                                                                                                             \
        const float4 x = *reinterpret_cast<const float4 *>((crow) + 4 * j4);                                      \
        v[4 * j4] = x.x, v[4 * j4 + 1] = x.y, v[4 * j4 + 2] = x.z, v[4 * j4 + 3] = x.w;                           \
    }                                                                                                             \
    _Pragma("unroll") for (int j = 0; j < EPT; j += 2)                                                            \
    {                                                                                                             \
        rn_gemm::f32x2 y = __builtin_elementwise_fma(rn_gemm::f32x2{v[j], v[j + 1]}, rn_gemm::f32x2{sc[j], sc[j + 1]}, \
                                                     rn_gemm::f32x2{sh[j], sh[j + 1]});                           \
        if constexpr (RES) y = y + rn_gemm::f32x2{v##_res[j], v##_res[j + 1]};                                    \
        v[j] = RELU ? fmaxf(y[0], 0.f) : y[0];                                                                    \
        v[j + 1] = RELU ? fmaxf(y[1], 0.f) : y[1];                                                                \
    }

// The two launch-uniform switches of an epilogue (residual, ReLU) pick one of four copies of its loop: `call`
// is run with with_res and with_relu naming std::true_type{} or std::false_type{}.  As per-element selects
// the switches cost as many vector instructions as the arithmetic itself.  (A macro for the reason given at
// RN_EPILOGUE_ROW.)
#define RN_WITH_RES_RELU(has_res, relu, call)                          \
    if (has_res) {                                                     \
        if (relu) { std::true_type with_res, with_relu; call; }        \
        else { std::true_type with_res; std::false_type with_relu; call; } \
    } else {                                                           \
        if (relu) { std::false_type with_res; std::true_type with_relu; call; } \
        else { std::false_type with_res, with_relu; call; }            \
    }

// ---- register epilogues (strip and chain kernels: weights are the MFMA's rows) ----

// elements 4j .. 4j+3 of an accumulator are four consecutive channels of one pixel: their channel affine
__device__ __forceinline__ float4 affine4(const f32x16 &acc, int j, const float4 sc, const float4 sh)
{
    return make_float4(fmaf(acc[4 * j], sc.x, sh.x), fmaf(acc[4 * j + 1], sc.y, sh.y), fmaf(acc[4 * j + 2], sc.z, sh.z),
                       fmaf(acc[4 * j + 3], sc.w, sh.w));
}
__device__ __forceinline__ float4 relu4(const float4 v)
{
    return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}
__device__ __forceinline__ float4 affine4_relu(const f32x16 &acc, int j, const float4 sc, const float4 sh)
{
    return make_float4(fmaxf(fmaf(acc[4 * j], sc.x, sh.x), 0.f), fmaxf(fmaf(acc[4 * j + 1], sc.y, sh.y), 0.f),
                       fmaxf(fmaf(acc[4 * j + 2], sc.z, sh.z), 0.f), fmaxf(fmaf(acc[4 * j + 3], sc.w, sh.w), 0.f));
}
// ... with a residual added in fp32 between the affine and the ReLU
__device__ __forceinline__ float4 affine4_add_relu(const f32x16 &acc, int j, const float4 sc, const float4 sh, const float4 r)
{
    return make_float4(fmaxf(fmaf(acc[4 * j], sc.x, sh.x) + r.x, 0.f), fmaxf(fmaf(acc[4 * j + 1], sc.y, sh.y) + r.y, 0.f),
                       fmaxf(fmaf(acc[4 * j + 2], sc.z, sh.z) + r.z, 0.f), fmaxf(fmaf(acc[4 * j + 3], sc.w, sh.w) + r.w, 0.f));
}
// two fp32 -> one dword of bf16, low half first (one rounding to nearest even)
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi)
{
    typedef bf16_t bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 o;
    o[0] = (bf16_t)lo, o[1] = (bf16_t)hi;
    return __builtin_bit_cast(unsigned, o);
}
// four fp32 -> two dwords of bf16, low half first
__device__ __forceinline__ void pack_bf16x4(const float4 v, unsigned (&d)[2])
{
    typedef bf16_t bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 a, b;
    a[0] = (bf16_t)v.x, a[1] = (bf16_t)v.y, b[0] = (bf16_t)v.z, b[1] = (bf16_t)v.w;
    d[0] = __builtin_bit_cast(unsigned, a);
    d[1] = __builtin_bit_cast(unsigned, b);
}

}  // namespace rn_gemm

#endif  // __HIPCC__
#endif
