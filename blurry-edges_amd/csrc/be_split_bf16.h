// Split-bf16 (bf16x6) operand helpers shared by the kernels that multiply fp32 operands on v_mfma_f32_32x32x16_bf16
// (be_wino.hip: k_wino_gemm_ps; be_conv_pm_bf6.hip: k_conv_pm_bf6; be_conv1_pool_bf6.hip: k_conv1_pool_bf6).
//
// x = hi + mid + lo exactly, each a bf16 rounded to nearest-even from what is left: |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x| (finite x
// whose lo stays a bf16 normal, |x| >= ~2^-110; below that lo loses bits to the bf16 subnormal grid, an absolute error < 2^-133).
// A product of two split operands is the six bf16 MFMAs of all pieces but mid.lo, lo.mid, lo.lo (<= 3 x 2^-24 relative), in fp32
// accumulation.  The arithmetic every kernel above keeps, bit for bit (a = the A operand's pieces, b = B's):
//   - per 16-deep K chunk and accumulator the six products in the order a_lo.b_hi, a_hi.b_lo, a_mid.b_mid, a_mid.b_hi, a_hi.b_mid,
//     a_hi.b_hi - the small ones first - each one v_mfma_f32_32x32x16_bf16 into the same fp32 accumulator;
//   - the MFMA's operand map: lane (li = lane & 31, lh = lane >> 5) holds row li's values k = 8 lh .. 8 lh + 7 of the chunk, so a
//     fragment is the two fp32 quads 2 lh and 2 lh + 1 of the row, split by split8 (B: at pack time, k_wino_pack_split);
//   - the K chunks ascending, from a zero accumulator per output tile (a second K segment follows the first).
// Inf / NaN: hi keeps them, x - hi is NaN, so the products stay non-finite.  The residuals are formed with plain
// v_sub_f32: hipcc's SLP pass otherwise packs them into v_pk_add_f32, which beside MFMAs costs more issue than two scalar ops.
#pragma once
#include <hip/hip_runtime.h>

namespace be {
namespace bf6 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ float sub_f32(float x, float y) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
// One pair unit of the split - two neighbouring values -> one packed dword of each plane - in two halves that a loop can place
// separately between its MFMAs (k_wino_gemm_ps, k_conv_pm_bf6: one half per MFMA gap; a half's issue fits under one 32-cycle MFMA):
//   half A (6 VALU): cvt_pk hi, shift, and, two exact v_sub_f32, cvt_pk mid;  it leaves the residuals r0, r1 for half B
//   half B (5 VALU): shift, and, two exact v_sub_f32, cvt_pk lo
// Every split below is built on these two, so the arithmetic exists once.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pair_a(float x0, float x1, unsigned& hu, unsigned& mu, float& r0, float& r1) {
    hu = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){x0, x1}, bf16x2));     // v_cvt_pk_bf16_f32: RNE
    r0 = sub_f32(x0, bf_lo(hu));                                                             // exact
    r1 = sub_f32(x1, bf_hi(hu));
    mu = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){r0, r1}, bf16x2));
}
__device__ __forceinline__ unsigned split_pair_b(float r0, float r1, unsigned mu) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){sub_f32(r0, bf_lo(mu)), sub_f32(r1, bf_hi(mu))}, bf16x2));   // exact
}

// the 8 values of two fp32 quads -> the hi / mid / lo fragments of one 32x32x16 bf16 MFMA operand
__device__ __forceinline__ void split8(f32x4 a, f32x4 b, bf16x8& h, bf16x8& m, bf16x8& l) {
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    u32x4 hu, mu, lu;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float r0, r1;
        unsigned h_, m_;
        split_pair_a(x[2 * u], x[2 * u + 1], h_, m_, r0, r1);
        hu[u] = h_; mu[u] = m_;
        lu[u] = split_pair_b(r0, r1, m_);
    }
    h = __builtin_bit_cast(bf16x8, hu);
    m = __builtin_bit_cast(bf16x8, mu);
    l = __builtin_bit_cast(bf16x8, lu);
}

// the 4 values of one fp32 quad -> 8 bytes of each plane: the same split, for a producer that stores the pieces (k_conv1_pool_bf6)
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void split4(f32x4 a, bf16x4& h, bf16x4& m, bf16x4& l) {
    const float x[4] = {a.x, a.y, a.z, a.w};
    u32x2 hu, mu, lu;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float r0, r1;
        unsigned h_, m_;
        split_pair_a(x[2 * u], x[2 * u + 1], h_, m_, r0, r1);
        hu[u] = h_; mu[u] = m_;
        lu[u] = split_pair_b(r0, r1, m_);
    }
    h = __builtin_bit_cast(bf16x4, hu);
    m = __builtin_bit_cast(bf16x4, mu);
    l = __builtin_bit_cast(bf16x4, lu);
}

// The pre-split weights' block (k_wino_pack_split): per (position, 128-row N tile, 16-deep K chunk) one contiguous 12-KB block
// [plane hi, mid, lo][128 rows][2 x 16 B], the 16-B half h of a row (k = 8 h .. 8 h + 7) at slot h ^ ((row >> 3) & 1).
constexpr int PS_BLOCK = 3 * 128 * 16;                 // bf16 values per block (12 KB)
__device__ __forceinline__ int ps_slot(int row, int half) { return half ^ ((row >> 3) & 1); }

}  // namespace bf6
}  // namespace be
