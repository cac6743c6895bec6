// LocalStage's head in ONE kernel, in split-bf16 (bf16x6) arithmetic: conv1 (7x7, 3 -> 64, padding 3) + folded BatchNorm + Smish +
// MaxPool(3, 2, 1), models/local_stage.py:34-37,42,64-65 - k_conv1_pool (be_conv1_pool.hip) on v_mfma_f32_32x32x16_bf16 (round 11).
//
// What stays from k_conv1_pool: image-major persistent workgroups, two per CU, images dealt round-robin; the image's padded staging
// (21 rows x 28 pixels x 4 channels, be_nchw3_to_nhwc4p_f32) in LDS between three zero rows above and below; a wave owns 32 output
// channels and keeps all their taps in registers for the whole launch; 14 row tiles of 32 pixels x 2 channel tiles per image; bias +
// Smish, the in-register 3-column maxima, the ds_max_f32 pooled cells 80 floats apart, the pooled map written after a barrier with
// the cells going back to -inf; the next image's global loads issued before the tile loop.
// What changes:
//   - the producer of the A operand is this kernel: `stash` splits every staged quad ONCE (be::bf6::split4, the round-to-nearest-even
//     split of split8) into three bf16 planes hi / mid / lo of [27 rows][53 pixels][4 channels]; every value is then read as an MFMA
//     fragment about 14 times (7 kernel rows x 2 channel tiles) with no conversion left in the loop;
//   - the weights are split once per wave at kernel start: chunk (kh, half) of lane (li, lh) = the two quads at
//     w[cout * 224 + kh * 32 + half * 16 + lh * 8 ...]: 14 chunks x 3 planes x 4 registers = 168 VGPRs.  Nothing new is packed;
//   - K chunk (kh, half) = pixels px + 4 half .. + 3 of image row py + kh, four channels each; lane (li, lh) holds k = 8 lh .. 8 lh + 7
//     = pixels px + 4 half + 2 lh and the next: 16 contiguous bytes per plane, 8-byte aligned only (px may be odd): two ds_read_b64.
//     The eighth pixel of a kernel row (half 1, lh 1, second pixel) carries zero weights only: its lanes read a column of zeros
//     instead, so that a non-finite pixel reaches exactly the outputs of its 7 x 7 taps (0 x inf would add a column on the left);
//   - ONE image buffer (three planes are 34 KB; with the 38.7 KB of pooled cells two would not leave two workgroups per CU): the next
//     image is stashed after the barrier that ends the tile loop, beside the pooled-map write; still two barriers per image;
//   - one row tile in flight per wave (a single accumulation chain of this MFMA runs at full rate), the next chunk's fragments read
//     behind the current chunk's MFMAs.
// Arithmetic per output element: a zero accumulator; chunks ascending (kh 0 .. 6, half 0, 1); in each the six products in the project's
// fixed order lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (A = image, B = weights: k_conv_pm_bf6's PA / PB), fp32 accumulation; then
// the bias, Smish, the maxima.  Rows outside the image are multiplied as zeros, not skipped.  An image's bits therefore depend on
// neither the workgroup nor the batch it ran in.  A NaN activation is dropped here as in k_conv1_pool (the maxima start from -inf and
// fmaxf / ds_max_f32 return the other operand), where torch.nn.MaxPool2d propagates it: a network whose conv1 emits NaN is broken
// either way, and the reference's checkpoints do not.
// Synchronisation: plain __syncthreads() hand-overs; no LDS-DMA, no counted vmcnt, no raw barrier.
#include "be_common.h"
#include "be_device_math.h"
#include "be_split_bf16.h"
#include <cstdlib>

namespace {

using be::bf6::bf16x4;
using be::bf6::bf16x8;
using be::bf6::f32x4;
using be::bf6::split4;
using be::bf6::split8;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// a fragment read: volatile, so that the reads stay ds_read_b64 in the order written (the compiler otherwise pairs reads of different
// chunks into ds_read2_b64 - half the rate - and keeps a base register per pair)
typedef const volatile __attribute__((address_space(3))) u32x2* lds_frag_t;

constexpr int R = 21, HW = R * R, WROW = 28, PADR = R + 6, COUT = 64, KTOT = 224, OR_ = 11;
// pixels per image row IN LDS: 53 = 21 + 32.  A fragment read is a ds_read_b64 of 32 consecutive output pixels (8 B each) per half
// wave, banked over 64 dwords = 32 pixels; a tile wraps into the next image row once or twice, and with 53 the LDS pixel index of
// pixel p stays congruent to p modulo 32: conflict-free as one row (37, right for 16-byte pixels, would put the lanes of the next
// row 16 pixels = half a bank row further: 2-way).  Columns 28 .. 52 are never stashed: they stay zero (the eighth tap reads column 28).
constexpr int LROW = 53;
constexpr int PLANE_BYTES = PADR * LROW * 8;           // 11 448: one bf16 plane of the padded image
constexpr int IMG_BYTES = (3 * PLANE_BYTES + 15) / 16 * 16;                      // 34 352
constexpr int IMG_QUADS = R * WROW;                    // 588 float4 of real rows
constexpr int POOL_FLOATS = OR_ * OR_ * COUT;          // 7744: the pooled map
constexpr int CELL = COUT + 16;                        // floats between pooled cells in LDS (be_conv1_pool.hip)
constexpr int POOL_LDS = OR_ * OR_ * CELL;             // 9680
constexpr size_t LDS_BYTES = (size_t)IMG_BYTES + POOL_LDS * sizeof(float);       // 73 072: two workgroups per CU
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
static_assert(3 * PLANE_BYTES + 6 * LROW * 8 + 64 < 65536, "fragment offsets are 16-bit immediates");

__device__ __forceinline__ void lds_fmax(float* p, float v) {
    __builtin_amdgcn_ds_fmaxf((__attribute__((address_space(3))) float*)p, v, __ATOMIC_RELAXED, __MEMORY_SCOPE_WRKGRP, false);
}

__global__ __launch_bounds__(256, 2)
void k_conv1_pool_bf6(const float* __restrict__ x4p, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ y,
                      int64_t n) {
    extern __shared__ __attribute__((aligned(16))) float smem_c1b[];
    char* const img_lds = reinterpret_cast<char*>(smem_c1b);                     // [hi, mid, lo][PADR][LROW][4] bf16
    const __attribute__((address_space(3))) char* const img3 = (const __attribute__((address_space(3))) char*)img_lds;
    float* pool = smem_c1b + IMG_BYTES / 4;            // [11][11][CELL]: running maxima of the image in flight (COUT of every CELL floats used)
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int ntile = wave & 1, mpar = wave >> 1;
    const int cout = ntile * 32 + li;

    // the whole image buffer to zero: the rows above and below the image and the columns right of the staging are never written again
    for (int i = tid; i < IMG_BYTES / 16; i += 256) reinterpret_cast<f32x4*>(img_lds)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the wave's weights, split once: chunk (kh, half) of lane (li, lh) = taps of pixels 4 half + 2 lh, + 1 of kernel row kh, channels 0..3
    bf16x8 bw[14][3];
#pragma unroll
    for (int c = 0; c < 14; ++c) {
        const float* wp = w + (size_t)cout * KTOT + (c >> 1) * 32 + (c & 1) * 16 + lh * 8;
        split8(*reinterpret_cast<const f32x4*>(wp), *reinterpret_cast<const f32x4*>(wp + 4), bw[c][0], bw[c][1], bw[c][2]);
    }
    const float bs = bias ? bias[cout] : 0.0f;
    for (int i = tid; i < POOL_LDS / 4; i += 256) reinterpret_cast<f32x4*>(pool)[i] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};

    int64_t img = blockIdx.x;
    f32x4 pre[3];
    auto fetch = [&](int64_t im) {
        const f32x4* src = reinterpret_cast<const f32x4*>(x4p + im * (int64_t)(R * WROW * 4));
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int q = tid + 256 * j;
            pre[j] = q < IMG_QUADS ? src[q] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int q = tid + 256 * j;
            if (q < IMG_QUADS) {
                bf16x4 h, m, l;
                split4(pre[j], h, m, l);
                char* dst = img_lds + ((q / WROW + 3) * LROW + q % WROW) * 8;    // staging row of 28 pixels -> LDS row of 53
                *reinterpret_cast<bf16x4*>(dst) = h;
                *reinterpret_cast<bf16x4*>(dst + PLANE_BYTES) = m;
                *reinterpret_cast<bf16x4*>(dst + 2 * PLANE_BYTES) = l;
            }
        }
    };
    __syncthreads();                                   // the zeros are below the first image
    if (img < n) { fetch(img); stash(); }
    __syncthreads();

    for (; img < n; img += gridDim.x) {
        const int64_t nxt = img + gridDim.x;
        if (nxt < n) fetch(nxt);                       // the next image's loads fly under this image's MFMAs
        // ---- this wave's 7 row tiles, one at a time: t = mpar + 2 s
#pragma unroll 1
        for (int s = 0; s < 7; ++s) {
            const int t0 = mpar + 2 * s;
            const int p0 = min(t0 * 32 + li, HW - 1);
            const int py0 = (p0 * 3121) >> 16, px0_ = p0 - py0 * R;              // p0 / 21 for p0 < 441
            // byte offsets of the lane's reads in chunk (0, 0) of plane hi: its first pixel; the second of half 0 through a register
            // of its own (two ds_read_b64, not one ds_read2_b64 at half the rate); the second of half 1, which for lh = 1 is the
            // zero column of the same row
            unsigned o0 = (unsigned)((py0 * LROW + px0_ + 2 * lh) * 8);
            unsigned o1 = o0 + 8;
            unsigned o2 = lh ? (unsigned)((py0 * LROW + WROW) * 8) : o0 + 40;
            asm("" : "+v"(o1));
            asm("" : "+v"(o2));
            auto frag = [&](int c, bf16x8 (&f)[3]) {
                const int kh = c >> 1, half = c & 1;
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    const int off = p * PLANE_BYTES + kh * LROW * 8;
                    const u32x2 a = *reinterpret_cast<lds_frag_t>(img3 + o0 + off + half * 32);
                    const u32x2 b = *reinterpret_cast<lds_frag_t>(img3 + (half ? o2 : o1) + off);
                    f[p] = __builtin_bit_cast(bf16x8, (u32x4){a.x, a.y, b.x, b.y});
                }
            };
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            bf16x8 fa[3];
            frag(0, fa);
#pragma unroll
            for (int c = 0; c < 14; ++c) {
                bf16x8 fn[3];
                if (c + 1 < 14) frag(c + 1, fn);       // the next chunk's pieces, under this chunk's MFMAs
                constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};   // lo.hi hi.lo mid.mid mid.hi hi.mid hi.hi
#pragma unroll
                for (int p = 0; p < 6; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA[p]], bw[c][PB[p]], acc, 0, 0, 0);
                if (c + 1 < 14) {
#pragma unroll
                    for (int p = 0; p < 3; ++p) fa[p] = fn[p];
                }
            }
            // D[row][col]: col = lane & 31 (the channel), row = (r & 3) + 8 (r >> 2) + 4 lh (the pixel of the tile): a lane's registers
            // 4 c .. 4 c + 3 are FOUR CONSECUTIVE pixels.  The epilogue of k_conv1_pool: the four pixels of a group in one image row meet
            // three pooled columns - those maxima in registers first, then 3 (6 for odd py) LDS maxima per group.
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const int qb = t0 * 32 + 8 * c4 + 4 * lh;
                if (qb >= HW) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = be::smish(acc[4 * c4 + e] + bs);
                const int py = (qb * 3121) >> 16, px0 = qb - py * R;               // qb / 21 for qb < 441
                if (px0 + 3 < R) {                          // the group stays in its image row (and inside the image: qb + 3 < 441)
                    const int a_ = px0 >> 1;
                    float ma, mb, mc;
                    if (px0 & 1) { ma = v[0]; mb = fmaxf(v[0], fmaxf(v[1], v[2])); mc = fmaxf(v[2], v[3]); }
                    else { ma = fmaxf(v[0], v[1]); mb = fmaxf(v[1], fmaxf(v[2], v[3])); mc = v[3]; }
                    float* c = pool + ((py >> 1) * OR_ + a_) * CELL + cout;
                    lds_fmax(c, ma); lds_fmax(c + CELL, mb); lds_fmax(c + 2 * CELL, mc);
                    if (py & 1) { c += OR_ * CELL; lds_fmax(c, ma); lds_fmax(c + CELL, mb); lds_fmax(c + 2 * CELL, mc); }
                } else {                                    // the group wraps into the next image row / ends with the image: pixel by pixel
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int q = qb + e;
                        if (q >= HW) continue;
                        const int qy = (q * 3121) >> 16, qx = q - qy * R;
                        float* c = pool + ((qy >> 1) * OR_ + (qx >> 1)) * CELL + cout;
                        lds_fmax(c, v[e]);
                        if (qx & 1) lds_fmax(c + CELL, v[e]);
                        if (qy & 1) {
                            lds_fmax(c + OR_ * CELL, v[e]);
                            if (qx & 1) lds_fmax(c + (OR_ + 1) * CELL, v[e]);
                        }
                    }
                }
            }
        }
        __syncthreads();                               // every wave has read the image and sent its maxima
        // ---- the pooled map -> y [img][11][11][64]; the cells go back to -inf; the next image takes the buffer
        float* yo = y + img * (int64_t)POOL_FLOATS;
        for (int i = tid; i < POOL_FLOATS / 4; i += 256) {
            f32x4* cell = reinterpret_cast<f32x4*>(pool + (i >> 4) * CELL) + (i & 15);       // 16 quads of real channels per cell
            reinterpret_cast<f32x4*>(yo)[i] = *cell;
            *cell = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
        if (nxt < n) stash();
        __syncthreads();
    }
}

}  // namespace

bool be::c1_bf6_enabled() {
    // A/B knobs: BE_C1_F32=1 sends only conv1 + pool back to the fp32 routing; BE_WINO_F32=1 restores fp32 everywhere
    static const bool f32 = be::knob_on("BE_C1_F32") || be::knob_on("BE_WINO_F32");
    return !f32;
}

extern "C" int be_conv7x7_pool_bf6_nhwc4p_f32(const float* x4p, int64_t n, const float* packed_w, const float* packed_bias, float* y,
                                              void* stream) {
    BE_REQUIRE(x4p && packed_w && y, "be_conv7x7_pool_bf6_nhwc4p_f32: null pointer");
    BE_REQUIRE(n > 0 && n < ((int64_t)1 << 31), "be_conv7x7_pool_bf6_nhwc4p_f32: n outside (0, 2^31)");
    BE_REQUIRE(be::aligned16(x4p) && be::aligned16(packed_w) && be::aligned16(y), "be_conv7x7_pool_bf6_nhwc4p_f32: 16-byte alignment");
    static be::DeviceFlags attr_set{};
    if (int rc_ = be::ensure_dynamic_lds(reinterpret_cast<const void*>(&k_conv1_pool_bf6), LDS_BYTES, attr_set)) return rc_;
    hipStream_t s = be::as_stream(stream);
    const int cus = be::device_cu_count();
    const unsigned grid = (unsigned)(n < 2 * cus ? n : 2 * cus);      // two workgroups per CU (71 KB of LDS each), images dealt round-robin
    {
        // algorithmic: 2 * M * 147 * 64; executed, as fp32 products: 14 row tiles x 2 channel tiles x 14 chunks of
        // 2 * 32 * 32 * 16 FLOP per image
        const double M = (double)n * HW;
        be::ProfileScope prof(s, BE_KERNEL_CONV1_POOL, 2.0 * M * 147.0 * COUT, 4.0 * (M * 3.0 + 147.0 * COUT + (double)n * OR_ * OR_ * COUT),
                              (double)n * 14.0 * 2.0 * 14.0 * 32768.0);
        hipLaunchKernelGGL(k_conv1_pool_bf6, dim3(grid), dim3(256), LDS_BYTES, s, x4p, packed_w, packed_bias, y, n);
    }
    return be::check_launch("be_conv7x7_pool_bf6_nhwc4p_f32");
}
