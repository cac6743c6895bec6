// Winograd convolution for the 3x3 layers on the 6x6 maps of LocalStage layers 1-3 (models/local_stage.py:20-28, 39-41).
// Tile shape (be_wino_math.h, BE_WINO_TH = 6, the default since round 4): F(6,3) along the rows x F(3,3) along the columns.  A 6x6
// output is TWO tiles of 6x3 outputs; each needs an 8x5 input window (one pixel of zero padding), and
//     Y = A^T [ (G g G^T) o (B^T d B) ] A      summed over the input channels
// turns the convolution into NPOS = 40 independent GEMMs [2N tiles x Cin] x [Cin x Cout] (one per position of the 8x5 transform
// domain): 80 multiplies per (cin, cout) pair and map instead of the 324 of the direct form - 4.05x less work for the matrix
// pipe.  The products are split-bf16 (bf16x6: each fp32 operand split exactly into three bf16 pieces, six bf16 MFMAs per product,
// fp32 accumulation - k_wino_gemm_ps); BE_WINO_F32=1 restores exact fp32 products (the kernels below marked fp32).
// Interpolation points: rows 0, +-1, +-2, +-1/2, inf; columns 0, +-1, 2, inf.
// -DBE_WINO_TH=3 builds rounds 1-3's F(3x3,3x3): four 5x5 tiles per map, 25 GEMMs, 100 multiplies (an A/B target, `make wino3`).
// Accuracy on the whole network against the fp64 oracle: logits 0.9-4.9e-6 over random, trained and stressed weights (5x5 tiles:
// 1.8-3.0e-6; direct fp32 convolutions 1.1-3.3e-6), tolerance 1e-5 - DESIGN.md 3.1 / 4.
//
//   k_wino_pack    weights [Cout,Cin,3,3] (+ folded BatchNorm) -> U [NPOS][Cout_pad][Cin] in the 1x1 layout of k_conv_igemm
//   k_wino_pack_split  U -> its hi / mid / lo bf16 planes behind it, in k_wino_gemm_ps's LDS image (round 8)
//   k_wino_in      x [N,6,6,C] NHWC -> V: tile-major [TPI N][NPOS][C] for large batches, plane-major [NPOS][TPI N][C] for small ones
//                  (HBM-bound: reads 36, writes TPI * NPOS = 80 values per channel)
//   k_wino_gemm_ps M[xi] = V[xi] U[xi]^T for the NPOS positions xi in split-bf16, every batch size (tile-major buffers for large
//                  batches, plane-major for small ones): one workgroup per 128x128 tile walks a group of the positions; A split in
//                  the loop, B's pieces read ready from the planes, a ring of four stages, counted waits
//                  <EPI, 1> (round 9): the same loop as a plain row GEMM on pre-split planes of a packed matrix - LocalStage's 1x1
//                  downsamples (raw accumulators) and fc.1 (bias + Smish), every batch size; BE_ROWS_F32=1: the fp32 kernels
//   k_wino_gemm    fp32 (BE_WINO_F32=1): <0> the same GEMMs for large batches, all positions per workgroup; small ones go through
//                  be_conv_nhwc_batched_f32 on k_conv_igemm, same arithmetic per output element.  <1>: be::gemm_rows
//   k_wino_gemm_ws the fp32 GEMMs weight-stationary (B tile in registers, A streamed through LDS by DMA): batches of >= 4096 maps
//   k_wino_out     M -> y [N,6,6,Cout] + bias (+ residual) (+ Smish)
//   k_wino_out_in  conv1 -> conv2 of a residual block: output transform + Smish + input transform, the map stays in registers
//   k_wino_out_pool2   the last block's output transform with the 2x2 max-pool that follows it
//   All transform kernels are one tile loop per side - wino_out_tiles: M's NPOS values (+ the residual's) -> be::wino_out ->
//   act(o + bias (+ res)) -> the caller's sink; wino_in_tiles: window from the caller's getter -> be::wino_in -> NPOS stores - over
//   one tile (k_wino_in, k_wino_out) or the TPI tiles of a map kept in registers (the others), with wino_strides for both layouts
//   Chained blocks (round 13; be::wino_pair's x_in_v / next_cmid, be_wino_conv3x3_pair_chain_6x6_f32): a block's input transform is
//   written by whatever produced its input map, out of the registers that hold the map, so no block reads its input a second time:
//   k_wino_out_res_in  k_wino_out (+ bias, residual, activation, y stored) + the NEXT block's input transform
//   k_pool_wino_in     max-pool 3/2/1 of [N,11,11,C] (k_maxpool_nhwc's bits) + the input transform of the pooled map
//   The downsample folded (round 14; be::wino_pair's packed_ds, be_wino_conv3x3_pair_ds_6x6_f32): a block's 1x1 downsample is a 3x3
//   with only the centre tap, whose kernel transform is non-zero at (NR - 2) x 3 = 18 of the 40 positions; there conv2's GEMMs run a
//   second K segment over the block's own input transform (k_wino_gemm_ps<0, 0, 1>: M2 = V_h U2^T + V_x U_ds^T - the direct 1x1's
//   multiply count), so the residual tensor [N,6,6,Cout] is neither computed by a row GEMM, nor written, nor read back behind the
//   output transform, and in a chain neither the maps between the blocks nor the pooled map are stored (STORE_Y / STORE_P = 0).
//   k_wino_pack<1> + k_wino_pack_split   the 1x1 kernel through the 3x3 pack's arithmetic: U_ds at its 18 positions, and its planes
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include "be_common.h"
#include "be_device_math.h"
#include "be_split_bf16.h"
#include "be_wino_math.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// tile shape (be_wino_math.h): TH x 3 outputs per tile from an NR x 5 window; TPI tiles per 6x6 map; NPOS positions = GEMMs
constexpr int TH = be::WINO_TH, NR = be::WINO_NR, TPI = be::WINO_TPI, NPOS = be::WINO_NPOS, NOUT = be::WINO_OUT;

inline unsigned grid_cap(int64_t total, int block, int64_t limit = 65535) {
    int64_t g = (total + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : (g > limit ? limit : g));
}

// A 1x1 convolution is a 3x3 with only the centre tap, and the middle column of G is zero at the points 0 and inf: its kernel
// transform lives on the (NR - 2) x 3 positions z = 5 zr + zc with 0 < zr < NR - 1, 0 < zc < 4 (18 of the 40) - the positions at
// which conv2's GEMMs take a block's 1x1 downsample as a second K segment (round 14).  Live position z is number wino_ds_index(z).
constexpr int NLIVE = (NR - 2) * 3;
constexpr bool wino_ds_live(int z) { return z / 5 > 0 && z / 5 < NR - 1 && z % 5 > 0 && z % 5 < 4; }
constexpr int wino_ds_index(int z) { return 3 * (z / 5 - 1) + z % 5 - 1; }
constexpr uint64_t wino_ds_mask() {
    uint64_t m = 0;
    for (int z = 0; z < NPOS; ++z)
        if (wino_ds_live(z)) m |= (uint64_t)1 << z;
    return m;
}

// DS = 1: w is a 1x1 kernel [Cout,Cin], taken as the centre tap of a 3x3 through the same arithmetic (the dead positions come out
// as exact zeros and are not stored): U [NLIVE][Cout_pad][Cin]
template <int DS>
__global__ void k_wino_pack(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma,
                            const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
                            float eps, int cout, int cin, int cout_pad, float* __restrict__ U, float* __restrict__ bias) {
    const int64_t total = (int64_t)cout_pad * cin;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        const int co = (int)(idx / cin), ci = (int)(idx % cin);
        float u[NR][5];
        if (co < cout) {
            const float scale = gamma ? gamma[co] / sqrtf(var[co] + eps) : 1.0f;
            const float* g = w + ((size_t)co * cin + ci) * (DS ? 1 : 9);
            float t[NR][3];                                 // G_rows g: the kernel's three rows -> NR transform rows, column by column
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float col[NR];
                if constexpr (DS) be::wino_g_rows(0.0f, c == 1 ? g[0] * scale : 0.0f, 0.0f, col);     // the centre tap alone
                else be::wino_g_rows(g[c] * scale, g[3 + c] * scale, g[6 + c] * scale, col);
#pragma unroll
                for (int r = 0; r < NR; ++r) t[r][c] = col[r];
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) be::wino_g5(t[r][0], t[r][1], t[r][2], u[r]);     // (G_rows g) G^T
        } else {
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int c = 0; c < 5; ++c) u[r][c] = 0.0f;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                if constexpr (DS) {
                    if (wino_ds_live(5 * r + c)) U[(size_t)wino_ds_index(5 * r + c) * total + idx] = u[r][c];
                } else {
                    U[(size_t)(5 * r + c) * total + idx] = u[r][c];
                }
            }
    }
    if (DS && !bias) return;                                // (the folded bias of a block's downsample is kept elsewhere)
    for (int64_t co = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; co < cout_pad; co += gs) {
        float v = 0.0f;
        if (co < cout) {
            const float bb = b ? b[co] : 0.0f;
            v = gamma ? (bb - mean[co]) * (gamma[co] / sqrtf(var[co] + eps)) + beta[co] : bb;
        }
        bias[co] = v;
    }
}

// streaming load of the transform kernels, which read every byte once: non-temporal loads move 5.42-5.46 TB/s where plain loads
// move 5.24-5.28 (2.65 -> 2.56 ms of transforms per step).  Their stores are plain: non-temporal stores had no effect, and the
// max-pool, whose windows overlap, loses a third with them.
template <class V> __device__ __forceinline__ V ld_s(const V* p) { return __builtin_nontemporal_load(p); }

// channels per thread of the output-side transform kernels: with the 8x5 tiles a thread holding a channel QUAD needs 40 + 18 + 18
// float4 values live (304 registers: the compiler parked 64-130 of them in AGPRs and the kernels fell to 4.9 TB/s); a channel
// PAIR per thread needs half and runs two waves per SIMD.  Per-channel arithmetic: the width changes no bit.
constexpr int VW_OUT = TH == 6 ? 2 : 4;
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int W> struct VecOf;
template <> struct VecOf<4> { typedef f32x4 type; };
template <> struct VecOf<2> { typedef f32x2 type; };

// The two layouts of a transform-domain buffer (V or M) of n maps x c channels: plane-major [NPOS][TPI n][c] for small batches,
// tile-major [TPI n][NPOS][c] for large ones (a tile's NPOS x c block is one contiguous piece of HBM for the transform kernels).
// plane / ts: elements between the positions of a tile / between tiles.  The kernels count in channel vectors (c = c4), the host,
// for the GEMMs' arguments, in floats.
struct WinoStrides { int64_t plane, ts; };
__host__ __device__ __forceinline__ WinoStrides wino_strides(int tm, int64_t n, int c) {
    return {tm ? c : n * TPI * c, tm ? NPOS * c : c};
}

// channel vector cq of pixel (row, col) of map img in [N,6,6,C]: where the residual is read and y is written
__device__ __forceinline__ size_t map_at(int64_t img, int row, int col, int c4, int cq) {
    return ((size_t)img * 36 + row * 6 + col) * c4 + cq;
}

// the activation of a tile's N values under ONE test of `act` (per value, the test and its branches cost the chained kernels a
// reload of the spilled kernel arguments at every pixel)
template <class V, int N>
__device__ __forceinline__ void wino_act(V (&v)[N], int act) {
    constexpr int W = (int)(sizeof(V) / sizeof(float));
    if (act == 1) {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int k = 0; k < W; ++k) v[i][k] = be::smish(v[i][k]);
    } else if (act == 2) {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int k = 0; k < W; ++k) v[i][k] = fmaxf(v[i][k], 0.f);
    }
}

// The tile loop of the input side: NTILES tiles of a 6x6 map from its tile t0 on (tile t is (ty, tx) = (t >> 1, t & 1)).  Per tile the
// NR x 5 window with one pixel of zero padding (get(yy, xx): the map's pixel, asked for inside the map only), be::wino_in
// (be_wino_math.h), and the NPOS stores from dst() on: tile t0's first position, this thread's channel vector - asked for once the
// values are there, so that a kernel which forms that address for the call does not hold it across the transform (k_wino_in needs
// every one of its 256 registers for two waves per SIMD).
template <int NTILES, class V, class Get, class Dst>
__device__ __forceinline__ void wino_in_tiles(int t0, WinoStrides so, Get get, Dst dst) {
    const V zero = V(0.f);
#pragma unroll
    for (int t = 0; t < NTILES; ++t) {
        const int ty = (t0 + t) >> 1, tx = (t0 + t) & 1;
        V d[NR][5], v[NPOS];
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                const int yy = TH * ty - 1 + r, xx = 3 * tx - 1 + c;
                d[r][c] = ((unsigned)xx < 6u && (unsigned)yy < 6u) ? get(yy, xx) : zero;
            }
        be::wino_in(d, v);
#pragma unroll
        for (int z = 0; z < NPOS; ++z) *(dst() + t * so.ts + (size_t)z * so.plane) = v[z];
    }
}

// input transform of map img held in registers (the kernels below that keep one): the TPI x NPOS values of its tiles go to channel
// vector cq of the image's tiles in the buffer Vb
template <class V>
__device__ __forceinline__ void wino_in_map(const V y[6][6], V* Vb, int64_t img, int cq, WinoStrides so) {
    V* dst = Vb + img * TPI * so.ts + cq;
    wino_in_tiles<TPI, V>(0, so, [&](int yy, int xx) { return y[yy][xx]; }, [&] { return dst; });
}

// The tile loop of the output side: NTILES tiles of map img from its tile t0 on.  Per tile the NPOS transform-domain values of M,
// be::wino_out, act(o + bias (+ res)) for the tile's TH x 3 pixels - the bias, the residual and the activation each in one pass over
// the tile, so `res` and `act` are tested once per tile - and sink(row, col, value) for each of them.  That operation order is
// what every kernel below computes: a block's y and the transform of it carry the same bits whichever of them writes them
// (tests/test_wino_chain.py).  The residual's values are fetched with the tile's transform-domain ones (inside the output loop
// each was a round trip of its own: k_wino_out sat 58 % of its wave cycles in s_waitcnt).
template <int NTILES, class vec, class Sink>
__device__ __forceinline__ void wino_out_tiles(int t0, const vec* M, WinoStrides sm, vec bv, const vec* res, int64_t img, int c4, int cq,
                                               int act, Sink sink) {
#pragma unroll
    for (int t = 0; t < NTILES; ++t) {
        const int ty = (t0 + t) >> 1, tx = (t0 + t) & 1;
        const vec* src = M + (img * TPI + t0 + t) * sm.ts + cq;
        vec m[NPOS], o[NOUT], rv[NOUT];
#pragma unroll
        for (int z = 0; z < NPOS; ++z) m[z] = ld_s(src + (size_t)z * sm.plane);
        if (res) {
#pragma unroll
            for (int r = 0; r < TH; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) rv[3 * r + c] = ld_s(res + map_at(img, TH * ty + r, 3 * tx + c, c4, cq));
        }
        be::wino_out(m, o);
#pragma unroll
        for (int k = 0; k < NOUT; ++k) o[k] = o[k] + bv;
        if (res) {
#pragma unroll
            for (int k = 0; k < NOUT; ++k) o[k] += rv[k];
        }
        wino_act(o, act);
#pragma unroll
        for (int r = 0; r < TH; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) sink(TH * ty + r, 3 * tx + c, o[3 * r + c]);
    }
}

// the 6x6 map of image img out of its TPI tiles of M, into registers (one thread = one image x one channel vector), and with
// STORE_Y also to y [N,6,6,C]
template <int STORE_Y, class vec>
__device__ __forceinline__ void wino_out_map(const vec* M, WinoStrides sm, vec bv, const vec* res, vec* y, int64_t img, int c4, int cq,
                                             int act, vec v[6][6]) {
    wino_out_tiles<TPI>(0, M, sm, bv, res, img, c4, cq, act, [&](int row, int col, vec w) {
        v[row][col] = w;
        if constexpr (STORE_Y) *(y + map_at(img, row, col, c4, cq)) = w;
    });
}

// one thread = one tile (patch, ty, tx) x one channel quad
// Compiler report (gfx950, hipcc -Rpass-analysis=kernel-resource-usage; in all six kernels 0 AGPRs, scratch 0, no VGPR spills, the
// SGPR spills go to VGPR lanes: the addresses): 254 VGPRs, 15 SGPR spills, two waves per SIMD.
__global__ __launch_bounds__(256)
void k_wino_in(const float* __restrict__ x, float* __restrict__ V, int64_t n, int c4, int tm) {
    const int64_t total = n * TPI * c4;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const WinoStrides sv = wino_strides(tm, n, c4);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        const int cq = (int)(idx % c4);
        const int64_t tile = idx / c4;
        const int64_t img = tile / TPI;
        const int tt = (int)(tile - img * TPI);
        const f32x4* src = reinterpret_cast<const f32x4*>(x) + img * 36 * c4 + cq;
        wino_in_tiles<1, f32x4>(tt, sv, [&](int yy, int xx) { return ld_s(src + (size_t)(yy * 6 + xx) * c4); },
                                [&] { return reinterpret_cast<f32x4*>(V) + tile * sv.ts + cq; });
    }
}

// one thread = one tile x one channel vector
// Compiler report: 163 VGPRs, 32 SGPR spills, three waves per SIMD.
template <int VW = VW_OUT>
__global__ __launch_bounds__(256)
void k_wino_out(const float* __restrict__ M, const float* __restrict__ bias, const float* __restrict__ res,
                float* __restrict__ y, int64_t n, int c4, int act, int tm) {
    typedef typename VecOf<VW>::type vec;
    const int64_t total = n * TPI * c4;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const WinoStrides sm = wino_strides(tm, n, c4);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        const int cq = (int)(idx % c4);
        const int64_t tile = idx / c4;
        const int64_t img = tile / TPI;
        const int tt = (int)(tile - img * TPI);
        wino_out_tiles<1>(tt, reinterpret_cast<const vec*>(M), sm, reinterpret_cast<const vec*>(bias)[cq], reinterpret_cast<const vec*>(res),
                          img, c4, cq, act, [&](int row, int col, vec w) { *(reinterpret_cast<vec*>(y) + map_at(img, row, col, c4, cq)) = w; });
    }
}

// conv1 -> conv2 of a residual block without the intermediate map in HBM: one thread = one image x one channel vector reads the
// TPI x NPOS transform-domain values of conv1's result, forms the 6x6 map (+ bias, Smish) in registers and writes the TPI x NPOS
// transform-domain values conv2's GEMMs read.  Saves the 36 values written and re-read (tile overlap) per channel.
// M as conv1's GEMMs wrote it (tm_in), V as conv2's GEMMs read it (tm_out).
// Compiler report: 173 VGPRs, 634 SGPR spills, two waves per SIMD.
template <int VW = VW_OUT>
__global__ __launch_bounds__(256, VW_OUT == 2 ? 2 : 1)
void k_wino_out_in(const float* __restrict__ M, const float* __restrict__ bias, float* __restrict__ V, int64_t n, int c4, int act,
                   int tm_in, int tm_out) {
    typedef typename VecOf<VW>::type vec;
    const int64_t total = n * c4;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const WinoStrides sm = wino_strides(tm_in, n, c4), sv = wino_strides(tm_out, n, c4);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        const int cq = (int)(idx % c4);
        const int64_t img = idx / c4;
        vec v[6][6];
        wino_out_map<0>(reinterpret_cast<const vec*>(M), sm, reinterpret_cast<const vec*>(bias)[cq], (const vec*)nullptr, (vec*)nullptr,
                        img, c4, cq, act, v);
        wino_in_map(v, reinterpret_cast<vec*>(V), img, cq, sv);
    }
}

// Block boundary (round 13): conv2's output transform + bias + residual + activation, the store of y [N,6,6,C] (the next block's
// 1x1 downsample reads it) AND the next block's input transform of that map out of the same registers - k_wino_out followed by
// k_wino_in without k_wino_in's read of y (36 values per channel and map) and without its launch.  M in the layout conv2's GEMMs
// wrote (tm_in), V in the one the next block's conv1 GEMMs read (tm_out).
// STORE_Y = 0 (round 14, a chained block whose successor folds its downsample into conv2's GEMMs): nothing reads y, it is not stored.
// Compiler report: STORE_Y = 1: 189 VGPRs, 187 SGPR spills; STORE_Y = 0: 244 VGPRs, 642 SGPR spills; two waves per SIMD both.
template <int VW = VW_OUT, int STORE_Y = 1>
__global__ __launch_bounds__(256, VW_OUT == 2 ? 2 : 1)
void k_wino_out_res_in(const float* __restrict__ M, const float* __restrict__ bias, const float* __restrict__ res,
                       float* __restrict__ y, float* __restrict__ V, int64_t n, int c4, int act, int tm_in, int tm_out) {
    typedef typename VecOf<VW>::type vec;
    const int64_t total = n * c4;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const WinoStrides sm = wino_strides(tm_in, n, c4), sv = wino_strides(tm_out, n, c4);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        const int cq = (int)(idx % c4);
        const int64_t img = idx / c4;
        vec v[6][6];
        wino_out_map<STORE_Y>(reinterpret_cast<const vec*>(M), sm, reinterpret_cast<const vec*>(bias)[cq], reinterpret_cast<const vec*>(res),
                              reinterpret_cast<vec*>(y), img, c4, cq, act, v);
        wino_in_map(v, reinterpret_cast<vec*>(V), img, cq, sv);
    }
}

// The max-pool 3/2/1 between layer0 and layer1 + layer1's input transform (round 13): one thread = one image x one channel vector
// reads [N,11,11,C] row by row (three input rows live: output row oy takes rows 2 oy - 1 .. 2 oy + 1, the last of them is the next
// output row's first), writes the pooled [N,6,6,C] (layer1's 1x1 downsample reads it) and the TPI x NPOS transform-domain values of
// that map.  The pooled values are k_maxpool_nhwc's bit for bit: its fold - from -inf over the nine taps, rows outer, columns inner,
// a tap outside the map replaced by the nearest one inside (taken twice) - so signed zeros, infinities and dropped NaNs come out
// as there.  Every input byte is read once, so the loads stream like the other transforms'.
// STORE_P = 0 (round 14): the pooled map is not stored (layer1 folds its downsample into conv2's GEMMs: nothing reads it).
// Compiler report: STORE_P = 1: 126 VGPRs, 90 SGPR spills, four waves per SIMD; STORE_P = 0: 162 VGPRs, 88 SGPR spills, three.
template <int VW = VW_OUT, int STORE_P = 1>
__global__ __launch_bounds__(256, VW_OUT == 2 ? 2 : 1)
void k_pool_wino_in(const float* __restrict__ x, float* __restrict__ pooled, float* __restrict__ V, int64_t n, int c4, int tm_out) {
    typedef typename VecOf<VW>::type vec;
    const int64_t total = n * c4;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const WinoStrides sv = wino_strides(tm_out, n, c4);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        const int cq = (int)(idx % c4);
        const int64_t img = idx / c4;
        const vec* src = reinterpret_cast<const vec*>(x) + img * 121 * c4 + cq;
        vec p[6][6], row[3][11];                       // row[0..2]: input rows 2 oy - 1, 2 oy, 2 oy + 1, clamped into the map
#pragma unroll
        for (int oy = 0; oy < 6; ++oy) {
#pragma unroll
            for (int c = 0; c < 11; ++c) {
                row[0][c] = oy ? row[2][c] : ld_s(src + (size_t)c * c4);
                row[1][c] = oy ? ld_s(src + (size_t)(22 * oy + c) * c4) : row[0][c];
            }
#pragma unroll
            for (int c = 0; c < 11; ++c) row[2][c] = oy < 5 ? ld_s(src + (size_t)(22 * oy + 11 + c) * c4) : row[1][c];
#pragma unroll
            for (int ox = 0; ox < 6; ++ox) {
                vec m = vec(-INFINITY);
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int xx = 2 * ox - 1 + dx < 0 ? 0 : (2 * ox - 1 + dx > 10 ? 10 : 2 * ox - 1 + dx);
#pragma unroll
                        for (int k = 0; k < VW; ++k) m[k] = fmaxf(m[k], row[dy][xx][k]);
                    }
                p[oy][ox] = m;
                if constexpr (STORE_P) *(reinterpret_cast<vec*>(pooled) + map_at(img, oy, ox, c4, cq)) = m;
            }
        }
        wino_in_map(p, reinterpret_cast<vec*>(V), img, cq, sv);
    }
}

// Last block of LocalStage: output transform + bias + residual + activation + the 2x2 max-pool that follows it
// (models/local_stage.py:42,67: maxpool after layer3), one thread per image and channel vector: the 6x6 map exists only in
// registers, [N,3,3,C] is written (saves the map's round trip through HBM and the pooling launch).
// Compiler report: 241 VGPRs, 265 SGPR spills, two waves per SIMD.
template <int VW = VW_OUT>
__global__ __launch_bounds__(256, VW_OUT == 2 ? 2 : 1)
void k_wino_out_pool2(const float* __restrict__ M, const float* __restrict__ bias, const float* __restrict__ res,
                      float* __restrict__ y, int64_t n, int c4, int act, int tm) {
    typedef typename VecOf<VW>::type vec;
    const int64_t total = n * c4;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const WinoStrides sm = wino_strides(tm, n, c4);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        const int cq = (int)(idx % c4);
        const int64_t img = idx / c4;
        vec v[6][6];
        wino_out_map<0>(reinterpret_cast<const vec*>(M), sm, reinterpret_cast<const vec*>(bias)[cq], reinterpret_cast<const vec*>(res),
                        (vec*)nullptr, img, c4, cq, act, v);
#pragma unroll
        for (int py = 0; py < 3; ++py)
#pragma unroll
            for (int px = 0; px < 3; ++px) {
                vec m;
#pragma unroll
                for (int k = 0; k < VW; ++k)
                    m[k] = fmaxf(fmaxf(v[2 * py][2 * px][k], v[2 * py][2 * px + 1][k]), fmaxf(v[2 * py + 1][2 * px][k], v[2 * py + 1][2 * px + 1][k]));
                *(reinterpret_cast<vec*>(y) + ((size_t)img * 9 + py * 3 + px) * c4 + cq) = m;
            }
    }
}

// ---- the 25 transform-domain GEMMs of one (M tile, N tile), walked by ONE workgroup --------------------------------
// M[z] = V[z] U[z]^T for z = 0..24: each problem has a K loop of only Cin/16 = 6-24 chunks, so as separate tiles every
// 12.6 MFLOP pay a prologue (first loads exposed), an epilogue and a workgroup turnover.  Here the software pipeline runs
// straight through the problem boundaries; at a boundary the accumulators are stored raw (no bias / residual / activation:
// the output transform does those) and cleared.  128x128 tile, 2x2 waves of 2x2 MFMA tiles (32x32x2 f32).
//
// Operand staging is global -> LDS directly (global_load_lds_dwordx4: no VGPR round trip, no ds_write, no per-chunk vector
// address arithmetic).  Knock-out runs of the register-staged version (tools/wino_gemm_lab.hip) showed that
// the MFMA pipe loses about as many cycles as the other instructions of the resident waves move registers: a loop of
// nothing but MFMAs runs at 99 % of the matrix rate, + the fragment ds_reads 94 %, + ds_writes 91 %, + global loads into
// registers 80 %; barriers and load latency cost nothing measurable.  So the loop carries as little else as it can.
// One DMA instruction of a wave fills a 1-KB piece = 16 rows x 64 B, lane-linear (LDS destination = piece base + lane x
// 16); without row padding the fragment reads would be 4-way bank conflicts, so the 16-byte quads of a row are
// XOR-swizzled by (row >> 2) & 3 - on the SOURCE address of the DMA and on the ds_read_b128 of the fragments
// (conflict-free for the four 16-lane groups of that instruction).  Rows past M load a valid row and are never stored.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

struct GemmArgs {
    const float* x;       // problem z: rows [M][K] at x + z * xb
    const float* w;       //            [Npad][K] at w + z * wb
    float* y;             //            [M][ldy] at y + z * yb
    int M, K, N, ldy, nb, m_tiles, n_tiles;
    int64_t xb, wb, yb;
    int lda;              // floats between rows of x (K for a plain matrix; 25 K for the tile-major Winograd V [4n][25][K])
    // the same kernel as a plain row GEMM (1x1 convolutions, linears: EPI = 1): the "problems" a workgroup walks are nb
    // consecutive 128-row tiles of ONE matrix (short K loops get the same continuous pipeline): mrows = 128 nb rows per
    // workgroup, zrows = 128 rows per problem, xb = 128 K, yb = 128 ldy, wb = 0.  Winograd: mrows = 128, zrows = 0.
    int mrows, zrows;
    const float* bias;    // EPI = 1: y = act(acc + bias[col] (+ res[row][col]))
    const float* res;     //          same row stride as y
    int act;
    int zgroups;          // k_wino_gemm_ps: problem groups (one workgroup per M tile x N tile x group walks ceil(nb / zgroups) problems;
                          // every output element sees the same K loop, so the group count changes no bit)
    int npad;             // k_wino_gemm_ps: rows of w's planes, 128 n_tiles (zero past Npad): every B piece a tile fetches exists
    // k_wino_gemm_ps<0, 0, 1> (round 14): a second K segment at the positions of the mask zext - problem z accumulates x[z] w[z]^T
    // over K and then, where bit z is set, x2[z] w2[e]^T over 16 kext more (e: the number of set bits below z), into one accumulator.
    const float* x2;      // rows [M][16 kext] at x2 + z * xb2, lda2 floats between rows
    const float* w2;      // the planes of the extended positions only, wb2 floats per position
    int64_t xb2, wb2;
    int lda2, kext;
    uint64_t zext;
    uint64_t ztab[4];     // the walk: group g takes the positions number g zper .. of this table, 6 bits each, ten to a word
};

// ---- split-bf16 operands --------------------------------------------------------------------------------------------------------
// x = hi + mid + lo, the six products per K chunk and split8: be_split_bf16.h (shared with be_conv_pm_bf6.hip)
using be::bf6::bf16x8;
using be::bf6::u32x4;
using be::bf6::split8;
using be::bf6::PS_BLOCK;
using be::bf6::ps_slot;

// ---- the weights pre-split (round 8) -------------------------------------------------------------------------------------------
// k_wino_pack_split writes the hi / mid / lo pieces of U behind it, formed by split8 - as k_wino_gemm_ps forms A's in
// registers - in the image k_wino_gemm_ps's LDS stage holds: per (position, 128-row N tile, 16-deep K chunk) one contiguous 12-KB
// block [plane hi, mid, lo][128 rows][2 x 16 B], the 16-B half h of a row (k = 8 h .. 8 h + 7) at slot h ^ ((row >> 3) & 1).  With
// the swap a ds_read_b128 of one half for 32 rows puts each 16-lane group (rows 0-3, 12-15, 20-27 / 4-11, 16-19, 28-31) on 16
// distinct 16-B slots of the 256-B bank row: conflict-free.  Rows from cout_pad up to the 128-row tile are zero.
// (PS_BLOCK = 3 * 128 * 16 bf16 values per block and ps_slot: be_split_bf16.h)
constexpr int PS_STAGES = 4;                           // k_wino_gemm_ps's LDS ring: 4 x 20 KB, two workgroups per CU (160 KB)

__global__ void k_wino_pack_split(const float* __restrict__ U, int npos, int cout_pad, int cin, int n_tiles, __bf16* __restrict__ P) {
    const int kg = cin / 8, rows = 128 * n_tiles;      // one thread = one (position, row, 8-deep K group); a plain matrix is npos = 1
    const int64_t total = (int64_t)npos * rows * kg;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        const int g = (int)(idx % kg), row = (int)((idx / kg) % rows), z = (int)(idx / ((int64_t)kg * rows));
        f32x4 lo4 = {0.f, 0.f, 0.f, 0.f}, hi4 = lo4;
        if (row < cout_pad) {
            const f32x4* src = reinterpret_cast<const f32x4*>(U + ((size_t)z * cout_pad + row) * cin + 8 * g);
            lo4 = src[0];
            hi4 = src[1];
        }
        bf16x8 h, m, l;
        split8(lo4, hi4, h, m, l);
        const int r = row & 127;
        bf16x8* dst = reinterpret_cast<bf16x8*>(P + ((size_t)(z * n_tiles + (row >> 7)) * (cin / 16) + (g >> 1)) * PS_BLOCK) + 2 * r +
                      ps_slot(r, g & 1);
        dst[0] = h;
        dst[256] = m;                                  // (planes 128 rows x 2 halves of 16 B apart)
        dst[512] = l;
    }
}

// EPI: 0 = raw Winograd problems, 1 = row GEMM with bias / residual / activation.
template <int EPI>
__global__ __launch_bounds__(256, 3)
void k_wino_gemm(GemmArgs a) {
    constexpr int BM = 128, BN = 128, BKT = 16;
    constexpr int STAGE = (BM + BN) * BKT;             // floats per stage: A 128 x 16, then B 128 x 16 (16 KB)
    extern __shared__ __attribute__((aligned(16))) float smem_w[];
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;          // all N tiles of an M tile on one XCD
    const int n_tile = slot % a.n_tiles;
    const int m_tile = (slot / a.n_tiles) * 8 + xcd;
    if (m_tile >= a.m_tiles) return;
    const int n0 = n_tile * BN, row_base = m_tile * a.mrows;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    // staging: wave w fills pieces 2w, 2w+1 of the A tile and of the B tile; lane -> (row = lane >> 2, slot = lane & 3),
    // and fetches the quad that belongs into that slot after the swizzle
    const int srow = lane >> 2, sq = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned a_off[2], b_off[2];                       // byte offsets from the tile's first row (tiles span < 2^31 bytes)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = (2 * wave + p) * 16 + srow;
        // (walked tiles, zrows > 0, are launched only when every tile is full: M % (128 nb) == 0)
        a_off[p] = (unsigned)((row_base + r < a.M ? r : 0) * a.lda + 4 * sq) * 4u;
        b_off[p] = (unsigned)(r * a.K + 4 * sq) * 4u;  // rows up to Npad exist (zero rows past N)
    }
    const float* xt = a.x + (int64_t)row_base * a.lda; // uniform
    const float* wt = a.w + (int64_t)n0 * a.K;
    const int kchunks = a.K / BKT, total = kchunks * a.nb;
    // fragment reads: row = 64 wm + 32 i + li, quad (lh + 2 g) ^ ((li >> 2) & 3)
    const int fsw = (li >> 2) & 3;
    const int q0 = lh, q1 = lh + 2;
    const int a_fr0 = (wm * 64 + li) * BKT + 4 * (q0 ^ fsw);
    const int a_fr1 = (wm * 64 + li) * BKT + 4 * (q1 ^ fsw);
    const int b_fr0 = BM * BKT + (wn * 64 + li) * BKT + 4 * (q0 ^ fsw);
    const int b_fr1 = BM * BKT + (wn * 64 + li) * BKT + 4 * (q1 ^ fsw);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    int lz = 0, lk = 0;                                // (problem, chunk) of the next load, advanced incrementally
#define WG_LOAD(BUF)                                                                                            \
    do {                                                                                                        \
        const char* xs_ = reinterpret_cast<const char*>(xt + (int64_t)lz * a.xb + lk * BKT);                     \
        const char* ws_ = reinterpret_cast<const char*>(wt + (int64_t)lz * a.wb + lk * BKT);                     \
        float* st_ = smem_w + (BUF) * STAGE + (2 * wave) * 256;                                                 \
        _Pragma("unroll") for (int p_ = 0; p_ < 2; ++p_) {                                                      \
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(xs_ + a_off[p_]), (lds_ptr_t)(st_ + p_ * 256), 16, 0, 0);            \
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(ws_ + b_off[p_]), (lds_ptr_t)(st_ + BM * BKT + p_ * 256), 16, 0, 0); \
        }                                                                                                       \
        if (lk + 1 < kchunks) ++lk; else if (lz + 1 < a.nb) { lk = 0; ++lz; }   /* past the end: the last chunk again */ \
    } while (0)
    const unsigned y_off = (unsigned)((wm * 64 + 4 * lh) * a.ldy + wn * 64 + li) * 4u;
    float bias_v[2] = {0.f, 0.f};
    if (EPI) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = n0 + wn * 64 + j * 32 + li;
            bias_v[j] = (a.bias && c < a.N) ? a.bias[c] : 0.0f;
        }
    }
    WG_LOAD(0);
    __syncthreads();                                   // (hipcc drains the DMA with vmcnt(0) before the barrier)
    int cz = 0, ck = 0;                                // (problem, chunk) being multiplied
    for (int kc = 0; kc < total; ++kc) {
        const int buf = kc & 1;
        WG_LOAD(buf ^ 1);                              // everyone left that buffer at the barrier of the last iteration
        __builtin_amdgcn_sched_barrier(0);
        {
            const float* sb = smem_w + buf * STAGE;
            f32x4 af[2][2], bf[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[0][i] = *reinterpret_cast<const f32x4*>(sb + a_fr0 + i * 32 * BKT);
                bf[0][i] = *reinterpret_cast<const f32x4*>(sb + b_fr0 + i * 32 * BKT);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[1][i] = *reinterpret_cast<const f32x4*>(sb + a_fr1 + i * 32 * BKT);
                bf[1][i] = *reinterpret_cast<const f32x4*>(sb + b_fr1 + i * 32 * BKT);
            }
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g][i].x, bf[g][j].x, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g][i].y, bf[g][j].y, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g][i].z, bf[g][j].z, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g][i].w, bf[g][j].w, acc[i][j], 0, 0, 0);
                    }
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        if (++ck == kchunks) {                          // problem cz is complete: store, clear
            const int zrow = row_base + cz * a.zrows;
            const int64_t yo = (int64_t)cz * a.yb + (int64_t)row_base * a.ldy + n0;                           // uniform
            char* yt = reinterpret_cast<char*>(a.y + yo);
            const char* rt = a.res ? reinterpret_cast<const char*>(a.res + yo) : nullptr;
            const bool interior = zrow + BM <= a.M && n0 + BN <= a.N;
#define WG_VALUE(J)                                                                                             \
            float v_ = acc[i][J][r];                                                                            \
            if (EPI) {                                                                                          \
                v_ += bias_v[J];                                                                                \
                if (a.res) v_ += reinterpret_cast<const float*>(rt + (size_t)ro * a.ldy * 4 + y_off)[(J) * 32]; \
                if (a.act == 1) v_ = be::smish(v_); else if (a.act == 2) v_ = fmaxf(v_, 0.0f);                  \
            }
            if (interior) {                             // no per-element bounds checks (they cost 10 instructions a store)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ro = i * 32 + (r & 3) + 8 * (r >> 2);
                        float* yr = reinterpret_cast<float*>(yt + (size_t)ro * a.ldy * 4 + y_off);
                        { WG_VALUE(0) yr[0] = v_; }
                        { WG_VALUE(1) yr[32] = v_; }
                    }
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const bool c_ok = n0 + wn * 64 + j * 32 + li < a.N;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int ro = i * 32 + (r & 3) + 8 * (r >> 2);
                            if (c_ok && zrow + wm * 64 + 4 * lh + ro < a.M) {
                                WG_VALUE(j)
                                reinterpret_cast<float*>(yt + (size_t)ro * a.ldy * 4 + y_off)[j * 32] = v_;
                            }
                        }
                }
            }
#undef WG_VALUE
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
            ck = 0; ++cz;
        }
    }
#undef WG_LOAD
}

// ---- split-bf16 GEMMs on the pre-split weights (round 8, the default) ---------------------------------------------------------------
// The arithmetic (be_split_bf16.h; the bits of round 7's kernel, which split both operands in the loop: tests/test_wino_presplit.py):
// both operands' hi / mid / lo pieces by split8 (B's at pack time), v_mfma_f32_32x32x16_bf16 with lane (li, lh) holding row li's
// k = 8 lh .. 8 lh + 7 of a 16-deep chunk, per chunk and accumulator the six products in the order lo.hi, hi.lo, mid.mid, mid.hi,
// hi.mid, hi.hi (A's piece first), fp32 accumulation, K ascending from a zero accumulator per problem.  B's pieces are read ready
// from LDS (k_wino_pack_split's blocks), so that only A (fp32 in HBM and LDS) is split in the loop: half the split instructions of
// splitting both.  A stage is 8 KB A + 12 KB B; the K loop runs over a ring of four
// stages (80 KB: two workgroups per CU) with the DMA three chunks ahead, explicit counted vmcnt waits and one raw s_barrier per chunk
// (the idiom of k_wino_gemm_ws: no full drain of the DMA in front of every barrier), and the next chunk's fragments are read and
// split right behind the current chunk's MFMAs (the read -> split chain no longer sits in front of every chunk's MFMAs).
// vmcnt: every wave issues 5 DMA pieces per chunk (2 A + 3 B), so "vmcnt(5)" = all but the newest chunk's have landed.  At the end of
// a problem the wait for the chunk after next sits IN FRONT of the stores (after them no count would be right without knowing how many
// store instructions the compiler emitted); the last one drains everything, so no DMA into LDS outlives the workgroup.
// Round 9, the same loop as a plain row GEMM.  EPI = 1: k_wino_gemm<1>'s epilogue, y = act(acc + bias[col] (+ res)).  ROWS = 1: the
// "problems" may be GemmArgs' walked row tiles (nb consecutive 128-row tiles of one matrix per workgroup: mrows = 128 nb, zrows = 128,
// xb = 128 lda, yb = 128 ldy, wb = 0; only when every walked tile is full), so that a short K loop keeps one continuous pipeline.
// <0, 0> is the Winograd kernel of round 8, instruction for instruction.
// Round 12, the same arithmetic on another instruction schedule (no result bit moves: the pieces, the MFMA, the lane -> k map, the
// six-product order per accumulator and the K order from a zero accumulator are those of round 8).  Until then hipcc issued a chunk as
// 24 MFMAs, the next chunk's 10 ds_read_b128, lgkmcnt(0), ~90 VALU of split8 in one run: an in-order wave hides at most one 32-cycle
// MFMA of that.  Now the pieces live in two register sets and the next chunk's reads and split sit BETWEEN this chunk's MFMAs, every
// gap closed by __builtin_amdgcn_sched_barrier(0) (PS_CHUNK; split_pair_a / split_pair_b of be_split_bf16.h).  What does not bind: a
// sched_group_barrier sequence over the one-set loop (no group mask matches the inline-asm v_sub_f32; with plain subtractions the
// scheduler regroups the MFMAs into runs of six dependent ones on one accumulator).  The emitted loop (hipcc -S, gfx950, read by hand;
// both bodies alike, <0, 0> and <0, 1> alike; <1, 1> keeps the one-set loop, see the loop):
//   [vmcnt(5)] s_barrier, 5 global_load_lds_dwordx4 + their scalar address arithmetic (7 VALU)
//   gaps 0-4    MFMA, 2 ds_read_b128 each (gap 0 also the 3 v_add_u32 of the slot's addresses)
//   gaps 5-7    MFMA alone
//   gap 8       MFMA, s_waitcnt lgkmcnt(0) (the youngest read is three MFMAs old), half A: 6 VALU + 1 s_nop
//   gaps 9-23   MFMA, half B (5 VALU + s_nop) and half A (6 VALU + s_nop) in turn; no run of VALU longer than 6
//   consecutive MFMAs write different accumulators (v[48:63] v[16:31] v[32:47] v[0:15] in turn); no v_pk_* f32 instruction, no v_mov
//   of a piece, no scratch access in the loop.  hipcc emits no counted lgkmcnt anywhere in this file, hence the early paired reads.
// Compiler report (gfx950; round 8-9 build in brackets), LDS 80 KB: two workgroups per CU = 2 waves per SIMD in every case:
//   <0, 0>  179 VGPRs [138], 0 AGPRs, scratch 0, no VGPR spills,  76 SGPR spills [126], 18.7 KB of code [11.5]
//   <0, 1>  210 VGPRs [140], 0 AGPRs, scratch 0, no VGPR spills,  15 SGPR spills [71],  15.3 KB [10.9]
//   <1, 1>  the one-set loop: 182 VGPRs [150], 0 AGPRs, scratch 0, no VGPR spills, 26 SGPR spills [84], 41.7 KB [43.8].  With the
//           two-set loop and the boundary block (Smish epilogue) behind both bodies it was 222 VGPRs and 80.0 KB, and slower.
// Round 14, EXT = 1 (<0, 0, 1>): a second K segment.  A problem whose position is in GemmArgs::zext runs kext chunks more, A from
// x2 (the transform of the block's input), B from w2 (the planes of the 1x1 downsample's kernel transform), into the same
// accumulators: the block's residual branch inside conv2's GEMMs.  Only the DMA's source addresses and the chunk count a problem
// ends at change (scalar work); a chunk is 2 A + 3 B pieces per wave whichever segment it is from, so the ring, the counted waits
// ("all but the newest chunk have landed"), the two register sets and the boundary block are the ones above, across the seam and
// across problems of unequal length.  K order per output element: x's chunks ascending, then x2's, from a zero accumulator - bits
// depend on neither batch, group count nor stream.  The groups' problems come from a walk table (GemmArgs::ztab) in which the host
// deals the dearer positions evenly.  A template parameter and not a run-time branch: the three instantiations without it are the
// parent's instruction for instruction (hipcc -S compared).  Emitted loop of <0, 0, 1>: per body the same 24 MFMAs, 10 ds_read_b128 and
// 5 global_load_lds_dwordx4 with the same gaps (no gap between two MFMAs of a chunk longer than 12 instructions, as <0, 0>); the
// additions are scalar (5 s_bcnt1_i32_b64, the table look-ups) in the DMA block and the boundary block.
//   <0, 0, 1>  180 VGPRs, 0 AGPRs, scratch 0, no VGPR spills, 94 SGPR spills, 21.5 KB of code, two workgroups per CU
//              (with the segment chosen by selects per piece instead of one branch: 181 VGPRs and 12 B of scratch - not kept)
// Round 16, WN: the wave grid as a template parameter.  WN = 2 is the 2x2 grid above (wave tile 64 x 64: waves (wm, 0) and (wm, 1)
// read and split the same 64 A rows, so every A value is split twice per workgroup); WN = 1 stacks the four waves in M (wave w owns
// rows 32 w .. 32 w + 31 and all 128 columns: ONE A fragment and one split8 per chunk, 3 x 4 B fragment reads, four 32x32
// accumulators).  No result bit moves: product p = g / 4 still goes into accumulator g % 4 in the order lo.hi hi.lo mid.mid mid.hi
// hi.mid hi.hi from the same pieces, K ascending from a zero accumulator with the second segment behind the first - only WHICH wave
// holds an element changes (tests/test_wino_wave_grid.py: both grids against float64 and against each other).  The ring, the 5 DMA
// pieces per wave and chunk (wave w's A pieces 2 w, 2 w + 1 are now its own rows), vmcnt(5), the barrier per chunk, the two register
// sets, the boundary block behind both bodies, the block map, GemmArgs and the host's group search are the ones above.  The default
// path (<0, 0, 0>, <0, 0, 1>) and the raw-store row GEMM <0, 1, 0> run WN = 1; BE_WINO_WAVES22=1 (read once per process) puts them
// back on WN = 2, round 12's loop (hipcc -S against the parent build: the same instruction sequence from the first MFMA to the
// last, both bodies and the boundary block between them; the prologue is 3-5 instructions shorter, register numbers differ).  <1, 1> (fc.1, the one-set loop) stays on WN = 2: its WN = 1
// form was not measured.  The emitted loop of WN = 1 (hipcc -S, gfx950, read by hand; both bodies alike, the three instantiations alike):
//   [vmcnt(5)] s_barrier, 5 global_load_lds_dwordx4 + their scalar address arithmetic
//   gap 0       MFMA, the 2 ds_read_b128 of A (and the 3 v_add_u32 of the slot's addresses)
//   gaps 1-6    MFMA, 2 ds_read_b128 of B each (plane (g - 1) / 2, column blocks 2 ((g - 1) % 2) and the next)
//   gaps 7-9    MFMA alone
//   gap 10      MFMA, s_waitcnt lgkmcnt(0) (the youngest read is three MFMAs old), half A of pair unit 0: 6 VALU + 1 s_nop
//   gaps 11-17  MFMA, half B (5 VALU + s_nop) and half A (6 VALU + s_nop) in turn
//   gaps 18-23  MFMA alone
//   per chunk and wave 24 MFMAs, 14 ds_read_b128 (2x2: 10), 44 VALU + 8 s_nop of split (2x2: 88 + 16), 5 DMA pieces; consecutive MFMAs
//   write different accumulators (v[48:63] v[32:47] v[16:31] v[0:15] in turn); no v_pk_* f32 instruction, no v_mov of a piece, no
//   scratch access in the loop; 64 stores per wave in either boundary form, as on the 2x2 grid.
// Compiler report, WN = 1 [WN = 2 of this build], LDS 80 KB, two workgroups per CU in every case:
//   <0, 0, 0>  202 VGPRs [179], 0 AGPRs, scratch 0, no VGPR spills, 18 SGPR spills [76], 14.1 KB of code [18.3]
//   <0, 0, 1>  203 VGPRs [180], 0 AGPRs, scratch 0, no VGPR spills, 32 SGPR spills [94], 17.2 KB [21.0]
//   <0, 1, 0>  218 VGPRs [210], 0 AGPRs, scratch 0, no VGPR spills,  0 SGPR spills [15], 12.5 KB [14.9]
//   <1, 1, 0>  WN = 2 only: 180 VGPRs, scratch 0, no VGPR spills, 25 SGPR spills, 41.0 KB
// What it bought, and what it did not (DESIGN 3.1 "Round 16", profiles/r21_wave_grid_*): half the split instructions, and the GEMM
// family 4.24 -> 4.16 ms per 8192-patch step (-1.9 %, the second-segment kernel -2.6 %, the plain one -0.6 %) - a quarter of what
// the vector-issue budget promised.
template <int EPI, int ROWS = 0, int EXT = 0, int WN = 2>
__global__ __launch_bounds__(256, 2)
void k_wino_gemm_ps(GemmArgs a) {
    static_assert(WN == 1 || WN == 2, "the four waves form a 4x1 (WN = 1) or a 2x2 (WN = 2) grid");
    constexpr int BM = 128, BKT = 16;
    constexpr int NI = WN == 1 ? 1 : 2, NJ = 4 / NI;    // a wave's 32-row A fragments and 32-column accumulators: NI x NJ = 4
    constexpr int ABYTES = BM * BKT * 4, BBYTES = PS_BLOCK * 2, STAGE = ABYTES + BBYTES;   // 8 KB + 12 KB
    constexpr int NS = PS_STAGES;
    extern __shared__ __attribute__((aligned(16))) float smem_w[];
    char* const lds = reinterpret_cast<char*>(smem_w);
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;          // all N tiles and problem groups of an M tile on one XCD
    const int n_tile = slot % a.n_tiles;
    int m_tile = (slot / a.n_tiles) * 8 + xcd;
    const int zg = m_tile % a.zgroups, zper = (a.nb + a.zgroups - 1) / a.zgroups;
    m_tile /= a.zgroups;
    if (m_tile >= a.m_tiles || zg * zper >= a.nb) return;
    const int nb = min(zper, a.nb - zg * zper), kchunks = a.K / BKT, total0 = kchunks * nb;
    // EXT: the group's problems are entries zg zper .. of the walk table, and a problem in the mask runs kext chunks more
    [[maybe_unused]] const int zbase = zg * zper;
    [[maybe_unused]] auto zpos = [&](int i) -> int {
        const int q = i / 10;
        const uint64_t t = q == 0 ? a.ztab[0] : q == 1 ? a.ztab[1] : q == 2 ? a.ztab[2] : a.ztab[3];
        return (int)((t >> (6 * (i - 10 * q))) & 63);
    };
    [[maybe_unused]] auto zchunks = [&](int pos) -> int { return kchunks + ((a.zext >> pos) & 1 ? a.kext : 0); };
    [[maybe_unused]] auto ext_chunks = [&]() -> int {
        int t = 0;
        for (int i = 0; i < nb; ++i) t += zchunks(zpos(zbase + i)) - kchunks;
        return t;
    };
    const int total = EXT ? total0 + ext_chunks() : total0;
    const int n0 = n_tile * 128, row_base = m_tile * (ROWS ? a.mrows : BM);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    // the wave's tile: rows row0 .. row0 + 32 NI - 1, columns col0 .. col0 + 32 NJ - 1 of the 128 x 128 workgroup tile
    const int row0 = WN == 1 ? wave * 32 : (wave >> 1) * 64, col0 = WN == 1 ? 0 : (wave & 1) * 64;
    const int li = lane & 31, lh = lane >> 5;
    // A staging as in k_wino_gemm: wave w fills pieces 2w, 2w+1 of the A tile, lane -> (row lane >> 2, swizzled quad)
    const int srow = lane >> 2, sq = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned a_off[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = (2 * wave + p) * 16 + srow;
        a_off[p] = (unsigned)((row_base + r < a.M ? r : 0) * a.lda + 4 * sq) * 4u;     // rows past M load a valid row, never stored
    }
    const char* xt = reinterpret_cast<const char*>(a.x + (EXT ? (int64_t)0 : (int64_t)zg * zper * a.xb) + (int64_t)row_base * a.lda);   // (EXT: positions from the table)
    // B: pieces 3w .. 3w+2 of the chunk's 12-KB block, which is already the LDS image (lane-linear: this lane's 16 B)
    const char* wt = reinterpret_cast<const char*>(a.w + (EXT ? (int64_t)0 : (int64_t)zg * zper * a.wb)) + (int64_t)n_tile * kchunks * BBYTES + lane * 16;
    float* const yg = a.y + (EXT ? (int64_t)0 : (int64_t)zg * zper * a.yb);
    // EXT: the second segment's operands - A rows of x2 (its own row stride), B blocks of w2
    [[maybe_unused]] unsigned a_off2[2] = {0u, 0u};
    [[maybe_unused]] const char* x2t = nullptr;
    [[maybe_unused]] const char* w2t = nullptr;
    if constexpr (EXT) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int r = (2 * wave + p) * 16 + srow;
            a_off2[p] = (unsigned)((row_base + r < a.M ? r : 0) * a.lda2 + 4 * sq) * 4u;
        }
        x2t = reinterpret_cast<const char*>(a.x2 + (int64_t)row_base * a.lda2);
        w2t = reinterpret_cast<const char*>(a.w2) + (int64_t)n_tile * a.kext * BBYTES + lane * 16;
    }
    // fragment reads: A row row0 + 32 i + li, quads 2 lh, 2 lh + 1 (swizzled as stored); B plane p, row col0 + 32 j + li, half lh
    // (row0, col0 and 32 j are multiples of 32: the same address function of li and lh on either wave grid, conflict-free)
    const int fsw = (li >> 2) & 3;
    const int a_fr0 = ((row0 + li) * BKT + 4 * ((2 * lh) ^ fsw)) * 4;
    const int a_fr1 = ((row0 + li) * BKT + 4 * ((2 * lh + 1) ^ fsw)) * 4;
    const int b_fr = ABYTES + (col0 + li) * 32 + ps_slot(li, lh) * 16;
    f32x16 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    int lz = 0, lk = 0, l_buf = 0;                     // (problem, chunk) of the next DMA and its ring slot
    // EXT: that problem's position and chunk count; chunks kchunks .. are the second segment's.  Every chunk is still 2 A + 3 B
    // pieces per wave, so the counted waits below hold across the seam and across problems of unequal length.
    [[maybe_unused]] int lpos = 0, lkz = 0;
    if constexpr (EXT) { lpos = zpos(zbase); lkz = zchunks(lpos); }
#define PS_DMA()                                                                                                \
    do {                                                                                                        \
        if constexpr (EXT) {                                                                                    \
            const char* xs_ = xt + ((int64_t)lpos * a.xb + lk * BKT) * 4;                                       \
            const char* ws_ = wt + (int64_t)lpos * a.wb * 4 + lk * BBYTES;                                      \
            unsigned ao_[2] = {a_off[0], a_off[1]};                                                             \
            if (lk >= kchunks) {                       /* the second segment: A from x2, B from w2 */           \
                const int e_ = __builtin_popcountll(a.zext & (((uint64_t)1 << lpos) - 1));                      \
                xs_ = x2t + ((int64_t)lpos * a.xb2 + (lk - kchunks) * BKT) * 4;                                 \
                ws_ = w2t + (int64_t)e_ * a.wb2 * 4 + (lk - kchunks) * BBYTES;                                  \
                ao_[0] = a_off2[0];                                                                             \
                ao_[1] = a_off2[1];                                                                             \
            }                                                                                                   \
            char* st_ = lds + l_buf * STAGE;                                                                    \
            _Pragma("unroll") for (int p_ = 0; p_ < 2; ++p_)                                                    \
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(xs_ + ao_[p_]), (lds_ptr_t)(st_ + (2 * wave + p_) * 1024), 16, 0, 0); \
            _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_)                                                    \
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(ws_ + (3 * wave + p_) * 1024),                     \
                                                 (lds_ptr_t)(st_ + ABYTES + (3 * wave + p_) * 1024), 16, 0, 0); \
        } else {                                                                                                \
            const char* xs_ = xt + ((int64_t)lz * a.xb + lk * BKT) * 4;                                         \
            const char* ws_ = wt + (int64_t)lz * a.wb * 4 + lk * BBYTES;                                        \
            char* st_ = lds + l_buf * STAGE;                                                                    \
            _Pragma("unroll") for (int p_ = 0; p_ < 2; ++p_)                                                    \
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(xs_ + a_off[p_]), (lds_ptr_t)(st_ + (2 * wave + p_) * 1024), 16, 0, 0); \
            _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_)                                                    \
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(ws_ + (3 * wave + p_) * 1024),                     \
                                                 (lds_ptr_t)(st_ + ABYTES + (3 * wave + p_) * 1024), 16, 0, 0); \
        }                                                                                                       \
        if constexpr (EXT) {                                                                                    \
            if (lk + 1 < lkz) ++lk;                                                                             \
            else if (lz + 1 < nb) { lk = 0; ++lz; lpos = zpos(zbase + lz); lkz = zchunks(lpos); }               \
        } else {                                                                                                \
            if (lk + 1 < kchunks) ++lk; else if (lz + 1 < nb) { lk = 0; ++lz; }   /* past the end: the last chunk again */ \
        }                                                                                                       \
        l_buf = (l_buf + 1) % NS;                                                                               \
    } while (0)
    const unsigned y_off = (unsigned)((row0 + 4 * lh) * a.ldy + col0 + li) * 4u;
    float bias_v[NJ] = {};
    if (EPI) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = n0 + col0 + j * 32 + li;
            bias_v[j] = (a.bias && c < a.N) ? a.bias[c] : 0.0f;
        }
    }
    // two sets of pieces: chunk c's MFMAs read set c & 1 while chunk c + 1's fragments are read and split into the other set, one
    // piece of that work in every gap between two MFMAs (PS_CHUNK).  The set is a compile-time parameter of the body (a run-time
    // index would send the pieces to scratch), so the body is compiled once per set.
    u32x4 ap[2][3][NI];                                // [set][hi, mid, lo][i], one dword per pair unit
    bf16x8 bp[2][3][NJ];                               // [set][hi, mid, lo][j]
    int r_buf = 0;                                     // ring slot whose fragments are read next
    // One chunk: 24 groups, each closed by a sched_barrier(0) (nothing crosses it, so the order below is the emitted order).
    // Group g issues MFMA g - product p = g / 4 (lo.hi hi.lo mid.mid mid.hi hi.mid hi.hi), accumulator (i, j) = ((g % 4) / NJ, g % NJ):
    // consecutive MFMAs never share an accumulator - and, for chunk + 1 out of ring slot r_buf into set S ^ 1,
    // on the 2x2 grid (two A fragments, 3 x 2 B fragments, two split8):
    //   g = 0, 1    the two fp32 A fragment reads (quads 2 lh, 2 lh + 1) of i = g
    //   g = 2..4    the two reads (j = 0, 1) of B plane g - 2
    //   g = 8..23   one half of one of the eight pair units of the two split8 (unit u = (g - 8) / 2: i = u / 4; half A, then half B)
    // on the 4x1 grid (one A fragment, 3 x 4 B fragments, one split8):
    //   g = 0       the two fp32 A fragment reads
    //   g = 1..6    two B reads each: plane (g - 1) / 2, j = 2 ((g - 1) % 2) and the next
    //   g = 10..17  one half of one of the four pair units of the split8 (unit u = (g - 10) / 2; half A, then half B)
    // The LDS reads are plain loads and the compiler places their wait.  It only ever emits lgkmcnt(0), in front of the first split
    // group: hence the reads two to a gap and early, so that the youngest is three MFMAs old when the wait comes.
    constexpr int G_SPLIT = WN == 1 ? 10 : 8;          // the first split group
#define PS_CHUNK(S)                                                                                             \
    do {                                                                                                        \
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};                                   \
        const char* sb_ = lds + r_buf * STAGE;                                                                  \
        f32x4 af_[2][NI];                              /* [quad][i] */                                          \
        float r0_[4 * NI], r1_[4 * NI];                                                                         \
        _Pragma("unroll") for (int g_ = 0; g_ < 24; ++g_) {                                                     \
            acc[(g_ & 3) / NJ][g_ % NJ] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                              \
                __builtin_bit_cast(bf16x8, ap[S][PA[g_ >> 2]][(g_ & 3) / NJ]), bp[S][PB[g_ >> 2]][g_ % NJ],     \
                acc[(g_ & 3) / NJ][g_ % NJ], 0, 0, 0);                                                          \
            if (g_ < NI) {                                                                                      \
                af_[0][g_] = *reinterpret_cast<const f32x4*>(sb_ + a_fr0 + g_ * 32 * BKT * 4);                  \
                af_[1][g_] = *reinterpret_cast<const f32x4*>(sb_ + a_fr1 + g_ * 32 * BKT * 4);                  \
            }                                                                                                   \
            if (WN == 2 && g_ >= 2 && g_ < 5)                                                                   \
                _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                                \
                    bp[(S) ^ 1][g_ - 2][j_ % NJ] = *reinterpret_cast<const bf16x8*>(sb_ + b_fr + (g_ - 2) * 4096 + j_ * 32 * 32); \
            if (WN == 1 && g_ >= 1 && g_ < 7)                                                                   \
                _Pragma("unroll") for (int j_ = 2 * ((g_ - 1) & 1); j_ < 2 * ((g_ - 1) & 1) + 2; ++j_)          \
                    bp[(S) ^ 1][(g_ - 1) >> 1][j_ % NJ] =                                                       \
                        *reinterpret_cast<const bf16x8*>(sb_ + b_fr + ((g_ - 1) >> 1) * 4096 + j_ * 32 * 32);   \
            if (g_ >= G_SPLIT && g_ < G_SPLIT + 8 * NI) {                                                       \
                const int u_ = (g_ - G_SPLIT) >> 1, i_ = u_ >> 2, e_ = u_ & 3;                                  \
                if ((g_ & 1) == 0) {                                                                            \
                    unsigned h_, m_;                                                                            \
                    be::bf6::split_pair_a(af_[e_ >> 1][i_][(2 * e_) & 3], af_[e_ >> 1][i_][(2 * e_ + 1) & 3], h_, m_, r0_[u_], r1_[u_]); \
                    ap[(S) ^ 1][0][i_][e_] = h_;                                                                \
                    ap[(S) ^ 1][1][i_][e_] = m_;                                                                \
                } else {                                                                                        \
                    unsigned l_ = be::bf6::split_pair_b(r0_[u_], r1_[u_], ap[(S) ^ 1][1][i_][e_]);              \
                    asm volatile("" : "+v"(l_));       /* (keeps the last cvt_pk in its group) */               \
                    ap[(S) ^ 1][2][i_][e_] = l_;                                                                \
                }                                                                                               \
            }                                                                                                   \
            __builtin_amdgcn_sched_barrier(0);                                                                  \
        }                                                                                                       \
        r_buf = (r_buf + 1) % NS;                                                                               \
    } while (0)
    // a chunk's pieces from ring slot SLOT into set 0 in one piece (the prologue)
#define PS_FRAGS0(SLOT)                                                                                         \
    do {                                                                                                        \
        const char* sb_ = lds + (SLOT) * STAGE;                                                                 \
        f32x4 af_[2][NI];                                                                                       \
        _Pragma("unroll") for (int i_ = 0; i_ < NI; ++i_) {                                                     \
            af_[0][i_] = *reinterpret_cast<const f32x4*>(sb_ + a_fr0 + i_ * 32 * BKT * 4);                      \
            af_[1][i_] = *reinterpret_cast<const f32x4*>(sb_ + a_fr1 + i_ * 32 * BKT * 4);                      \
        }                                                                                                       \
        _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_)                                                        \
            _Pragma("unroll") for (int j_ = 0; j_ < NJ; ++j_)                                                   \
                bp[0][p_][j_] = *reinterpret_cast<const bf16x8*>(sb_ + b_fr + p_ * 4096 + j_ * 32 * 32);        \
        _Pragma("unroll") for (int i_ = 0; i_ < NI; ++i_) {                                                     \
            bf16x8 h_, m_, l_;                                                                                  \
            split8(af_[0][i_], af_[1][i_], h_, m_, l_);                                                         \
            ap[0][0][i_] = __builtin_bit_cast(u32x4, h_);                                                       \
            ap[0][1][i_] = __builtin_bit_cast(u32x4, m_);                                                       \
            ap[0][2][i_] = __builtin_bit_cast(u32x4, l_);                                                       \
        }                                                                                                       \
    } while (0)
    PS_DMA();                                          // chunk 0
    PS_DMA();                                          // chunk 1
    PS_DMA();                                          // chunk 2
    __builtin_amdgcn_s_waitcnt(0x0F75);                // vmcnt(5): chunks 0 and 1 have landed
    __builtin_amdgcn_s_barrier();                      // ... every wave's
    PS_FRAGS0(0);                                      // chunk 0's pieces
    r_buf = 1;
    int cz = 0, ck = 0;
    [[maybe_unused]] int cpos = 0, ckz = 0;            // EXT: position and chunk count of problem cz
    if constexpr (EXT) { cpos = zpos(zbase); ckz = zchunks(cpos); }
    bool landed = true;                                // the NEXT chunk's DMA is known to be in LDS
    // The loop walks two chunks per trip, body 0 then body 1, each followed by the problem-boundary block; an odd total ends behind
    // body 0.  (One shared boundary block - body by parity, or set 1 moved / read again into set 0 behind an odd problem - was tried:
    // the register allocator then assembles every chunk's tuples with 12 v_mov in front of the first MFMA, or spills.)  With an even
    // chunk count per problem, K % 32 == 0 - every layer of LocalStage -, only the block behind body 1 is ever executed.
#define PS_TOP()                                                                                                \
    do {                                                                                                        \
        if (!landed) __builtin_amdgcn_s_waitcnt(0x0F75);                               /* vmcnt(5): chunk + 1 has landed */ \
        landed = false;                                                                                         \
        __builtin_amdgcn_s_barrier();                  /* ... every wave's; everyone has read the slot of chunk - 1 (a chunk ago) */ \
        PS_DMA();                                      /* chunk + 3, into that slot */                          \
        __builtin_amdgcn_sched_barrier(0);                                                                      \
    } while (0)
    auto boundary = [&](int kc) __attribute__((always_inline)) {   // behind chunk kc
        if (++ck == (EXT ? ckz : kchunks)) {            // problem cz is complete: store, clear
            if (kc + 1 < total) __builtin_amdgcn_s_waitcnt(0x0F75);                    // chunk + 2 has landed
            else __builtin_amdgcn_s_waitcnt(0x0F70);                                   // nothing left in flight
            landed = true;
            __builtin_amdgcn_sched_barrier(0);
            const int zrow = ROWS ? row_base + cz * a.zrows : row_base;
            char* yt = reinterpret_cast<char*>(yg + (int64_t)(EXT ? cpos : cz) * a.yb + (int64_t)row_base * a.ldy + n0);   // uniform
            const char* rt = EPI && a.res ? reinterpret_cast<const char*>(a.res) + (yt - reinterpret_cast<char*>(a.y)) : nullptr;
#define PS_VALUE(J)                                                                                             \
            float v_ = acc[i][J][r];                                                                            \
            if (EPI) {                                                                                          \
                v_ += bias_v[J];                                                                                \
                if (rt) v_ += reinterpret_cast<const float*>(rt + (size_t)ro * a.ldy * 4 + y_off)[(J) * 32];    \
                if (a.act == 1) v_ = be::smish(v_); else if (a.act == 2) v_ = fmaxf(v_, 0.0f);                  \
            }
            if (zrow + BM <= a.M && n0 + 128 <= a.N) {
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ro = i * 32 + (r & 3) + 8 * (r >> 2);
                        float* yr = reinterpret_cast<float*>(yt + (size_t)ro * a.ldy * 4 + y_off);
#pragma unroll
                        for (int j = 0; j < NJ; ++j) { PS_VALUE(j) yr[32 * j] = v_; }
                    }
            } else {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const bool c_ok = n0 + col0 + j * 32 + li < a.N;
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int ro = i * 32 + (r & 3) + 8 * (r >> 2);
                            if (c_ok && zrow + row0 + 4 * lh + ro < a.M) {
                                PS_VALUE(j)
                                reinterpret_cast<float*>(yt + (size_t)ro * a.ldy * 4 + y_off)[j * 32] = v_;
                            }
                        }
                }
            }
#undef PS_VALUE
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
            ck = 0; ++cz;
            if constexpr (EXT)
                if (cz < nb) { cpos = zpos(zbase + cz); ckz = zchunks(cpos); }
        }
    };
    if constexpr (EPI) {
        // <1, 1> (fc.1: one problem of 144 chunks per workgroup) keeps the one-set loop of rounds 8-9 - the MFMAs, then chunk + 1's
        // pieces into set 0 in one piece: measured with the two-set loop it LOST 5.5 % (195.7 -> 206.4 us per launch, round 12), and
        // its Smish epilogue behind both bodies made 80 KB of code
        for (int kc = 0; kc < total; ++kc) {
            PS_TOP();
            {
                constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};   // lo.hi hi.lo mid.mid mid.hi hi.mid hi.hi
#pragma unroll
                for (int p = 0; p < 6; ++p)
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ap[0][PA[p]][i]), bp[0][PB[p]][j],
                                                                                acc[i][j], 0, 0, 0);
                PS_FRAGS0(r_buf);                      // chunk + 1's pieces, under this chunk's MFMAs
                r_buf = (r_buf + 1) % NS;
            }
            __builtin_amdgcn_sched_barrier(0);
            boundary(kc);
        }
    } else {
        for (int kc = 0; kc < total; kc += 2) {
            PS_TOP();
            PS_CHUNK(0);                               // this chunk's MFMAs with chunk + 1's reads and split in their gaps
            __builtin_amdgcn_sched_barrier(0);
            boundary(kc);
            if (kc + 1 < total) {
                PS_TOP();
                PS_CHUNK(1);
                __builtin_amdgcn_sched_barrier(0);
                boundary(kc + 1);
            }
        }
    }
#undef PS_TOP
#undef PS_DMA
#undef PS_FRAGS0
#undef PS_CHUNK
}

// ---- weight-stationary form of the same GEMMs (large batches, K = 96 / 256 / 384) ------------------------------------------
// A workgroup owns ONE (problem z, N tile), keeps that B tile [128 cols][K] in REGISTERS (K fragment registers per lane: 384
// at K = 384, so one wave per SIMD) and walks a range of M tiles streaming only A: half the DMA pieces and half the fragment
// reads per MFMA of k_wino_gemm.  The issue model of DESIGN 3.1d prices the loop at 2048 / (2048 + 64 + 120 + 60) = 89 %; with
// one wave per SIMD every latency has to be hidden inside the wave: three LDS buffers for A, DMA two chunks ahead, the
// fragments of chunk s+1 read while the MFMAs of chunk s run, one raw barrier per chunk, explicit vmcnt waits (the wait for a tile's
// successor DMA sits in FRONT of that tile's stores, so no count depends on the number of store instructions).  Same order of operations per output element as k_wino_gemm:
// bit-identical.  Measured (tools/wino_gemm_lab.hip, weight_stationary_run13.log): +3...5 % over k_wino_gemm.
// KIND (0: the 25 problems of a Winograd layer, 1: a plain row GEMM - the blocks' 1x1 downsamples) changes nothing in the code: it
// gives the two uses different kernel symbols, so that a profiler's per-kernel averages do not mix launches of different sizes
template <int KCH, int KIND>
__global__ __launch_bounds__(256, 1)
void k_wino_gemm_ws(GemmArgs a, int mgroups) {
    constexpr int BM = 128, BKT = 16, ABUF = BM * BKT;     // floats per A stage (8 KB)
    extern __shared__ __attribute__((aligned(16))) float smem_w[];
    // workgroup -> (problem z, M range, N tile): the N tiles of one (z, M range) are consecutive slots of ONE XCD (ids congruent
    // mod 8 share an XCD), so they run side by side and the A rows they all stream come from HBM once and from that L2 after
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    const int n_tile = slot % a.n_tiles;
    const int unit = (slot / a.n_tiles) * 8 + xcd;
    const int z = unit / mgroups, mg = unit % mgroups;
    const int tiles_per = (a.m_tiles + mgroups - 1) / mgroups;
    const int t0 = mg * tiles_per, t1 = min(a.m_tiles, t0 + tiles_per);
    if (z >= a.nb || t0 >= t1) return;
    const int n0 = n_tile * 128;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int srow = lane >> 2, sq = (lane & 3) ^ ((lane >> 4) & 3);
    const int fsw = (li >> 2) & 3;
    const int fr0 = li * BKT + 4 * (lh ^ fsw), fr1 = li * BKT + 4 * ((lh + 2) ^ fsw);
    // ---- B tile -> registers through LDS, eight K chunks (64 KB) per pass: all the DMAs of a pass are in flight together, ONE
    //      wait per pass (chunk by chunk the fill was 24 dependent DMA round trips: ~36 us of a ~530 us workgroup)
    f32x4 breg[KCH][2][2];
    {
        constexpr int PASS = 8;
        const float* wt = a.w + (int64_t)z * a.wb + (int64_t)n0 * a.K;
        unsigned b_off[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) b_off[p] = (unsigned)(((2 * wave + p) * 16 + srow) * a.K + 4 * sq) * 4u;
#pragma unroll
        for (int c0 = 0; c0 < KCH; c0 += PASS) {
#pragma unroll
            for (int cc = 0; cc < PASS; ++cc)
                if (c0 + cc < KCH) {
#pragma unroll
                    for (int p = 0; p < 2; ++p)
                        __builtin_amdgcn_global_load_lds((glb_ptr_t)(reinterpret_cast<const char*>(wt + (c0 + cc) * BKT) + b_off[p]),
                                                         (lds_ptr_t)(smem_w + cc * ABUF + (2 * wave + p) * 256), 16, 0, 0);
                }
            __syncthreads();
#pragma unroll
            for (int cc = 0; cc < PASS; ++cc)
                if (c0 + cc < KCH) {
                    const float* st = smem_w + cc * ABUF;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        breg[c0 + cc][0][j] = *reinterpret_cast<const f32x4*>(st + (wn * 64 + j * 32) * BKT + fr0);
                        breg[c0 + cc][1][j] = *reinterpret_cast<const f32x4*>(st + (wn * 64 + j * 32) * BKT + fr1);
                    }
                }
            __syncthreads();                               // everyone has its fragments before the next pass / the A ring overwrites
        }
    }
    // ---- stream A over the M tiles [t0, t1): flat step s = (tile, chunk); every tile is full (the launcher checks M % 128 == 0)
    unsigned a_off[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) a_off[p] = (unsigned)(((2 * wave + p) * 16 + srow) * a.lda + 4 * sq) * 4u;
    const float* xz = a.x + (int64_t)z * a.xb;
    int l_tile = t0, l_c = 0, l_buf = 0;                   // next DMA: (tile, chunk) into ring slot l_buf
#define WS_DMA()                                                                                                \
    do {                                                                                                        \
        const int lt_ = l_tile < t1 ? l_tile : t1 - 1;                       /* past the end: a harmless re-read */  \
        const char* xs_ = reinterpret_cast<const char*>(xz + (int64_t)lt_ * BM * a.lda + l_c * BKT);            \
        float* st_ = smem_w + l_buf * ABUF + (2 * wave) * 256;                                                  \
        _Pragma("unroll") for (int p_ = 0; p_ < 2; ++p_)                                                        \
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(xs_ + a_off[p_]), (lds_ptr_t)(st_ + p_ * 256), 16, 0, 0); \
        if (++l_c == KCH) { l_c = 0; ++l_tile; }                                                                \
        l_buf = l_buf == 2 ? 0 : l_buf + 1;                                                                     \
    } while (0)
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    f32x4 fa[2][2][2];                                     // [set][g][i]: the fragments of step s and of step s + 1
    WS_DMA();                                              // step 0
    WS_DMA();                                              // step 1
    __builtin_amdgcn_s_waitcnt(0x0F72);                    // vmcnt(2): step 0 has landed
    __builtin_amdgcn_s_barrier();
    int r_buf = 0;                                         // ring slot whose fragments are read next
#define WS_READ(SET)                                                                                            \
    do {                                                                                                        \
        const float* sb_ = smem_w + r_buf * ABUF + (wm * 64) * BKT;                                             \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                      \
            fa[SET][0][i_] = *reinterpret_cast<const f32x4*>(sb_ + i_ * 32 * BKT + fr0);                        \
            fa[SET][1][i_] = *reinterpret_cast<const f32x4*>(sb_ + i_ * 32 * BKT + fr1);                        \
        }                                                                                                       \
        r_buf = r_buf == 2 ? 0 : r_buf + 1;                                                                     \
    } while (0)
    WS_READ(0);
    const unsigned y_off = (unsigned)((wm * 64 + 4 * lh) * a.ldy + wn * 64 + li) * 4u;
    for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            // the DMA of the NEXT step (issued one step ago) has to land before its fragments are read below: vmcnt(0) - it is
            // the only vector-memory operation in flight here.  After a finished tile that wait has already happened, in front
            // of the tile's stores (below), so nothing here depends on how many store instructions the compiler emitted (round 1
            // waited "all but the newest 63" behind the 64 stores: right only for exactly that store count)
            if (!(c == 0 && t != t0)) __builtin_amdgcn_s_waitcnt(0x0F70);
            __builtin_amdgcn_s_barrier();                  // every wave's pieces of step + 1 are in LDS; slot (step + 2) % 3 is free
            WS_DMA();                                      // step + 2
            __builtin_amdgcn_sched_barrier(0);
            WS_READ((c + 1) & 1);                          // fragments of step + 1 (KCH is even: the parity is static)
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c & 1][g][i].x, breg[c][g][j].x, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c & 1][g][i].y, breg[c][g][j].y, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c & 1][g][i].z, breg[c][g][j].z, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c & 1][g][i].w, breg[c][g][j].w, acc[i][j], 0, 0, 0);
                    }
            __builtin_amdgcn_sched_barrier(0);
        }
        // the first step of the next tile needs its DMA (issued at the top of the step that just ended, a whole chunk of MFMAs
        // ago) in LDS: wait for it HERE, while it is still the only thing in flight, then issue the tile's stores
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __builtin_amdgcn_sched_barrier(0);
        char* yt = reinterpret_cast<char*>(a.y + (int64_t)z * a.yb + (int64_t)t * BM * a.ldy + n0);   // uniform; full tile, N % 128 == 0
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = i * 32 + (r & 3) + 8 * (r >> 2);
                float* yr = reinterpret_cast<float*>(yt + (size_t)ro * a.ldy * 4 + y_off);
                yr[0] = acc[i][0][r];
                yr[32] = acc[i][1][r];
                acc[i][0][r] = 0.0f; acc[i][1][r] = 0.0f;
            }
    }
#undef WS_DMA
#undef WS_READ
}

// kid = BE_KERNEL_WINO_GEMM: the 25 problems of a Winograd layer (n patches -> 4 n rows each);  BE_KERNEL_GEMM_ROWS: one plain GEMM
// of n rows
template <int KCH, int KIND = 0>
int launch_ws(const GemmArgs& g, hipStream_t s, int64_t n, int cin, int cout, int kid = BE_KERNEL_WINO_GEMM) {
    constexpr size_t lds = (size_t)8 * 128 * 16 * sizeof(float);     // 64 KB: eight chunks of the B fill (the A ring uses three)
    static be::DeviceFlags attr_set{};                      // dynamic-LDS cap raised once per device (thread-safe)
    if (int rc_ = be::ensure_dynamic_lds(reinterpret_cast<const void*>(&k_wino_gemm_ws<KCH, KIND>), lds, attr_set)) return rc_;
    const int cus = be::device_cu_count();
    // ONE workgroup per CU at a time (the kernel takes the whole register file of a CU).  Workgroup ids go round-robin over the 8
    // XCDs, so what has to fit is per XCD: ceil(units / 8) * n_tiles workgroups in rounds of (CUs per XCD).  mgroups = M ranges per
    // problem: the launch lasts rounds x (tiles per range + the register fill, ~0.5 of a tile's time).  Searched, not guessed
    // (round 4): with 40 problems x 128 row tiles and N = 256 the old rule (first round count that gives >= 8 ranges) chose 9 ranges =
    // 3 rounds of 15 tiles where 16 ranges are exactly 5 rounds of 8 (ideal: 40 tile times per CU; 45 -> 41).
    const int per_xcd = cus / 8 > 0 ? cus / 8 : 1;
    int mgroups = 1;
    {
        const int mg_max = g.m_tiles / 4 > 0 ? g.m_tiles / 4 : 1;                   // >= 4 tiles per register fill
        double best = 1e30;
        for (int mg = 1; mg <= mg_max; ++mg) {
            const int tiles_per = (g.m_tiles + mg - 1) / mg;
            const int ranges = (g.m_tiles + tiles_per - 1) / tiles_per;             // ranges that really have tiles
            if (ranges != mg) continue;
            const int wg_xcd = ((g.nb * mg + 7) / 8) * g.n_tiles;
            const int rounds = (wg_xcd + per_xcd - 1) / per_xcd;
            const double cost = rounds * (tiles_per + 0.5);
            if (cost < best - 1e-9) { best = cost; mgroups = mg; }
        }
    }
    const int units = g.nb * mgroups;
    const unsigned grid = (unsigned)(8 * ((units + 7) / 8) * g.n_tiles);
    {
        const double rows = kid == BE_KERNEL_WINO_GEMM ? (double)TPI * n : (double)n, probs = g.nb;
        be::ProfileScope prof(s, kid, probs * 2.0 * rows * cin * cout,
                              probs * 4.0 * (rows * cin + (double)cin * cout + rows * cout),
                              probs * 2.0 * g.m_tiles * g.n_tiles * 128.0 * 128.0 * cin);
        hipLaunchKernelGGL((k_wino_gemm_ws<KCH, KIND>), dim3(grid), dim3(256), lds, s, g, mgroups);
    }
    return be::check_launch("be_wino_conv3x3_6x6_f32(gemm, weight-stationary)");
}

}  // namespace

extern "C" int be_wino_tile_rows(void) { return TH; }

// U [NPOS][cout_pad32][cin] fp32, then its pre-split bf16 planes: NPOS x (cout padded to 128) x cin x 3 bf16 (k_wino_pack_split)
static size_t wino_u_floats(int cout, int cin) { return (size_t)NPOS * ((cout + 31) / 32 * 32) * cin; }

extern "C" size_t be_wino_packed_floats(int cout, int cin) {
    if (cout <= 0 || cin <= 0 || cin % 32) return 0;
    return wino_u_floats(cout, cin) + (size_t)NPOS * ((cout + 127) / 128 * 128) * cin * 3 / 2;
}

extern "C" int be_wino_pack_f32(const float* w, const float* b, const float* gamma, const float* beta, const float* mean,
                                const float* var, float eps, int cout, int cin, float* packed_w, float* packed_bias,
                                void* stream) {
    BE_REQUIRE(w && packed_w && packed_bias, "be_wino_pack_f32: null pointer");
    BE_REQUIRE(cout > 0 && cin > 0 && cin % 32 == 0, "be_wino_pack_f32: cin must be a multiple of 32 (got %d)", cin);
    BE_REQUIRE((gamma == nullptr) == (beta == nullptr) && (gamma == nullptr) == (mean == nullptr) && (gamma == nullptr) == (var == nullptr),
               "be_wino_pack_f32: BatchNorm tensors must be all set or all null");
    const int cp = (cout + 31) / 32 * 32;
    hipLaunchKernelGGL(k_wino_pack<0>, dim3(grid_cap((int64_t)cp * cin, 256, 4096)), dim3(256), 0, be::as_stream(stream), w, b, gamma,
                       beta, mean, var, eps, cout, cin, cp, packed_w, packed_bias);
    if (int rc = be::check_launch("be_wino_pack_f32")) return rc;
    const int n_tiles = (cout + 127) / 128;
    hipLaunchKernelGGL(k_wino_pack_split, dim3(grid_cap((int64_t)NPOS * 128 * n_tiles * (cin / 8), 256, 4096)), dim3(256), 0,
                       be::as_stream(stream), packed_w, NPOS, cp, cin, n_tiles,
                       reinterpret_cast<__bf16*>(packed_w + wino_u_floats(cout, cin)));
    return be::check_launch("be_wino_pack_f32(split)");
}

// A block's 1x1 downsample in the form conv2's GEMMs take as their second K segment (round 14): the transform of the kernel as a
// centre-tap 3x3 at its NLIVE non-zero positions, U_ds [NLIVE][cout_pad32][cin] fp32 (position 5 zr + zc is number 3 (zr - 1) + zc - 1),
// then its hi / mid / lo planes in the GEMM's block layout
static size_t wino_ds_u_floats(int cout, int cin) { return (size_t)NLIVE * ((cout + 31) / 32 * 32) * cin; }

extern "C" int be_wino_ds_positions(void) { return NLIVE; }

extern "C" size_t be_wino_ds_packed_floats(int cout, int cin) {
    if (cout <= 0 || cin <= 0 || cin % 16) return 0;
    return wino_ds_u_floats(cout, cin) + (size_t)NLIVE * ((cout + 127) / 128 * 128) * cin * 3 / 2;
}

extern "C" int be_wino_ds_pack_f32(const float* w, const float* b, const float* gamma, const float* beta, const float* mean,
                                   const float* var, float eps, int cout, int cin, float* packed_ds, float* packed_bias, void* stream) {
    BE_REQUIRE(w && packed_ds, "be_wino_ds_pack_f32: null pointer");
    BE_REQUIRE(cout > 0 && cin > 0 && cin % 16 == 0, "be_wino_ds_pack_f32: cin must be a multiple of 16 (got %d)", cin);
    BE_REQUIRE((gamma == nullptr) == (beta == nullptr) && (gamma == nullptr) == (mean == nullptr) && (gamma == nullptr) == (var == nullptr),
               "be_wino_ds_pack_f32: BatchNorm tensors must be all set or all null");
    BE_REQUIRE(be::aligned16(packed_ds), "be_wino_ds_pack_f32: packed_ds must be 16-byte aligned");
    const int cp = (cout + 31) / 32 * 32, n_tiles = (cout + 127) / 128;
    hipLaunchKernelGGL(k_wino_pack<1>, dim3(grid_cap((int64_t)cp * cin, 256, 4096)), dim3(256), 0, be::as_stream(stream), w, b, gamma,
                       beta, mean, var, eps, cout, cin, cp, packed_ds, packed_bias);
    if (int rc = be::check_launch("be_wino_ds_pack_f32")) return rc;
    hipLaunchKernelGGL(k_wino_pack_split, dim3(grid_cap((int64_t)NLIVE * 128 * n_tiles * (cin / 8), 256, 4096)), dim3(256), 0,
                       be::as_stream(stream), packed_ds, NLIVE, cp, cin, n_tiles,
                       reinterpret_cast<__bf16*>(packed_ds + wino_ds_u_floats(cout, cin)));
    return be::check_launch("be_wino_ds_pack_f32(split)");
}

extern "C" size_t be_wino_workspace_floats(int64_t n, int cin, int cout) {
    if (n <= 0) return 0;
    return (size_t)100 * n * ((size_t)cin + cout);              // room for V + M of either tile shape (NPOS x TPI = 100 or 80 values per channel)
}

namespace {

// large batches take k_wino_gemm and the tile-major buffers, small ones the batched k_conv_igemm launch and plane-major buffers
bool wino_large(int64_t n, int cout) {
    static const bool no_persist = getenv("BE_WINO_NO_PERSIST") != nullptr;        // A/B knob
    return ((cout + 31) / 32 * 32) % 128 == 0 && n >= 1024 && !no_persist && (int64_t)NPOS * TPI * n * (int64_t)cout < ((int64_t)1 << 31);
}

// The split-bf16 GEMMs (k_wino_gemm_ps) for every batch size: A (V) split in the loop, B from the pre-split planes behind U;
// tile-major buffers for large batches, plane-major for small ones (only the strides differ), so one patch gets the same bits in
// any batch.
// Round 14, Vx != nullptr: at the NLIVE positions of a 1x1 kernel's transform M[z] = V[z] U[z]^T + Vx[z] Uds[z]^T, K order V's chunks
// ascending, then Vx's, from a zero accumulator (k_wino_gemm_ps<0, 0, 1>) - a block's downsample inside conv2's GEMMs.  Vx: the
// transform of the block's input (cin_ext channels) in V's layout; ds_planes: the planes of be_wino_ds_pack_f32.  tm_force >= 0
// picks the layout (tile-major 1 / plane-major 0) whatever the batch size.
// A/B knob: BE_WINO_WAVES22=1 puts the two-set loops back on the 2x2 wave grid of rounds 8-15 (the same bits; read once per process)
bool ps_waves22() {
    static const bool on = be::knob_on("BE_WINO_WAVES22");
    return on;
}

// one instantiation of k_wino_gemm_ps: its dynamic-LDS cap raised once per device, then the launch
template <int EPI, int ROWS, int EXT, int WN>
int launch_ps(const GemmArgs& g, hipStream_t s, unsigned grid) {
    constexpr size_t lds = (size_t)PS_STAGES * (128 * 16 * 4 + PS_BLOCK * 2);    // stages of 8 KB A + 12 KB B
    static be::DeviceFlags attr_set{};                          // (thread-safe)
    if (int rc_ = be::ensure_dynamic_lds(reinterpret_cast<const void*>(&k_wino_gemm_ps<EPI, ROWS, EXT, WN>), lds, attr_set)) return rc_;
    hipLaunchKernelGGL((k_wino_gemm_ps<EPI, ROWS, EXT, WN>), dim3(grid), dim3(256), lds, s, g);
    return BE_OK;
}

int wino_gemms_ps(const float* V, const float* packed_w, float* M, int64_t n, int cin, int cout, hipStream_t s,
                  const float* Vx = nullptr, const float* ds_planes = nullptr, int cin_ext = 0, int tm_force = -1) {
    const bool w22 = ps_waves22();
    const int64_t rows = (int64_t)TPI * n;
    const bool tm = tm_force >= 0 ? tm_force != 0 : wino_large(n, cout);
    const int m_tiles = (int)((rows + 127) / 128), n_tiles = (cout + 127) / 128, kchunks = cin / 16;
    const int kext = Vx ? cin_ext / 16 : 0;
    // problem groups: two workgroups fit on a CU, and a CU with one runs no faster than with two, so a launch costs rounds of two
    // workgroups per CU times a workgroup's problems x K chunks + ~2 chunks of prologue and turnover; the fewest groups of least cost
    static const int zg_env = getenv("BE_WINO_ZGROUPS") ? atoi(getenv("BE_WINO_ZGROUPS")) : 0;   // A/B knob
    const int cus = be::device_cu_count();
    int zgroups = 1;
    if (zg_env > 0 && zg_env <= NPOS) {
        zgroups = zg_env;
    } else {
        // (with the second segment a workgroup is priced by its real chunks: the extended positions are dealt evenly, so the
        // dearest group has ceil(NLIVE / zg) of them)
        int64_t best = INT64_MAX;
        for (int zg = 1; zg <= NPOS; ++zg) {
            if (NPOS % zg) continue;
            const int64_t wgs = (int64_t)m_tiles * zg * n_tiles, rounds = ((wgs + cus - 1) / cus + 1) / 2;
            const int64_t cost = rounds * ((NPOS / zg) * kchunks + (kext ? (NLIVE + zg - 1) / zg * kext : 0) + 2);
            if (cost < best) { best = cost; zgroups = zg; }
        }
    }
    // (w: the planes; wb = floats per position of them)
    const WinoStrides sv = wino_strides(tm, n, cin), sm = wino_strides(tm, n, cout);           // in floats
    GemmArgs g{V, packed_w + wino_u_floats(cout, cin), M, (int)rows, cin, cout, (int)sm.ts, NPOS, m_tiles, n_tiles, sv.plane,
               (int64_t)n_tiles * kchunks * (PS_BLOCK / 2), sm.plane, (int)sv.ts, 128, 0, nullptr, nullptr, 0, zgroups, n_tiles * 128};
    const unsigned grid = (unsigned)(8 * ((m_tiles * zgroups + 7) / 8) * n_tiles);
    if (Vx) {
        const WinoStrides sx = wino_strides(tm, n, cin_ext);
        g.x2 = Vx;
        g.w2 = ds_planes;
        g.xb2 = sx.plane;
        g.wb2 = (int64_t)n_tiles * kext * (PS_BLOCK / 2);
        g.lda2 = (int)sx.ts;
        g.kext = kext;
        g.zext = wino_ds_mask();
        // the walk: the extended positions first, dealt one at a time round the groups that still have room, then the others - the
        // groups' chunk counts are as equal as the group count allows.  (Which group computes a position changes no bit of it.)
        const int zper = (NPOS + zgroups - 1) / zgroups;
        int fill[NPOS] = {0}, order[NPOS] = {0}, grp = 0;
        for (int live = 1; live >= 0; --live)
            for (int z = 0; z < NPOS; ++z) {
                if ((int)wino_ds_live(z) != live) continue;
                while (fill[grp] >= std::min(zper, NPOS - grp * zper)) grp = (grp + 1) % zgroups;
                order[grp * zper + fill[grp]++] = z;
                grp = (grp + 1) % zgroups;
            }
        for (int i = 0; i < NPOS; ++i) g.ztab[i / 10] |= (uint64_t)order[i] << (6 * (i % 10));
        const double ext = (double)NLIVE;
        be::ProfileScope prof(s, BE_KERNEL_WINO_GEMM, 2.0 * rows * cout * ((double)NPOS * cin + ext * cin_ext),
                              4.0 * rows * ((double)NPOS * (cin + cout) + ext * cin_ext) + 6.0 * n_tiles * 128 * ((double)NPOS * cin + ext * cin_ext),
                              2.0 * m_tiles * n_tiles * 128.0 * 128.0 * ((double)NPOS * cin + ext * cin_ext));
        if (int rc_ = w22 ? launch_ps<0, 0, 1, 2>(g, s, grid) : launch_ps<0, 0, 1, 1>(g, s, grid)) return rc_;
    } else {
        // (FLOPs in fp32-equivalent products: what the layer computes, not the six bf16 products the matrix pipe issues)
        be::ProfileScope prof(s, BE_KERNEL_WINO_GEMM, (double)NPOS * 2.0 * rows * cin * cout,
                              (double)NPOS * 4.0 * ((double)rows * cin + (double)rows * cout) + (double)NPOS * 6.0 * cin * n_tiles * 128,
                              (double)NPOS * 2.0 * m_tiles * n_tiles * 128.0 * 128.0 * cin);
        if (int rc_ = w22 ? launch_ps<0, 0, 0, 2>(g, s, grid) : launch_ps<0, 0, 0, 1>(g, s, grid)) return rc_;
    }
    return be::check_launch("be_wino_conv3x3_6x6_f32(gemm, split bf16, pre-split weights)");
}

int wino_gemms(const float* V, const float* packed_w, float* M, int64_t n, int cin, int cout, hipStream_t s, void* stream,
               const float* Vx = nullptr, const float* ds_planes = nullptr, int cin_ext = 0) {
    if (Vx) {
        // only the GEMMs on pre-split weights have the second K segment
        static const bool other_arm = be::knob_on("BE_WINO_F32");
        BE_REQUIRE(!other_arm, "be_wino_conv3x3_pair_ds_6x6_f32: no folded downsample under BE_WINO_F32=1");
        return wino_gemms_ps(V, packed_w, M, n, cin, cout, s, Vx, ds_planes, cin_ext);
    }
    // A/B knob: BE_WINO_F32=1 restores the fp32-MFMA GEMMs of all three batch regimes (weight-stationary, walked 128x128, and
    // the batched k_conv_igemm of small batches)
    static const bool f32 = be::knob_on("BE_WINO_F32");
    if (!f32) return wino_gemms_ps(V, packed_w, M, n, cin, cout, s);
    const int cp = (cout + 31) / 32 * 32;
    if (wino_large(n, cout)) {
        // large batches: one workgroup per (M tile, N tile) walks the 25 problems back to back
        constexpr size_t lds = (size_t)2 * (128 + 128) * 16 * sizeof(float);
        static be::DeviceFlags attr_set{};                      // dynamic-LDS cap raised once per device (thread-safe)
        if (int rc_ = be::ensure_dynamic_lds(reinterpret_cast<const void*>(&k_wino_gemm<0>), lds, attr_set)) return rc_;
        // tile-major V [4n][25][cin] and M [4n][25][cout]: problem z = column block z of a row
        const int64_t rows = (int64_t)TPI * n;
        GemmArgs g{V, packed_w, M, (int)rows, cin, cout, NPOS * cout, NPOS, (int)((rows + 127) / 128), cp / 128,
                   (int64_t)cin, (int64_t)cp * cin, (int64_t)cout, NPOS * cin, 128, 0, nullptr, nullptr, 0};
        // weight-stationary form: full tiles only, enough M tiles to amortise the register fill, cout a multiple of 128
        static const bool no_ws = getenv("BE_WINO_NO_WS") != nullptr;               // A/B knob
        // (>= 64 row tiles: a 4096-patch half of the two-stream schedule has 2 x 4096 rows per position with the 8x5 tiles)
        static const int ws_min_tiles = getenv("BE_WINO_WS_MIN_TILES") ? atoi(getenv("BE_WINO_WS_MIN_TILES")) : (TPI == 2 ? 64 : 128);   // A/B knob
        if (!no_ws && rows % 128 == 0 && g.m_tiles >= ws_min_tiles && cout % 128 == 0) {
            if (cin == 96) return launch_ws<6>(g, s, n, cin, cout);
            if (cin == 256) return launch_ws<16>(g, s, n, cin, cout);
            if (cin == 384) return launch_ws<24>(g, s, n, cin, cout);
        }
        const unsigned grid = (unsigned)(8 * ((g.m_tiles + 7) / 8) * g.n_tiles);
        {
            be::ProfileScope prof(s, BE_KERNEL_WINO_GEMM, (double)NPOS * 2.0 * rows * cin * cout,
                                  (double)NPOS * 4.0 * ((double)rows * cin + (double)cin * cout + (double)rows * cout),
                                  (double)NPOS * 2.0 * g.m_tiles * g.n_tiles * 128.0 * 128.0 * cin);
            hipLaunchKernelGGL(k_wino_gemm<0>, dim3(grid), dim3(256), lds, s, g);
        }
        return be::check_launch("be_wino_conv3x3_6x6_f32(gemm)");
    }
    be_conv_desc d;
    d.n = (int)(TPI * n); d.h = 1; d.w = 1; d.cin = cin; d.cout = cout; d.ksize = 1; d.act = 0;
    return be_conv_nhwc_batched_f32(&d, V, packed_w, nullptr, M, cout, NPOS, (int64_t)TPI * n * cin, (int64_t)cp * cin,
                                    (int64_t)TPI * n * cout, stream);
}

int wino_args_ok(const char* who, int64_t n, int cin, int cout) {
    BE_REQUIRE(n > 0 && 4 * n < ((int64_t)1 << 31) / 128, "%s: batch out of range", who);
    BE_REQUIRE(cin % 32 == 0 && cout % 4 == 0 && cin > 0 && cout > 0, "%s: cin %% 32, cout %% 4 required", who);
    return BE_OK;
}

}  // namespace

// 1x1 convolutions and linears of large batches through the same kernel: y[M][ldy] = act(x[M][K] w[Npad][K]^T + bias (+ res)).
// The caller (conv_plan in be_conv.hip chose the route) has checked: K % 16 == 0, Npad % 128 == 0, 16-byte aligned x / w, M >= 4096.
// Same order of operations per output element as k_conv_igemm (K ascending in chunks of 16, fp32 MFMA): bit-identical.
int be::gemm_rows(const float* x, int64_t M, int K, const float* packed_w, int N, const float* bias, const float* res, int act,
                  float* y, int ldy, void* stream) {
    hipStream_t s = be::as_stream(stream);
    constexpr size_t lds = (size_t)2 * (128 + 128) * 16 * sizeof(float);
    static be::DeviceFlags attr_set{};                      // dynamic-LDS cap raised once per device (thread-safe)
    if (int rc_ = be::ensure_dynamic_lds(reinterpret_cast<const void*>(&k_wino_gemm<1>), lds, attr_set)) return rc_;
    const int cp = (N + 127) / 128 * 128, n_tiles = cp / 128;
    const int64_t tiles = (M + 127) / 128;
    // short K loops: one workgroup walks nb consecutive row tiles (only when all of them are full), about one round of
    // the 768 resident workgroups
    int nb = 1;
    if (M % 128 == 0)
        for (int c = 2; c <= 16; ++c)
            if (tiles % c == 0 && (tiles / c) * n_tiles >= 768) nb = c;
    GemmArgs g{x, packed_w, y, (int)M, K, N, ldy, nb, (int)(tiles / nb), n_tiles, (int64_t)128 * K, 0, (int64_t)128 * ldy,
               K, 128 * nb, nb > 1 ? 128 : 0, bias, res, act};
    const unsigned grid = (unsigned)(8 * ((g.m_tiles + 7) / 8) * g.n_tiles);
    {
        be::ProfileScope prof(s, BE_KERNEL_GEMM_ROWS, 2.0 * M * K * N, 4.0 * ((double)M * K + (double)K * N + (double)M * N),
                              2.0 * tiles * n_tiles * 128.0 * 128.0 * K);
        hipLaunchKernelGGL(k_wino_gemm<1>, dim3(grid), dim3(256), lds, s, g);
    }
    return be::check_launch("be_conv_nhwc_f32(gemm rows)");
}

// a plain row GEMM on the weight-stationary kernel: ONE "problem" (z = 0) of M / 128 row tiles
int be::gemm_rows_ws(const float* x, int64_t M, int K, const float* packed_w, int N, float* y, int ldy, void* stream) {
    static const bool off = getenv("BE_NO_ROWS_WS") != nullptr || getenv("BE_WINO_NO_WS") != nullptr;      // A/B knobs
    if (off || M % 128 || M / 128 < 128 || N % 128 || ldy % 4 || M * (int64_t)ldy >= ((int64_t)1 << 31)) return 1;
    if (!(K == 96 || K == 256 || K == 384) || !be::aligned16(x) || !be::aligned16(packed_w) || !be::aligned16(y)) return 1;
    hipStream_t s = be::as_stream(stream);
    GemmArgs g{x, packed_w, y, (int)M, K, N, ldy, 1, (int)(M / 128), N / 128, 0, 0, 0, K, 128, 0, nullptr, nullptr, 0};
    // (n, cin, cout of the profile record: 2 M K N FLOPs = 25 x 2 x 4 n' x cin x cout with n' = M / 100)
    if (K == 96) return launch_ws<6, 1>(g, s, M, K, N, BE_KERNEL_GEMM_ROWS);
    if (K == 256) return launch_ws<16, 1>(g, s, M, K, N, BE_KERNEL_GEMM_ROWS);
    return launch_ws<24, 1>(g, s, M, K, N, BE_KERNEL_GEMM_ROWS);
}

// ---- split-bf16 row GEMMs (round 9): LocalStage's 1x1 downsamples and fc.1 on k_wino_gemm_ps ---------------------------------------
// y[M][ldy] = act(x[M][K] w^T + bias (+ res)) with w's hi / mid / lo planes in k_wino_pack_split's block layout (one "position").
// ONE body for every M: a row's bits depend on neither the batch nor the walk (every output element sees the same K loop from a zero
// accumulator).  Without bias, residual and activation the raw-store instantiation runs (the downsamples).
extern "C" size_t be_gemm_rows_bf6_packed_floats(int cout, int cin) {
    if (cout <= 0 || cin <= 0 || cin % 16) return 0;
    return (size_t)((cout + 127) / 128 * 128) * cin * 3 / 2;
}

extern "C" int be_gemm_rows_bf6_pack_f32(const float* packed_w, int cout, int cin, float* planes, void* stream) {
    BE_REQUIRE(packed_w && planes, "be_gemm_rows_bf6_pack_f32: null pointer");
    BE_REQUIRE(cout > 0 && cin > 0 && cin % 16 == 0, "be_gemm_rows_bf6_pack_f32: cin must be a multiple of 16 (got %d)", cin);
    BE_REQUIRE(be::aligned16(packed_w) && be::aligned16(planes), "be_gemm_rows_bf6_pack_f32: packed_w / planes must be 16-byte aligned");
    const int cp = (cout + 31) / 32 * 32, n_tiles = (cout + 127) / 128;     // the fp32 matrix: [cout_pad32][cin], zero rows past cout
    hipLaunchKernelGGL(k_wino_pack_split, dim3(grid_cap((int64_t)128 * n_tiles * (cin / 8), 256, 4096)), dim3(256), 0,
                       be::as_stream(stream), packed_w, 1, cp, cin, n_tiles, reinterpret_cast<__bf16*>(planes));
    return be::check_launch("be_gemm_rows_bf6_pack_f32");
}

bool be::rows_bf6_enabled() {
    // A/B knobs: BE_ROWS_F32=1 sends only these row GEMMs back to the fp32 kernels; BE_WINO_F32=1 restores fp32 everywhere
    static const bool f32 = be::knob_on("BE_ROWS_F32") || be::knob_on("BE_WINO_F32");
    return !f32;
}

int be::gemm_rows_bf6(const float* x, int64_t M, int K, const float* planes, int N, const float* bias, const float* res, int act,
                      float* y, int ldy, void* stream) {
    BE_REQUIRE(x && planes && y, "be_gemm_rows_bf6_f32: null pointer");
    BE_REQUIRE(M > 0 && M < ((int64_t)1 << 31) - 128 && K > 0 && K % 16 == 0 && N > 0 && ldy >= N && (unsigned)act <= 2u,
               "be_gemm_rows_bf6_f32: bad shape (M %lld, K %d, N %d, ldy %d, act %d; K %% 16 == 0)", (long long)M, K, N, ldy, act);
    BE_REQUIRE((int64_t)128 * std::max(K, ldy) * 4 < ((int64_t)1 << 31), "be_gemm_rows_bf6_f32: rows too long");
    BE_REQUIRE(be::aligned16(x) && be::aligned16(planes), "be_gemm_rows_bf6_f32: x / planes must be 16-byte aligned");
    hipStream_t s = be::as_stream(stream);
    const int n_tiles = (N + 127) / 128, kchunks = K / 16;
    const int64_t tiles = (M + 127) / 128;
    // short K loops: one workgroup walks nb consecutive row tiles (only when all of them are full).  Cost as for the Winograd problem
    // groups: rounds of two workgroups per CU times a workgroup's tiles x K chunks + ~2 chunks of prologue and turnover; a walk is worth
    // it only while a tile's loop is short (<= 16 chunks)
    static const int nb_env = getenv("BE_ROWS_WALK") ? atoi(getenv("BE_ROWS_WALK")) : 0;         // A/B knob: tiles per workgroup
    int nb = 1;
    if (nb_env > 0) {
        if (M % 128 == 0 && tiles % nb_env == 0) nb = nb_env;
    } else if (M % 128 == 0 && kchunks <= 16) {
        const int cus = be::device_cu_count();
        int64_t best = INT64_MAX;
        for (int c = 1; c <= 16; ++c) {
            if (tiles % c) continue;
            const int64_t wgs = (tiles / c) * n_tiles, rounds = ((wgs + cus - 1) / cus + 1) / 2;
            const int64_t cost = rounds * ((int64_t)c * kchunks + 2);
            if (cost <= best) { best = cost; nb = c; }
        }
    }
    const int m_tiles = (int)(tiles / nb);
    GemmArgs g{x, planes, y, (int)M, K, N, ldy, nb, m_tiles, n_tiles, (int64_t)128 * K, 0, (int64_t)128 * ldy,
               K, 128 * nb, nb > 1 ? 128 : 0, bias, res, act, 1, n_tiles * 128};
    const unsigned grid = (unsigned)(8 * ((m_tiles + 7) / 8) * n_tiles);
    {
        // (FLOPs in fp32-equivalent products, as the Winograd GEMMs)
        be::ProfileScope prof(s, BE_KERNEL_GEMM_ROWS, 2.0 * M * K * N, 4.0 * ((double)M * K + (double)M * N) + 6.0 * K * n_tiles * 128,
                              2.0 * tiles * n_tiles * 128.0 * 128.0 * K);
        // (<1, 1>, fc.1, keeps its one-set loop on the 2x2 grid; the raw-store GEMM follows the Winograd GEMMs' grid)
        const int rc = (bias || res || act) ? launch_ps<1, 1, 0, 2>(g, s, grid)
                       : ps_waves22()       ? launch_ps<0, 1, 0, 2>(g, s, grid)
                                            : launch_ps<0, 1, 0, 1>(g, s, grid);
        if (rc) return rc;
    }
    return be::check_launch("be_gemm_rows_bf6_f32");
}

extern "C" int be_gemm_rows_bf6_f32(const float* x, int64_t m, int k, const float* planes, int n, const float* bias,
                                    const float* residual, int act, float* y, int ldy, void* stream) {
    return be::gemm_rows_bf6(x, m, k, planes, n, bias, residual, act, y, ldy, stream);
}

// a transform kernel over `threads` threads of its grid-stride loop, 256 to a workgroup
template <class... P, class... A>
static void launch_transform(void (*kernel)(P...), int64_t threads, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_cap(threads, 256)), dim3(256), 0, s, static_cast<P>(args)...);
}

extern "C" int be_wino_conv3x3_6x6_f32(const float* x, const float* packed_w, const float* packed_bias, const float* residual,
                                       float* y, int64_t n, int cin, int cout, int act, float* workspace,
                                       size_t workspace_floats, void* stream) {
    BE_REQUIRE(x && packed_w && packed_bias && y && workspace, "be_wino_conv3x3_6x6_f32: null pointer");
    if (int rc = wino_args_ok("be_wino_conv3x3_6x6_f32", n, cin, cout)) return rc;
    BE_REQUIRE(workspace_floats >= be_wino_workspace_floats(n, cin, cout), "be_wino_conv3x3_6x6_f32: workspace too small");
    BE_REQUIRE(be::aligned16(x) && be::aligned16(y) && be::aligned16(workspace) && be::aligned16(packed_w),
               "be_wino_conv3x3_6x6_f32: 16-byte alignment");
    hipStream_t s = be::as_stream(stream);
    float* V = workspace;
    float* M = workspace + (size_t)100 * n * cin;
    const int tm = wino_large(n, cout);
    launch_transform(k_wino_in, n * TPI * (cin / 4), s, x, V, n, cin / 4, tm);
    if (int rc = be::check_launch("be_wino_conv3x3_6x6_f32(in)")) return rc;
    if (int rc = wino_gemms(V, packed_w, M, n, cin, cout, s, stream)) return rc;
    launch_transform(k_wino_out<>, n * TPI * (cout / VW_OUT), s, M, packed_bias, residual, y, n, cout / VW_OUT, act, tm);
    return be::check_launch("be_wino_conv3x3_6x6_f32(out)");
}

extern "C" size_t be_wino_pair_workspace_floats(int64_t n, int cin, int cmid, int cout) {
    if (n <= 0) return 0;
    const size_t big = (size_t)(cin > cmid ? cin : cmid), out = (size_t)(cmid > cout ? cmid : cout);
    return (size_t)100 * n * (big + out);                       // V (cin, then cmid) + M (cmid, then cout)
}

// The pair with the downsample folded into conv2's GEMMs keeps x's transform alive beside conv1's: three regions, V_x (cin; a
// following block's transform, cout channels, is written there once conv2's GEMMs have run), M (cmid, then cout) and V_h (cmid)
extern "C" size_t be_wino_pair_ds_workspace_floats(int64_t n, int cin, int cmid, int cout) {
    if (n <= 0) return 0;
    const size_t first = (size_t)(cin > cout ? cin : cout), out = (size_t)(cmid > cout ? cmid : cout);
    return (size_t)100 * n * (first + out + (size_t)cmid);
}

// pool2 = 1: y is [n,3,3,cout], the 2x2 max-pool of the block's output (k_wino_out_pool2)
// x_in_v = 1: the start of the workspace already holds x's input transform in this block's layout (left there by the block or the
// pool kernel in front: k_wino_in is skipped).  next_cmid > 0: the last launch is k_wino_out_res_in, which writes y and, at the
// start of the workspace, y's input transform for a following block whose conv1 has next_cmid outputs.
// packed_ds != nullptr (round 14; be_wino_conv3x3_pair_ds_6x6_f32): the block's 1x1 downsample (be_wino_ds_pack_f32) runs inside
// conv2's GEMMs as a second K segment over x's transform; there is no residual tensor, the workspace has three regions
// (be_wino_pair_ds_workspace_floats: x's transform outlives k_wino_out_in), x may be null with x_in_v and y with next_cmid > 0
// (the map is then not stored: nothing reads it).
int be::wino_pair(const float* x, const float* packed_w1, const float* packed_bias1, int act1, const float* packed_w2,
                  const float* packed_bias2, const float* residual, int act2, float* y, int64_t n, int cin, int cmid, int cout,
                  float* workspace, size_t workspace_floats, void* stream, int pool2, int x_in_v, int next_cmid, const float* packed_ds) {
    const bool ds = packed_ds != nullptr;
    const float* ds_planes = ds ? packed_ds + wino_ds_u_floats(cout, cin) : nullptr;
    BE_REQUIRE((x || (ds && x_in_v)) && packed_w1 && packed_bias1 && packed_w2 && packed_bias2 && (y || (ds && next_cmid > 0)) && workspace,
               "be_wino_conv3x3_pair_6x6_f32: null pointer");
    if (int rc = wino_args_ok("be_wino_conv3x3_pair_6x6_f32", n, cin, cmid)) return rc;
    if (int rc = wino_args_ok("be_wino_conv3x3_pair_6x6_f32", n, cmid, cout)) return rc;
    BE_REQUIRE(workspace_floats >= (ds ? be_wino_pair_ds_workspace_floats(n, cin, cmid, cout) : be_wino_pair_workspace_floats(n, cin, cmid, cout)),
               "be_wino_conv3x3_pair_6x6_f32: workspace too small");
    BE_REQUIRE(be::aligned16(x) && be::aligned16(y) && be::aligned16(workspace) && be::aligned16(packed_w1) && be::aligned16(packed_w2) &&
               be::aligned16(packed_ds), "be_wino_conv3x3_pair_6x6_f32: 16-byte alignment");
    hipStream_t s = be::as_stream(stream);
    const size_t big = ds ? (size_t)(cin > cout ? cin : cout) : (size_t)(cin > cmid ? cin : cmid);
    float* V = workspace;                                       // x's transform; without ds then also conv1's result's
    float* M = workspace + (size_t)100 * n * big;
    float* Vh = ds ? M + (size_t)100 * n * (size_t)(cmid > cout ? cmid : cout) : V;
    const int tm1 = wino_large(n, cmid), tm2 = wino_large(n, cout);
    BE_REQUIRE(next_cmid >= 0 && !(next_cmid > 0 && pool2), "be_wino_conv3x3_pair_6x6_f32: next_cmid cannot be combined with pool2");
    if (ds) {
        BE_REQUIRE(!residual, "be_wino_conv3x3_pair_ds_6x6_f32: the folded downsample replaces the residual tensor");
        BE_REQUIRE(tm1 == tm2, "be_wino_conv3x3_pair_ds_6x6_f32: x's transform and conv1's must share a layout (cmid %d, cout %d)", cmid, cout);
    }
    if (next_cmid > 0) {
        if (int rc = wino_args_ok("be_wino_conv3x3_pair_6x6_f32", n, cout, next_cmid)) return rc;
        // the boundary kernel writes V' while it reads M: V' must end where M starts at the latest
        BE_REQUIRE((size_t)(NPOS * TPI) * n * cout <= (size_t)100 * n * big,
                   "be_wino_conv3x3_pair_6x6_f32: the next block's transform (cout %d) would reach M (%s = %d)", cout,
                   ds ? "max(cin, cout)" : "max(cin, cmid)", (int)big);
    }
    if (!x_in_v) {
        be::ProfileScope prof(s, BE_KERNEL_WINO_TRANSFORM, 0.0, 4.0 * n * cin * (36.0 + (double)(NPOS * TPI)), 0.0);
        launch_transform(k_wino_in, n * TPI * (cin / 4), s, x, V, n, cin / 4, tm1);
    }
    if (int rc = be::check_launch("be_wino_conv3x3_pair_6x6_f32(in)")) return rc;
    if (int rc = wino_gemms(V, packed_w1, M, n, cin, cmid, s, stream)) return rc;
    {
        be::ProfileScope prof(s, BE_KERNEL_WINO_TRANSFORM, 0.0, 4.0 * n * cmid * (2.0 * NPOS * TPI), 0.0);
        launch_transform(k_wino_out_in<>, n * (cmid / VW_OUT), s, M, packed_bias1, Vh, n, cmid / VW_OUT, act1, tm1, tm2);
    }
    if (int rc = be::check_launch("be_wino_conv3x3_pair_6x6_f32(out_in)")) return rc;
    if (int rc = wino_gemms(Vh, packed_w2, M, n, cmid, cout, s, stream, ds ? V : nullptr, ds_planes, cin)) return rc;
    {
        be::ProfileScope prof(s, BE_KERNEL_WINO_TRANSFORM, 0.0, 4.0 * n * cout * ((double)(NPOS * TPI) + (residual ? 36.0 : 0.0) +
                                                                                   (pool2 ? 9.0 : y ? 36.0 : 0.0) +
                                                                                   (next_cmid > 0 ? (double)(NPOS * TPI) : 0.0)), 0.0);
        const int c4 = cout / VW_OUT, tm_next = next_cmid > 0 ? (int)wino_large(n, next_cmid) : 0;
        if (next_cmid > 0 && !y)
            launch_transform(k_wino_out_res_in<VW_OUT, 0>, n * c4, s, M, packed_bias2, residual, y, V, n, c4, act2, tm2, tm_next);
        else if (next_cmid > 0)
            launch_transform(k_wino_out_res_in<>, n * c4, s, M, packed_bias2, residual, y, V, n, c4, act2, tm2, tm_next);
        else if (pool2)
            launch_transform(k_wino_out_pool2<>, n * c4, s, M, packed_bias2, residual, y, n, c4, act2, tm2);
        else
            launch_transform(k_wino_out<>, n * TPI * c4, s, M, packed_bias2, residual, y, n, c4, act2, tm2);
    }
    return be::check_launch("be_wino_conv3x3_pair_6x6_f32(out)");
}

extern "C" int be_wino_conv3x3_pair_6x6_f32(const float* x, const float* packed_w1, const float* packed_bias1, int act1,
                                            const float* packed_w2, const float* packed_bias2, const float* residual, int act2,
                                            float* y, int64_t n, int cin, int cmid, int cout, float* workspace,
                                            size_t workspace_floats, void* stream) {
    return be::wino_pair(x, packed_w1, packed_bias1, act1, packed_w2, packed_bias2, residual, act2, y, n, cin, cmid, cout, workspace,
                         workspace_floats, stream, 0);
}

extern "C" int be_wino_conv3x3_pair_chain_6x6_f32(const float* x, const float* packed_w1, const float* packed_bias1, int act1,
                                                  const float* packed_w2, const float* packed_bias2, const float* residual, int act2,
                                                  float* y, int64_t n, int cin, int cmid, int cout, float* workspace,
                                                  size_t workspace_floats, void* stream, int x_in_v, int next_cmid) {
    return be::wino_pair(x, packed_w1, packed_bias1, act1, packed_w2, packed_bias2, residual, act2, y, n, cin, cmid, cout, workspace,
                         workspace_floats, stream, 0, x_in_v, next_cmid);
}

// The folded pair (round 14): be_wino_conv3x3_pair_chain_6x6_f32 with the block's 1x1 downsample inside conv2's GEMMs
// (packed_ds: be_wino_ds_pack_f32; its bias belongs in packed_bias2) instead of a residual tensor
extern "C" int be_wino_conv3x3_pair_ds_6x6_f32(const float* x, const float* packed_w1, const float* packed_bias1, int act1,
                                               const float* packed_w2, const float* packed_bias2, const float* packed_ds, int act2,
                                               float* y, int64_t n, int cin, int cmid, int cout, float* workspace,
                                               size_t workspace_floats, void* stream, int x_in_v, int next_cmid) {
    BE_REQUIRE(packed_ds, "be_wino_conv3x3_pair_ds_6x6_f32: null pointer");
    return be::wino_pair(x, packed_w1, packed_bias1, act1, packed_w2, packed_bias2, nullptr, act2, y, n, cin, cmid, cout, workspace,
                         workspace_floats, stream, 0, x_in_v, next_cmid, packed_ds);
}

// The transform-domain GEMMs alone on k_wino_gemm_ps: M[z] = V[z] U[z]^T and, with Vx, + Vx[z] U_ds[z]^T at U_ds's positions.
// V [positions][tiles][cin] (tile_major = 0) or [tiles][positions][cin] (1), tiles = (12 / be_wino_tile_rows()) n; Vx and M likewise
extern "C" int be_wino_gemms_ext_f32(const float* V, const float* packed_w, float* M, int64_t n, int cin, int cout, const float* Vx,
                                     const float* packed_ds, int cin_ext, int tile_major, void* stream) {
    BE_REQUIRE(V && packed_w && M && (Vx == nullptr) == (packed_ds == nullptr), "be_wino_gemms_ext_f32: null pointer");
    BE_REQUIRE(n > 0 && 4 * n < ((int64_t)1 << 31) / 128, "be_wino_gemms_ext_f32: batch out of range");
    BE_REQUIRE(cin > 0 && cin % 16 == 0 && cout > 0 && cout % 4 == 0, "be_wino_gemms_ext_f32: cin %% 16, cout %% 4 required");
    BE_REQUIRE(!Vx || (cin_ext > 0 && cin_ext % 16 == 0), "be_wino_gemms_ext_f32: cin_ext must be a multiple of 16 (got %d)", cin_ext);
    BE_REQUIRE((int64_t)NPOS * TPI * n * (int64_t)std::max(std::max(cin, cout), cin_ext) < ((int64_t)1 << 31), "be_wino_gemms_ext_f32: batch out of range");
    BE_REQUIRE(be::aligned16(V) && be::aligned16(packed_w) && be::aligned16(M) && be::aligned16(Vx) && be::aligned16(packed_ds),
               "be_wino_gemms_ext_f32: 16-byte alignment");
    return wino_gemms_ps(V, packed_w, M, n, cin, cout, be::as_stream(stream), Vx, Vx ? packed_ds + wino_ds_u_floats(cout, cin_ext) : nullptr,
                         cin_ext, tile_major != 0);
}

bool be::wino_ds_fold_enabled() {
    // A/B knob BE_WINO_DS_GEMM=1: the blocks' downsamples stay separate row GEMMs; so they do in the arms without the second K segment
    static const bool on = be::rows_bf6_enabled() && !be::knob_on("BE_WINO_DS_GEMM");
    return on;
}

int be::pool_wino_in(const float* x, float* pooled, int64_t n, int c, int next_cmid, float* workspace, size_t workspace_floats, void* stream) {
    BE_REQUIRE(x && workspace, "be_maxpool_wino_in_11x11_f32: null pointer");
    if (int rc = wino_args_ok("be_maxpool_wino_in_11x11_f32", n, c, next_cmid)) return rc;
    BE_REQUIRE(workspace_floats >= (size_t)(NPOS * TPI) * n * c, "be_maxpool_wino_in_11x11_f32: workspace too small");
    BE_REQUIRE(be::aligned16(x) && be::aligned16(pooled) && be::aligned16(workspace), "be_maxpool_wino_in_11x11_f32: 16-byte alignment");
    hipStream_t s = be::as_stream(stream);
    {
        be::ProfileScope prof(s, BE_KERNEL_WINO_TRANSFORM, 0.0, 4.0 * n * c * (121.0 + (pooled ? 36.0 : 0.0) + (double)(NPOS * TPI)), 0.0);
        const int c4 = c / VW_OUT, tm_next = (int)wino_large(n, next_cmid);
        if (pooled)
            launch_transform(k_pool_wino_in<>, n * c4, s, x, pooled, workspace, n, c4, tm_next);
        else
            launch_transform(k_pool_wino_in<VW_OUT, 0>, n * c4, s, x, pooled, workspace, n, c4, tm_next);
    }
    return be::check_launch("be_maxpool_wino_in_11x11_f32");
}

extern "C" int be_maxpool_wino_in_11x11_f32(const float* x, float* pooled, int64_t n, int c, int next_cmid, float* workspace,
                                            size_t workspace_floats, void* stream) {
    BE_REQUIRE(pooled, "be_maxpool_wino_in_11x11_f32: null pointer");
    return be::pool_wino_in(x, pooled, n, c, next_cmid, workspace, workspace_floats, stream);
}
