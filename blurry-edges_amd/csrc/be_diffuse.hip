// Dense depth from sparse samples by edge-aware diffusion (be_fill_diffuse_f32): the holes take the harmonic
// interpolant of the seeds' boundary values, u_p sum_q c_pq = sum_q c_pq u_q over the 4-neighbours inside the image, with the
// conductance c_pq = max(leak, 1 - max(e_p, e_q)) of an edge map e clamped to [0, 1].  Where nearest-sample fill puts a step halfway
// between two samples of a slanted surface, this puts the plane through them, and an edge keeps two surfaces from mixing.
//
// The start is be_fill_nearest_f32's result.  A pyramid of 2 x 2 poolings (boundary values, seed mask, edge map, start value) is
// relaxed from the coarsest level up, every level handing its result to the holes of the next finer one (cascadic): the levels only
// accelerate, the finest level's equations are the problem's.  A level is relaxed by red-black over-relaxed sweeps on LDS regions
// of up to 128 x 128, many sweeps per launch: Gauss-Seidel inside a region, block-Jacobi between the 96 x 96 tiles of a level
// larger than one region, whose 16-pixel halo is refreshed by the next launch.  The number of launches and sweeps is a function of
// (H, W, iters) alone; nothing depends on the data, nothing synchronises with the host, and no float is accumulated atomically, so
// the result is a function of the inputs.  All float arithmetic is float32 with one rounding per written operation (no contraction):
// be_hip/diffuse.py restates the pyramid and the sweeps in numpy, operation by operation, and the tests hold the kernels to it.
#include <cmath>
#include <cstdint>
#include "be_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DIFF_MAX_SIDE = 16384;
constexpr int DIFF_MAX_R = 8;
constexpr int DIFF_MAX_ITERS = 4096;
constexpr int TILE = 96, HALO = 16, REGION = TILE + 2 * HALO;      // 128: a region's u is 66 KB of LDS
constexpr int COARSEST = 4;                                        // the pyramid stops when the longer side is <= 4
constexpr int PER_LAUNCH = 16;                                     // sweeps per launch on a level of several tiles (= HALO)
constexpr int MAX_LEVELS = 16;
constexpr int THREADS = 1024, LANES_X = 64, LANES_Y = 16;          // a thread owns rows ly + 16 t (t < 8) and one pixel per colour there
constexpr int ROWS = REGION / LANES_Y;                             // 8
constexpr int STRIDE = REGION + 2;                                 // LDS rows: one cell of padding (0) on every side of the region

struct Level {
    int H, W;
    float* u[2];                                                   // double buffered between launches
    float* e;                                                      // the edge map, clamped to [0, 1]
    uint8_t* fixed;                                                // 1: a seed (or a cell that holds one)
};

__device__ __forceinline__ float clamp_edge(float e) { return e > 0.0f ? fminf(e, 1.0f) : 0.0f; }          // NaN -> 0
__device__ __forceinline__ float link(float leak, float ep, float eq) { return fmaxf(leak, 1.0f - fmaxf(ep, eq)); }

// level 0 from the nearest-sample fill: a seed (index[p] == p) holds its boundary value (its robust local mean, its depth when
// mean is null), a hole the depth nearest-sample fill gave it
__global__ __launch_bounds__(256) void k_diffuse_init(const float* __restrict__ depth, const float* __restrict__ near,
                                                      const int32_t* __restrict__ index, const float* __restrict__ mean,
                                                      const float* __restrict__ edge, int N, float* __restrict__ u,
                                                      float* __restrict__ e, uint8_t* __restrict__ fixed) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const bool seed = index[p] == p;
    u[p] = seed ? (mean ? mean[p] : depth[p]) : near[p];
    e[p] = edge ? clamp_edge(edge[p]) : 0.0f;
    fixed[p] = seed ? 1 : 0;
}

// 2 x 2 pooling, one thread per cell of the coarser level (a cell at an odd border holds fewer pixels): fixed = any; u = the mean
// of the cell's fixed pixels where there is one, of all its pixels otherwise, summed in row-major order; e = max
__global__ __launch_bounds__(256) void k_diffuse_pool(const float* __restrict__ u, const float* __restrict__ e,
                                                      const uint8_t* __restrict__ fixed, int H, int W, float* __restrict__ uc,
                                                      float* __restrict__ ec, uint8_t* __restrict__ fc, int h, int w) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= h * w) return;
    const int cy = c / w, cx = c - cy * w;
    float su = 0.0f, sf = 0.0f, nu = 0.0f, nf = 0.0f, em = 0.0f;
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int y = 2 * cy + dy, x = 2 * cx + dx;
            if (y >= H || x >= W) continue;
            const int p = y * W + x;
            const float v = u[p];
            su += v;
            nu += 1.0f;
            if (fixed[p]) { sf += v; nf += 1.0f; }
            em = fmaxf(em, e[p]);
        }
    uc[c] = nf > 0.0f ? sf / nf : su / nu;
    ec[c] = em;
    fc[c] = nf > 0.0f ? 1 : 0;
}

// `sweeps` red-black over-relaxed sweeps on one region per workgroup.  The region is the whole level on an axis where the level is
// at most 128 long (tiled = 0), else the 96-wide tile plus 16 on both sides, whose outermost ring stays as loaded.  A hole's start
// value comes from `coarse` (the level below, piecewise constant) on the first launch of a level, from src otherwise.  Every
// thread keeps the four weights c_q / sum c of its (up to) 16 pixels in registers, so a sweep reads u alone; a pixel that is fixed,
// on the ring or outside the level has a cleared bit in `free_mask`.  The tile is written to dst.
__global__ __launch_bounds__(THREADS) void k_diffuse_relax(const float* __restrict__ src, float* __restrict__ dst,
                                                           const float* __restrict__ coarse, int wc, const float* __restrict__ e,
                                                           const uint8_t* __restrict__ fixed, int H, int W, int tiled_y, int tiled_x,
                                                           float leak, float omega, int sweeps) {
    __shared__ float u[STRIDE * STRIDE];
    const int rh = tiled_y ? REGION : H, rw = tiled_x ? REGION : W;                  // the region held
    const int oy = tiled_y ? (int)blockIdx.y * TILE - HALO : 0, ox = tiled_x ? (int)blockIdx.x * TILE - HALO : 0;
    for (int i = threadIdx.x; i < STRIDE * STRIDE; i += THREADS) {
        const int ry = i / STRIDE - 1, rx = i % STRIDE - 1;
        const int gy = oy + ry, gx = ox + rx;
        float v = 0.0f;                                                              // the padding, and what lies outside the level
        if (ry >= 0 && ry < rh && rx >= 0 && rx < rw && gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int g = gy * W + gx;
            v = (coarse && !fixed[g]) ? coarse[(gy >> 1) * wc + (gx >> 1)] : src[g];
        }
        u[i] = v;
    }
    const int lx = threadIdx.x & (LANES_X - 1), ly = threadIdx.x / LANES_X;
    float wgt[2][ROWS][4];                                                           // north, south, west, east
    unsigned free_mask = 0;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < ROWS; ++t) {
            const int ry = ly + LANES_Y * t;
            const int gy = oy + ry;
            const int rx = 2 * lx + ((c + gy + ox) & 1), gx = ox + rx;
            bool ok = ry < rh && rx < rw && gy >= 0 && gy < H && gx >= 0 && gx < W;
            ok = ok && !(tiled_y && (ry == 0 || ry == REGION - 1)) && !(tiled_x && (rx == 0 || rx == REGION - 1));
            float cn = 0.0f, cs = 0.0f, cw = 0.0f, ce = 0.0f;
            if (ok) {
                const int g = gy * W + gx;
                ok = !fixed[g];
                if (ok) {
                    const float ep = e[g];
                    if (gy > 0) cn = link(leak, ep, e[g - W]);
                    if (gy < H - 1) cs = link(leak, ep, e[g + W]);
                    if (gx > 0) cw = link(leak, ep, e[g - 1]);
                    if (gx < W - 1) ce = link(leak, ep, e[g + 1]);
                }
            }
            float den = ((cn + cs) + cw) + ce;
            den = den > 0.0f ? den : 1.0f;
            wgt[c][t][0] = cn / den;
            wgt[c][t][1] = cs / den;
            wgt[c][t][2] = cw / den;
            wgt[c][t][3] = ce / den;
            if (ok) free_mask |= 1u << (c * ROWS + t);
        }
    __syncthreads();
    // rows ly + 16 t have the parity of ly, so a colour's pixels of one thread share their column: one address per colour
    float* const at[2] = {u + (ly + 1) * STRIDE + 1 + 2 * lx + ((0 + oy + ly + ox) & 1),
                          u + (ly + 1) * STRIDE + 1 + 2 * lx + ((1 + oy + ly + ox) & 1)};
    for (int s = 0; s < sweeps; ++s) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int t = 0; t < ROWS; ++t) {
                if (free_mask >> (c * ROWS + t) & 1u) {
                    float* const q = at[c] + t * LANES_Y * STRIDE;                   // a neighbour that does not exist has weight 0
                    const float un = q[-STRIDE], us = q[STRIDE], uw = q[-1], ue = q[1], v = q[0];
                    const float avg = ((wgt[c][t][0] * un + wgt[c][t][1] * us) + wgt[c][t][2] * uw) + wgt[c][t][3] * ue;
                    q[0] = v + omega * (avg - v);
                }
            }
            __syncthreads();
        }
    }
    // the tile: the whole region on an axis that is not tiled
    const int y0 = tiled_y ? (int)blockIdx.y * TILE : 0, y1 = tiled_y ? min(y0 + TILE, H) : H;
    const int x0 = tiled_x ? (int)blockIdx.x * TILE : 0, x1 = tiled_x ? min(x0 + TILE, W) : W;
    const int tw = x1 - x0, tn = (y1 - y0) * tw;
    for (int i = threadIdx.x; i < tn; i += THREADS) {
        const int y = y0 + i / tw, x = x0 + i % tw;
        dst[y * W + x] = u[(y - oy + 1) * STRIDE + (x - ox + 1)];
    }
}

// the outputs: depth_out = the input at a seed, u at a hole; residual = max over the holes of |avg - u|, avg = sum c u / sum c,
// as the integer maximum of the bits of a non-negative float (order independent)
__global__ __launch_bounds__(256) void k_diffuse_finish(const float* __restrict__ depth, const float* __restrict__ u,
                                                        const float* __restrict__ e, const uint8_t* __restrict__ fixed, int H, int W,
                                                        float leak, float* __restrict__ depth_out, unsigned* __restrict__ residual) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    float r = 0.0f;
    if (p < H * W) {
        const float v = u[p];
        if (fixed[p]) {
            depth_out[p] = depth[p];
        } else {
            depth_out[p] = v;
            const int y = p / W, x = p - y * W;
            const float ep = e[p];
            float num = 0.0f, den = 0.0f;
            if (y > 0) { const float c = link(leak, ep, e[p - W]); num += c * u[p - W]; den += c; }
            if (y < H - 1) { const float c = link(leak, ep, e[p + W]); num += c * u[p + W]; den += c; }
            if (x > 0) { const float c = link(leak, ep, e[p - 1]); num += c * u[p - 1]; den += c; }
            if (x < W - 1) { const float c = link(leak, ep, e[p + 1]); num += c * u[p + 1]; den += c; }
            if (den > 0.0f) r = fabsf(num / den - v);
            if (!(r >= 0.0f)) r = 0.0f;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) r = fmaxf(r, __shfl_xor(r, off));
    if ((threadIdx.x & 63) == 0 && r > 0.0f) atomicMax(residual, __float_as_uint(r));
}

int level_sizes(int H, int W, int* hs, int* ws) {
    int n = 0;
    hs[n] = H, ws[n] = W, ++n;
    while ((hs[n - 1] > ws[n - 1] ? hs[n - 1] : ws[n - 1]) > COARSEST) {
        hs[n] = (hs[n - 1] + 1) / 2, ws[n] = (ws[n - 1] + 1) / 2;
        ++n;
    }
    return n;
}

// int32 words: be_fill_nearest_f32's three images, then per level u (twice), e and the fixed bytes
int64_t level_words(int h, int w) { return 3 * (int64_t)h * w + ((int64_t)h * w + 3) / 4; }

}  // namespace

extern "C" int64_t be_fill_diffuse_scratch_bytes(int H, int W) {
    if (H < 1 || W < 1 || H > DIFF_MAX_SIDE || W > DIFF_MAX_SIDE) return -1;
    int hs[MAX_LEVELS], ws[MAX_LEVELS];
    const int L = level_sizes(H, W, hs, ws);
    int64_t words = 3 * (int64_t)H * W;
    for (int l = 0; l < L; ++l) words += level_words(hs[l], ws[l]);
    return 4 * words;
}

extern "C" int be_fill_diffuse_f32(const float* depth, const float* weight, const float* edge, int H, int W, int smooth_r, float sigma_z,
                                   float leak, int iters, int fuse, int32_t* scratch, float* depth_out, int32_t* index, int32_t* dist2,
                                   float* residual, void* stream) {
    BE_REQUIRE(depth && scratch && depth_out && index && dist2 && residual, "be_fill_diffuse_f32: null pointer");
    BE_REQUIRE(H >= 1 && W >= 1 && H <= DIFF_MAX_SIDE && W <= DIFF_MAX_SIDE, "be_fill_diffuse_f32: H and W must be in [1, %d], got %d x %d",
               DIFF_MAX_SIDE, H, W);
    BE_REQUIRE(smooth_r >= 0 && smooth_r <= DIFF_MAX_R, "be_fill_diffuse_f32: smooth_r must be in [0, %d], got %d", DIFF_MAX_R, smooth_r);
    BE_REQUIRE(sigma_z > 0.0f && sigma_z < __builtin_inff(), "be_fill_diffuse_f32: sigma_z must be a finite number > 0");
    BE_REQUIRE(leak > 0.0f && leak <= 1.0f, "be_fill_diffuse_f32: leak must be in (0, 1]");
    BE_REQUIRE(iters >= 0 && iters <= DIFF_MAX_ITERS, "be_fill_diffuse_f32: iters must be in [0, %d] (0: the default schedule), got %d",
               DIFF_MAX_ITERS, iters);
    BE_REQUIRE(fuse == 0 || fuse == 1, "be_fill_diffuse_f32: fuse must be 0 or 1, got %d", fuse);
    hipStream_t st = be::as_stream(stream);
    const int N = H * W;
    // the start value, index and dist2; be_fill_nearest_f32 leaves the per-seed means in the third image of its scratch
    if (const int rc = be_fill_nearest_f32(depth, weight, H, W, smooth_r, sigma_z, 1, scratch, depth_out, index, dist2, stream)) return rc;
    const float* mean = smooth_r > 0 ? reinterpret_cast<const float*>(scratch + 2 * (int64_t)N) : nullptr;
    if (hipMemsetAsync(residual, 0, sizeof(float), st) != hipSuccess) return be::check_launch("be_fill_diffuse_f32(memset)");

    int hs[MAX_LEVELS], ws[MAX_LEVELS];
    const int L = level_sizes(H, W, hs, ws);
    Level lv[MAX_LEVELS];
    int32_t* at = scratch + 3 * (int64_t)N;
    for (int l = 0; l < L; ++l) {
        const int64_t n = (int64_t)hs[l] * ws[l];
        lv[l].H = hs[l], lv[l].W = ws[l];
        lv[l].u[0] = reinterpret_cast<float*>(at);
        lv[l].u[1] = reinterpret_cast<float*>(at + n);
        lv[l].e = reinterpret_cast<float*>(at + 2 * n);
        lv[l].fixed = reinterpret_cast<uint8_t*>(at + 3 * n);
        at += level_words(hs[l], ws[l]);
    }
    hipLaunchKernelGGL(k_diffuse_init, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, depth, (const float*)depth_out,
                       (const int32_t*)index, mean, edge, N, lv[0].u[0], lv[0].e, lv[0].fixed);
    if (const int rc = be::check_launch("be_fill_diffuse_f32(init)")) return rc;
    for (int l = 1; l < L; ++l) {
        const int n = lv[l].H * lv[l].W;
        hipLaunchKernelGGL(k_diffuse_pool, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)lv[l - 1].u[0],
                           (const float*)lv[l - 1].e, (const uint8_t*)lv[l - 1].fixed, lv[l - 1].H, lv[l - 1].W, lv[l].u[0], lv[l].e,
                           lv[l].fixed, lv[l].H, lv[l].W);
        if (const int rc = be::check_launch("be_fill_diffuse_f32(pool)")) return rc;
    }
    const float* coarse = nullptr;                                  // the relaxed level below
    const float* result = lv[0].u[0];
    for (int l = L - 1; l >= 0; --l) {
        const int h = lv[l].H, w = lv[l].W, side = h > w ? h : w;
        const int ty = h <= REGION ? 0 : 1, tx = w <= REGION ? 0 : 1;
        const dim3 grid(tx ? (unsigned)((w + TILE - 1) / TILE) : 1u, ty ? (unsigned)((h + TILE - 1) / TILE) : 1u);
        const int total = iters > 0 ? iters : (4 * side + PER_LAUNCH - 1) / PER_LAUNCH * PER_LAUNCH;
        const int per = !fuse ? 1 : (ty || tx) ? PER_LAUNCH : total;            // fuse = 0: one sweep per launch, the timing baseline
        const float omega = (float)(2.0 / (1.0 + std::sin(M_PI / (double)side)));
        int cur = 0;
        for (int done = 0; done < total; done += per) {
            const int sweeps = total - done < per ? total - done : per;
            hipLaunchKernelGGL(k_diffuse_relax, grid, dim3(THREADS), 0, st, (const float*)lv[l].u[cur], lv[l].u[cur ^ 1],
                               done == 0 ? coarse : (const float*)nullptr, l + 1 < L ? lv[l + 1].W : 0, (const float*)lv[l].e,
                               (const uint8_t*)lv[l].fixed, h, w, ty, tx, leak, omega, sweeps);
            if (const int rc = be::check_launch("be_fill_diffuse_f32(relax)")) return rc;
            cur ^= 1;
        }
        coarse = result = lv[l].u[cur];
    }
    hipLaunchKernelGGL(k_diffuse_finish, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, depth, result, (const float*)lv[0].e,
                       (const uint8_t*)lv[0].fixed, H, W, leak, depth_out, reinterpret_cast<unsigned*>(residual));
    return be::check_launch("be_fill_diffuse_f32(finish)");
}
