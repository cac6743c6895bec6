// Dense depth from sparse samples by nearest-sample flood fill (be_fill_nearest_f32).  The pipeline's depth_map holds
// depth in a band on both sides of every boundary and 0 elsewhere; a hole's nearest sample lies on the hole's own side of the nearest
// boundary, so every hole takes the depth of its nearest sample.  Nearest-sample assignment is the jump-flooding algorithm: passes
// over double-buffered int32 seed maps, integer arithmetic only, each pixel taking the minimum of the key (squared distance,
// seed index) over nine candidates - a minimum over a total order, so the outputs are a function of the inputs alone.
//
// The only float arithmetic, the robust local mean around a seed, is float32 with one rounding per written operation (no
// contraction): be_hip/fill.py restates all of it in numpy, operation by operation, and the tests hold the kernels to that statement
// bit for bit.
#include <cstdint>
#include "be_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int FILL_MAX_SIDE = 16384;               // d2 < 2^29 and a linear index < 2^28: everything fits int32
constexpr int FILL_MAX_R = 8;
constexpr int TILE = 32;                           // the fused tail: a 32 x 32 tile per 256-thread workgroup
constexpr int HALO_MAX = 15;                       // 8 + 4 + 2 + 1
constexpr int SIDE_MAX = TILE + 2 * HALO_MAX;      // 62: two int32 images of 62 x 62 = 30 752 B of LDS

__device__ __forceinline__ bool is_seed(const float* __restrict__ depth, const float* __restrict__ weight, int p) {
    const float z = depth[p];
    const float w = weight ? weight[p] : 1.0f;
    return w > 0.0f && z > 0.0f && z < __builtin_inff();         // NaN fails all three
}

// one thread per pixel: the first seed map (the pixel's own index at a seed, -1 elsewhere) and, for r > 0, the robust local mean
// of every seed: num / den over the valid samples q of the (2r+1)^2 window clipped to the image, in row-major order
__global__ __launch_bounds__(256) void k_fill_seeds(const float* __restrict__ depth, const float* __restrict__ weight, int H, int W, int r,
                                                    float inv, int32_t* __restrict__ seeds, float* __restrict__ mean) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const bool seed = is_seed(depth, weight, p);
    seeds[p] = seed ? p : -1;
    if (r == 0) return;
    float m = 0.0f;
    if (seed) {
        const int sy = p / W, sx = p - sy * W;
        const float zs = depth[p];
        const int y0 = max(sy - r, 0), y1 = min(sy + r, H - 1), x0 = max(sx - r, 0), x1 = min(sx + r, W - 1);
        float num = 0.0f, den = 0.0f;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) {
                const int q = y * W + x;
                if (!is_seed(depth, weight, q)) continue;
                const float zq = depth[q];
                const float wq = weight ? weight[q] : 1.0f;
                const float d = zq - zs;
                const float k = wq / (1.0f + (d * d) * inv);
                num = num + k * zq;
                den = den + k;
            }
        m = num / den;                                             // den > 0: q = s contributes w_s
    }
    mean[p] = m;
}

// the three outputs of pixel p whose seed is c (-1: the image holds no seed at all)
struct FillOut {
    const float* depth;
    const float* mean;                                             // null when r == 0: a hole takes its seed's depth exactly
    float* depth_out;
    int32_t* index;
    int32_t* dist2;
};

__device__ __forceinline__ void emit(const FillOut& o, int p, int c, int d2) {
    o.index[p] = c;
    o.dist2[p] = c < 0 ? -1 : d2;
    o.depth_out[p] = c < 0 ? 0.0f : c == p ? o.depth[p] : o.mean ? o.mean[c] : o.depth[c];
}

// one pass with step s, one thread per pixel: of the nine positions p + (dy, dx) s inside the image that hold a seed, the
// candidate with the smallest key (d2(p, c), c).  LAST: the pass writes the outputs instead of the next seed map.
template <bool LAST>
__global__ __launch_bounds__(256) void k_fill_pass(const int32_t* __restrict__ src, int H, int W, int s, int32_t* __restrict__ dst,
                                                   FillOut o) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    // the nine loads are issued together, from addresses clamped into the image; a position outside it counts as -1
    int cand[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + (k / 3 - 1) * s, xx = x + (k % 3 - 1) * s;
        const int v = src[min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)];
        cand[k] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? v : -1;
    }
    int bc = -1, bd = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int c = cand[k];
        const int cy = max(c, 0) / W, cx = max(c, 0) - cy * W;
        const int d2 = (y - cy) * (y - cy) + (x - cx) * (x - cx);
        if (c >= 0 && (d2 < bd || (d2 == bd && c < bc))) { bd = d2; bc = c; }
    }
    if (LAST) emit(o, p, bc, bd);
    else dst[p] = bc;
}

// The passes with steps first, first / 2, .., 1 (first <= 8) in one launch: after them a pixel depends only on the seed map within
// halo = 2 first - 1 <= 15 of it (Chebyshev).  A workgroup loads its 32 x 32 tile plus that halo into LDS (-1 outside the image),
// runs the passes there - the region that is still exact shrinks by s per pass, and a position outside the image stays -1, as the
// per-pass kernel never reads one - and writes the outputs of its tile.  In LDS a seed is held as cy << 16 | cx: no division in
// the passes, and the order of the packed words is the order of the linear indices, so ties break the same way.
__global__ __launch_bounds__(256) void k_fill_tail(const int32_t* __restrict__ src, int H, int W, int first, FillOut o) {
    __shared__ int32_t buf[2][SIDE_MAX * SIDE_MAX];
    const int halo = 2 * first - 1;
    const int n = TILE + 2 * halo;                                 // the side of the region held; rows of buf are n long
    const int oy = (int)blockIdx.y * TILE - halo, ox = (int)blockIdx.x * TILE - halo;
    for (int i = threadIdx.x; i < n * n; i += 256) {
        const int ry = i / n, rx = i - ry * n;
        const int gy = oy + ry, gx = ox + rx;
        int v = -1;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int c = src[gy * W + gx];
            if (c >= 0) {
                const int cy = c / W;
                v = (cy << 16) | (c - cy * W);
            }
        }
        buf[0][i] = v;
    }
    __syncthreads();
    int cur = 0, m = 0;
    for (int s = first; s >= 1; s >>= 1) {
        m += s;                                                    // positions [m, n - m)^2 are exact after this pass
        const int side = n - 2 * m;
        for (int i = threadIdx.x; i < side * side; i += 256) {
            const int ry = m + i / side, rx = m + i % side;
            const int gy = oy + ry, gx = ox + rx;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            int cand[9];                                           // the nine reads are issued together
#pragma unroll
            for (int k = 0; k < 9; ++k) cand[k] = buf[cur][(ry + (k / 3 - 1) * s) * n + (rx + (k % 3 - 1) * s)];
            int bc = -1, bd = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int c = cand[k];
                const int ey = gy - (max(c, 0) >> 16), ex = gx - (max(c, 0) & 0xffff);
                const int d2 = ey * ey + ex * ex;
                if (in && c >= 0 && (d2 < bd || (d2 == bd && c < bc))) { bd = d2; bc = c; }
            }
            if (s > 1) buf[cur ^ 1][ry * n + rx] = bc;
            else if (in) emit(o, gy * W + gx, bc < 0 ? -1 : (bc >> 16) * W + (bc & 0xffff), bd);      // side == TILE: the tile itself
        }
        __syncthreads();
        cur ^= 1;
    }
}

}  // namespace

extern "C" int be_fill_nearest_f32(const float* depth, const float* weight, int H, int W, int smooth_r, float sigma_z, int fuse,
                                   int32_t* scratch, float* depth_out, int32_t* index, int32_t* dist2, void* stream) {
    BE_REQUIRE(depth && scratch && depth_out && index && dist2, "be_fill_nearest_f32: null pointer");
    BE_REQUIRE(H >= 1 && W >= 1 && H <= FILL_MAX_SIDE && W <= FILL_MAX_SIDE, "be_fill_nearest_f32: H and W must be in [1, %d], got %d x %d",
               FILL_MAX_SIDE, H, W);
    BE_REQUIRE(smooth_r >= 0 && smooth_r <= FILL_MAX_R, "be_fill_nearest_f32: smooth_r must be in [0, %d], got %d", FILL_MAX_R, smooth_r);
    BE_REQUIRE(sigma_z > 0.0f && sigma_z < __builtin_inff(), "be_fill_nearest_f32: sigma_z must be a finite number > 0");
    BE_REQUIRE(fuse == 0 || fuse == 1, "be_fill_nearest_f32: fuse must be 0 or 1, got %d", fuse);
    hipStream_t st = be::as_stream(stream);
    const int N = H * W;
    const unsigned blocks = (unsigned)((N + 255) / 256);
    int32_t* map[2] = {scratch, scratch + N};
    float* mean = smooth_r > 0 ? reinterpret_cast<float*>(scratch + 2 * (int64_t)N) : nullptr;
    const float inv = 1.0f / (sigma_z * sigma_z);
    const FillOut o{depth, mean, depth_out, index, dist2};
    hipLaunchKernelGGL(k_fill_seeds, dim3(blocks), dim3(256), 0, st, depth, weight, H, W, smooth_r, inv, map[0], mean);
    if (const int rc = be::check_launch("be_fill_nearest_f32(seeds)")) return rc;
    // the schedule 1, 2^(L-1), .., 2, 1 with L = ceil(log2(max(H, W))); with fuse the final run of steps <= 8 is one launch
    int L = 0;
    while ((1 << L) < (H > W ? H : W)) ++L;
    int cur = 0;
    for (int i = -1; i < L; ++i) {
        const int s = i < 0 ? 1 : 1 << (L - 1 - i);
        const bool last = i == L - 1;
        if (fuse && i >= 0 && s <= 8) {
            hipLaunchKernelGGL(k_fill_tail, dim3((unsigned)((W + TILE - 1) / TILE), (unsigned)((H + TILE - 1) / TILE)), dim3(256), 0, st,
                               map[cur], H, W, s, o);
            return be::check_launch("be_fill_nearest_f32(tail)");
        }
        if (last) hipLaunchKernelGGL(k_fill_pass<true>, dim3(blocks), dim3(256), 0, st, map[cur], H, W, s, (int32_t*)nullptr, o);
        else hipLaunchKernelGGL(k_fill_pass<false>, dim3(blocks), dim3(256), 0, st, map[cur], H, W, s, map[cur ^ 1], o);
        if (const int rc = be::check_launch("be_fill_nearest_f32(pass)")) return rc;
        cur ^= 1;
    }
    return BE_OK;
}
