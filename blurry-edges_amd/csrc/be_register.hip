// Depth registration: the pose between two views from their depth maps, by point-to-plane ICP.  Two entries:
// be_depth_normals_f32 - surface normals of a depth map from central differences of its unprojected samples - and
// be_icp_linearize_f32 - the linearised point-to-plane step at one pose, reduced to the 27 sums of a 6 x 6 normal system plus its
// residual, weight and count.  The host loop around them (solve, compose, repeat) is be_hip/registration.py, shared with the numpy
// statement of both kernels.
//
// Every sample is projected as be_reproject.hip projects it (be_projection.h).  All per-sample arithmetic is float32 with one
// rounding per written operation (no contraction; `/` and sqrtf are correctly rounded), so registration.normals_f32 and
// registration.linearize restate it bit for bit.  The sums are double, and their order is a function of the sample count alone:
//   grid     nblocks = min(ceil(Ns / 256), 64) workgroups of 256; thread t of T = 256 nblocks walks samples t, t + T, .. in
//            increasing order and adds each term to its own accumulator (+0.0 at the start; a sample that fails a gate adds nothing)
//   wave     across the 64 lanes: for off = 32, 16, 8, 4, 2, 1: v[l] += v[l + off]; lane 0 holds the wave's sum
//   group    (w0 + w1) + (w2 + w3) over the 4 waves, through LDS -> partial [nblocks,32]
//   k_icp_sum  one wave per term: lane l holds partial[l] (+0.0 for l >= nblocks), the wave fold again -> sums [32]
// No float or double atomics; no dependence on the device, the CU count or the stream.
//
// Resources (gfx950, hipcc -O3 -Rpass-analysis=kernel-resource-usage):
//   k_depth_normals   34 VGPRs, 8 waves / SIMD, no LDS, no scratch
//   k_icp_rows        108 VGPRs (30 double accumulators are 60 of them), 4 waves / SIMD - the grid is at most 64 workgroups of 4
//                     waves, one per SIMD of 64 CUs, so occupancy does not bind; 1 KiB LDS (4 x 32 doubles: lane k of the final
//                     read touches the two 4-byte banks 2k, 2k + 1 of 64 - conflict free); no scratch
//   k_icp_sum         15 VGPRs, 8 waves / SIMD, no LDS, no scratch
#include <cstdint>
#include "be_common.h"
#include "be_projection.h"   // Geom, Proj, project, taking_part, make_geom: shared with be_reproject.hip and be_fuse.hip

#pragma clang fp contract(off)

namespace {

constexpr int ICP_MAX_BLOCKS = 64;                  // one wave folds the partials
constexpr int ICP_TERMS = 30;                       // 21 + 6 + 3; a row of partial / sums holds 32 doubles, the last two zero

__device__ __forceinline__ bool good(float Z) { return Z > 0.0f && Z < __builtin_inff(); }     // NaN fails both

struct Vec3 { float x, y, z; };

__device__ __forceinline__ Vec3 point(const Geom& g, int64_t i, float Z) {
    const Proj p = project(g, i, Z);                // under the identity pose: k_unproject's arithmetic
    return Vec3{p.Xd, p.Yd, p.Zd};
}

// the difference of the unprojected samples along one axis of the lattice: `stride` apart in memory, `at` the pixel's coordinate on
// that axis and `n` the image's extent.  A neighbour counts when it is inside, good and within `jump` of the pixel's depth.
__device__ __forceinline__ bool axis_diff(const Geom& g, const float* __restrict__ depth, int64_t i, int64_t stride, int at, int n, int r,
                                          float Zc, const Vec3& Pc, float jump, Vec3* d) {
    bool hp = at + r < n, hm = at - r >= 0;
    const float Zp = hp ? depth[i + stride] : 0.0f, Zm = hm ? depth[i - stride] : 0.0f;
    hp = hp && good(Zp) && fabsf(Zp - Zc) <= jump;
    hm = hm && good(Zm) && fabsf(Zm - Zc) <= jump;
    if (!hp && !hm) return false;
    const Vec3 a = hp ? point(g, i + stride, Zp) : Pc;
    const Vec3 b = hm ? point(g, i - stride, Zm) : Pc;
    d->x = a.x - b.x;
    d->y = a.y - b.y;
    d->z = a.z - b.z;
    return true;
}

// one thread per pixel; every output element is written exactly once
__global__ __launch_bounds__(256) void k_depth_normals(Geom g, const float* __restrict__ depth, int H, int W, int r, float jump,
                                                       float* __restrict__ normal) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.Ns) return;
    const int iy = (int)(i / W), ix = (int)(i - (int64_t)iy * W);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    const float Zc = depth[i];
    if (good(Zc)) {
        const Vec3 Pc = point(g, i, Zc);
        Vec3 du, dv;
        if (axis_diff(g, depth, i, r, ix, W, r, Zc, Pc, jump, &du) && axis_diff(g, depth, i, (int64_t)r * W, iy, H, r, Zc, Pc, jump, &dv)) {
            float cx = du.y * dv.z - du.z * dv.y;
            float cy = du.z * dv.x - du.x * dv.z;
            float cz = du.x * dv.y - du.y * dv.x;
            const float l = sqrtf((cx * cx + cy * cy) + cz * cz);
            if (l > 0.0f && l < __builtin_inff()) {
                cx = cx / l;
                cy = cy / l;
                cz = cz / l;
                const float s = (cx * Pc.x + cy * Pc.y) + cz * Pc.z;
                if (s > 0.0f) {                     // towards the camera: n . P <= 0
                    cx = -cx;
                    cy = -cy;
                    cz = -cz;
                }
                nx = cx; ny = cy; nz = cz;
            }
        }
    }
    normal[i] = nx;
    normal[g.Ns + i] = ny;
    normal[2 * g.Ns + i] = nz;
}

struct IcpMaps {
    const float* depth_s;
    const float* weight_s;                          // may be null: 1
    const float* depth_d;
    const float* normal_d;                          // [3,Hd*Wd]
    const float* weight_d;                          // may be null: 1
    float max_dist2, huber;
};

// the row (J[0..5], r, w) of source sample i, or false when a gate fails
__device__ __forceinline__ bool icp_row(const Geom& g, const IcpMaps& m, int64_t i, float* row) {
    const Proj p = project(g, i, m.depth_s[i]);
    if (!taking_part(g, p)) return false;
    const int64_t Nd = (int64_t)g.Ho * g.Wo;
    const int64_t j = (int64_t)(int)p.fv * g.Wo + (int)p.fu;            // 0 <= fv < Ho, 0 <= fu < Wo: inside [0, Nd)
    const float Zq = m.depth_d[j];
    if (!good(Zq)) return false;
    const float nx = m.normal_d[j], ny = m.normal_d[Nd + j], nz = m.normal_d[2 * Nd + j];
    if (!(nx != 0.0f || ny != 0.0f || nz != 0.0f)) return false;
    const float Qx = ((p.fu - g.cxd) / g.fxd) * Zq;
    const float Qy = ((p.fv - g.cyd) / g.fyd) * Zq;
    const float Dx = p.Xd - Qx, Dy = p.Yd - Qy, Dz = p.Zd - Zq;
    const float dd = (Dx * Dx + Dy * Dy) + Dz * Dz;
    if (!(dd <= m.max_dist2)) return false;                             // NaN fails
    const float ws = m.weight_s ? m.weight_s[i] : 1.0f;
    const float wd = m.weight_d ? m.weight_d[j] : 1.0f;
    float w = ws * wd;
    if (!(w > 0.0f && w < __builtin_inff())) return false;              // NaN fails
    const float r = (nx * Dx + ny * Dy) + nz * Dz;
    if (m.huber > 0.0f) {
        const float a = fabsf(r);
        if (a > m.huber) w = w * (m.huber / a);
    }
    row[0] = p.Yd * nz - p.Zd * ny;                                     // P x n: the row of a left-multiplied twist (omega, v)
    row[1] = p.Zd * nx - p.Xd * nz;
    row[2] = p.Xd * ny - p.Yd * nx;
    row[3] = nx;
    row[4] = ny;
    row[5] = nz;
    row[6] = r;
    row[7] = w;
    return true;
}

__device__ __forceinline__ double wave_fold(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                                           // lane 0: the sum in the order of the header
}

__global__ __launch_bounds__(256) void k_icp_rows(Geom g, IcpMaps m, double* __restrict__ partial, float* __restrict__ rows_out) {
    __shared__ double s_wave[4][32];
    double acc[ICP_TERMS];
#pragma unroll
    for (int k = 0; k < ICP_TERMS; ++k) acc[k] = 0.0;
    const int64_t T = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.Ns; i += T) {
        float row[8];
        const bool ok = icp_row(g, m, i, row);
        if (rows_out) {
#pragma unroll
            for (int c = 0; c < 8; ++c) rows_out[(int64_t)c * g.Ns + i] = ok ? row[c] : 0.0f;
        }
        if (!ok) continue;
        double J[6], wJ[6];
        const double r = (double)row[6], w = (double)row[7];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            J[a] = (double)row[a];
            wJ[a] = w * J[a];
        }
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) acc[k++] += wJ[a] * J[b];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] += wJ[a] * r;
        acc[27] += (w * r) * r;
        acc[28] += w;
        acc[29] += 1.0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < ICP_TERMS; ++k) {
        const double v = wave_fold(acc[k]);
        if (lane == 0) s_wave[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        const int k = threadIdx.x;
        partial[(int64_t)blockIdx.x * 32 + k] = k < ICP_TERMS ? (s_wave[0][k] + s_wave[1][k]) + (s_wave[2][k] + s_wave[3][k]) : 0.0;
    }
}

// one workgroup of 4 waves; wave w folds terms w, w + 4, ..
__global__ __launch_bounds__(256) void k_icp_sum(const double* __restrict__ partial, int nblocks, double* __restrict__ sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = wave; k < 32; k += 4) {
        double v = (k < ICP_TERMS && lane < nblocks) ? partial[lane * 32 + k] : 0.0;
        v = wave_fold(v);
        if (lane == 0) sums[k] = v;
    }
}

inline int icp_blocks(int64_t Ns) {
    const int64_t nb = (Ns + 255) / 256;
    return (int)(nb < ICP_MAX_BLOCKS ? nb : ICP_MAX_BLOCKS);
}

const float kIdentity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};

}  // namespace

extern "C" int be_depth_normals_f32(const float* depth, int H, int W, int scale, int top, int left, const float* cam, int step,
                                    float max_jump, float* normal, void* stream) {
    BE_REQUIRE(depth && normal, "be_depth_normals_f32: null pointer");
    BE_REQUIRE(step >= 1 && step <= BE_NORMALS_MAX_STEP, "be_depth_normals_f32: step must be in [1, %d], got %d", BE_NORMALS_MAX_STEP, step);
    BE_REQUIRE(max_jump >= 0.0f && max_jump < __builtin_inff(), "be_depth_normals_f32: max_jump must be a finite number >= 0");
    Geom g;
    if (const int rc = make_geom("be_depth_normals_f32", H, W, scale, top, left, cam, cam, kIdentity, 0.0f, H, W, &g)) return rc;
    hipLaunchKernelGGL(k_depth_normals, dim3((unsigned)((g.Ns + 255) / 256)), dim3(256), 0, be::as_stream(stream), g, depth, H, W, step,
                       max_jump * (float)step, normal);
    return be::check_launch("be_depth_normals_f32");
}

extern "C" int64_t be_icp_scratch_bytes(int Hs, int Ws) {
    if (Hs < 1 || Ws < 1 || (int64_t)Hs * Ws > SAMPLES_MAX) return -1;
    return (int64_t)icp_blocks((int64_t)Hs * Ws) * 32 * (int64_t)sizeof(double);
}

extern "C" int be_icp_linearize_f32(const float* depth_s, const float* weight_s, int Hs, int Ws, int scale, int top, int left,
                                    const float* cam_src, const float* depth_d, const float* normal_d, const float* weight_d, int Hd, int Wd,
                                    const float* cam_dst, const float* pose, float near, float max_dist, float huber, void* scratch,
                                    double* sums, float* rows_out, void* stream) {
    BE_REQUIRE(depth_s && depth_d && normal_d && scratch && sums, "be_icp_linearize_f32: null pointer");
    BE_REQUIRE(max_dist >= 0.0f && max_dist < __builtin_inff(), "be_icp_linearize_f32: max_dist must be a finite number >= 0");
    BE_REQUIRE(huber >= 0.0f && huber < __builtin_inff(), "be_icp_linearize_f32: huber must be a finite number >= 0");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7u) == 0,
               "be_icp_linearize_f32: scratch and sums must be 8-byte aligned");
    Geom g;
    if (const int rc = make_geom("be_icp_linearize_f32", Hs, Ws, scale, top, left, cam_src, cam_dst, pose, near, Hd, Wd, &g)) return rc;
    const IcpMaps m{depth_s, weight_s, depth_d, normal_d, weight_d, max_dist * max_dist, huber};
    const int nblocks = icp_blocks(g.Ns);
    hipStream_t st = be::as_stream(stream);
    double* partial = static_cast<double*>(scratch);
    hipLaunchKernelGGL(k_icp_rows, dim3((unsigned)nblocks), dim3(256), 0, st, g, m, partial, rows_out);
    if (const int rc = be::check_launch("be_icp_linearize_f32(rows)")) return rc;
    hipLaunchKernelGGL(k_icp_sum, dim3(1), dim3(256), 0, st, partial, nblocks, sums);
    return be::check_launch("be_icp_linearize_f32(sum)");
}
