// Truncated signed distance volumes: posed depth views integrated one at a time into a regular voxel grid, and any pinhole camera
// ray-cast out of it (be_tsdf_integrate_f32, be_tsdf_mean_f32, be_tsdf_raycast_f32).  Where be_fuse.hip merges V
// views in one target camera and starts over for every new viewpoint, a volume takes one more view without the others and renders
// any viewpoint from the same sums.
//
// Nothing is accumulated in floating point: a voxel's sums are integers of fixed-point terms (weights in units of 2^-8, signed
// distances in units of trunc * 2^-15, channels in units of 2^-16) and every voxel is owned by one thread, so there are no atomics
// and the sums depend neither on the order of the views nor on how they are grouped into calls.  be_hip/volume.py restates the
// three kernels in numpy and the tests hold them to it bit for bit.  The sums are exact below 2^19 views (wq <= 2^12 in an int32).
//
// All float arithmetic is float32 with one rounding per written operation (no contraction); the means are formed in double from
// the integer sums and rounded to float once.
#include <cstdint>
#include "be_common.h"
#include "be_tsdf_vol.h"     // Vol, make_vol: the volume by value, shared with be_tsdf_mesh.hip
#include "be_projection.h"   // Geom, make_geom: the camera, pose and lattice constants, shared with be_reproject.hip and be_fuse.hip

#pragma clang fp contract(off)

namespace {

using be::Vol;
using be::make_vol;

// One thread per voxel, one launch per view.  g: the view's camera in (fyd, fxd, cyd, cxd), the INVERSE pose (volume frame -> view
// frame) in (r, t), the view's lattice in (top, left, k, Ws) and its sample count in (Ho, Wo).  A voxel that does not take part
// neither reads nor writes its sums.
__global__ __launch_bounds__(256) void k_tsdf_integrate(Geom g, Vol vol, const float* __restrict__ depth, const float* __restrict__ weight,
                                                        const float* __restrict__ feat, int C, int32_t* __restrict__ sw,
                                                        long long* __restrict__ swd, long long* __restrict__ swf) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= vol.n) return;
    const int ix = (int)(i % vol.nx);
    const int64_t r = i / vol.nx;
    const int iy = (int)(r % vol.ny), iz = (int)(r / vol.ny);
    const float x = vol.x0 + (float)ix * vol.sx;
    const float y = vol.y0 + (float)iy * vol.sy;
    const float z = vol.z0 + (float)iz * vol.sz;
    const float X = ((g.r[0] * x + g.r[1] * y) + g.r[2] * z) + g.t[0];
    const float Y = ((g.r[3] * x + g.r[4] * y) + g.r[5] * z) + g.t[1];
    const float Z = ((g.r[6] * x + g.r[7] * y) + g.r[8] * z) + g.t[2];
    if (!(Z > g.near)) return;                                          // NaN fails
    const float u = (g.fxd * X) / Z + g.cxd;
    const float v = (g.fyd * Y) / Z + g.cyd;
    const float su = floorf((u - (float)g.left) * (float)g.k + 0.5f);
    const float sv = floorf((v - (float)g.top) * (float)g.k + 0.5f);
    if (!(su >= 0.0f && su < (float)g.Wo && sv >= 0.0f && sv < (float)g.Ho)) return;   // in float, before any conversion
    const int64_t j = (int64_t)(int)sv * g.Wo + (int)su;               // inside [0, Hs * Ws)
    const float Zq = depth[j];
    if (!(Zq > 0.0f && Zq < __builtin_inff())) return;
    const float w = weight ? weight[j] : 1.0f;
    if (!(w > 0.0f)) return;
    const float sdf = Zq - Z;
    if (!(sdf >= -vol.trunc)) return;
    const float wqf = floorf(fminf(w, 16.0f) * 256.0f + 0.5f);
    if (wqf == 0.0f) return;
    const long long wq = (long long)wqf;                                // at most 2^12
    const long long dq = (long long)floorf(fminf(sdf, vol.trunc) / vol.trunc * 32768.0f + 0.5f);
    sw[i] += (int32_t)wq;
    swd[i] += wq * dq;
    for (int c = 0; c < C; ++c) {
        const float f = feat[(int64_t)c * g.Ns + j];
        const float fc = f != f ? 0.0f : fminf(fmaxf(f, -2048.0f), 2048.0f);
        swf[(int64_t)c * vol.n + i] += wq * (long long)floorf(fc * 65536.0f + 0.5f);
    }
}

// one thread per voxel: the means of the integer sums, +0 where the voxel holds nothing
__global__ __launch_bounds__(256) void k_tsdf_mean(int64_t n, int C, const int32_t* __restrict__ sw, const long long* __restrict__ swd,
                                                   const long long* __restrict__ swf, float* __restrict__ D, float* __restrict__ W,
                                                   float* __restrict__ Fm) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t s = sw[i];
    const double ds = (double)s;
    D[i] = s != 0 ? (float)((double)swd[i] / ds * 0x1p-15) : 0.0f;
    W[i] = (float)(ds * 0x1p-8);
    for (int c = 0; c < C; ++c) {
        const int64_t k = (int64_t)c * n + i;
        Fm[k] = s != 0 ? (float)((double)swf[k] / ds * 0x1p-16) : 0.0f;
    }
}

// the grid position of the camera point (xn z, yn z, z): the linear index of corner (0, 0, 0) and the three fractions
struct Cell { bool ok; int64_t j; float fx, fy, fz; };

__device__ __forceinline__ Cell locate(const Geom& g, const Vol& vol, float xn, float yn, float z) {
    Cell c;
    const float X = xn * z;
    const float Y = yn * z;
    const float Px = ((g.r[0] * X + g.r[1] * Y) + g.r[2] * z) + g.t[0];
    const float Py = ((g.r[3] * X + g.r[4] * Y) + g.r[5] * z) + g.t[1];
    const float Pz = ((g.r[6] * X + g.r[7] * Y) + g.r[8] * z) + g.t[2];
    const float gx = (Px - vol.x0) / vol.sx;
    const float gy = (Py - vol.y0) / vol.sy;
    const float gz = (Pz - vol.z0) / vol.sz;
    const float ix = floorf(gx), iy = floorf(gy), iz = floorf(gz);
    // in float, before any conversion: NaN and the infinities fail
    c.ok = ix >= 0.0f && ix <= (float)(vol.nx - 2) && iy >= 0.0f && iy <= (float)(vol.ny - 2) && iz >= 0.0f && iz <= (float)(vol.nz - 2);
    c.j = c.ok ? ((int64_t)(int)iz * vol.ny + (int)iy) * vol.nx + (int)ix : 0;
    c.fx = gx - ix;
    c.fy = gy - iy;
    c.fz = gz - iz;
    return c;
}

// a + t (b - a) along x, then y, then z over the 8 corners of a cell that is ok (every index inside the volume)
__device__ __forceinline__ float trilinear(const float* __restrict__ a, const Vol& vol, const Cell& c) {
    const int64_t dy = vol.nx, dz = (int64_t)vol.nx * vol.ny;
    const float* p = a + c.j;
    const float a000 = p[0], a001 = p[1], a010 = p[dy], a011 = p[dy + 1];
    const float a100 = p[dz], a101 = p[dz + 1], a110 = p[dz + dy], a111 = p[dz + dy + 1];
    const float c00 = a000 + c.fx * (a001 - a000);
    const float c01 = a010 + c.fx * (a011 - a010);
    const float c10 = a100 + c.fx * (a101 - a100);
    const float c11 = a110 + c.fx * (a111 - a110);
    const float c0 = c00 + c.fy * (c01 - c00);
    const float c1 = c10 + c.fy * (c11 - c10);
    return c0 + c.fz * (c1 - c0);
}

__device__ __forceinline__ bool observed(const float* __restrict__ W, const Vol& vol, const Cell& c) {
    const int64_t dy = vol.nx, dz = (int64_t)vol.nx * vol.ny;
    const float* p = W + c.j;
    return p[0] > 0.0f && p[1] > 0.0f && p[dy] > 0.0f && p[dy + 1] > 0.0f && p[dz] > 0.0f && p[dz + 1] > 0.0f && p[dz + dy] > 0.0f &&
           p[dz + dy + 1] > 0.0f;
}

// One thread per target pixel.  g: the target camera in (fy, fx, cy, cx), the pose (camera frame -> volume frame) in (r, t), the
// target size in (Ho, Wo).  A sample outside the volume gathers nothing; the 8 corner weights are tested before D is read; the
// loop exits at the hit, where the previous sample's position is formed again from (i - 1) - the same operations, the same bits.
__global__ __launch_bounds__(256) void k_tsdf_raycast(Geom g, Vol vol, const float* __restrict__ D, const float* __restrict__ W,
                                                      const float* __restrict__ Fm, int C, float z_near, float step, int n,
                                                      float* __restrict__ depth, float* __restrict__ weight, float* __restrict__ feat) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t No = (int64_t)g.Ho * g.Wo;
    if (o >= No) return;
    const int v = (int)(o / g.Wo), u = (int)(o - (int64_t)v * g.Wo);
    const float xn = ((float)u - g.cx) / g.fx;
    const float yn = ((float)v - g.cy) / g.fy;
    bool prev_ok = false;
    float F_prev = 0.0f, z_prev = z_near;
    float d_out = 0.0f, w_out = 0.0f;
    int hit = -1;
    float a = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float z = z_near + (float)i * step;
        const Cell c = locate(g, vol, xn, yn, z);
        const bool ok = c.ok && observed(W, vol, c);
        float F = 0.0f;
        if (ok) {
            F = trilinear(D, vol, c);
            if (prev_ok && F_prev > 0.0f && F <= 0.0f) {
                a = F_prev / (F_prev - F);
                d_out = z_prev + (z - z_prev) * a;
                hit = i;
                break;
            }
        }
        prev_ok = ok;
        F_prev = F;
        z_prev = z;
    }
    Cell c0, c1;
    if (hit >= 0) {
        c0 = locate(g, vol, xn, yn, z_near + (float)(hit - 1) * step);
        c1 = locate(g, vol, xn, yn, z_near + (float)hit * step);
        const float w0 = trilinear(W, vol, c0), w1 = trilinear(W, vol, c1);
        w_out = w0 + a * (w1 - w0);
    }
    depth[o] = d_out;
    weight[o] = w_out;
    for (int c = 0; c < C; ++c) {
        float f = 0.0f;
        if (hit >= 0) {
            const float* Fc = Fm + (int64_t)c * vol.n;
            const float f0 = trilinear(Fc, vol, c0), f1 = trilinear(Fc, vol, c1);
            f = f0 + a * (f1 - f0);
        }
        feat[(int64_t)c * No + o] = f;
    }
}

}  // namespace

extern "C" int be_tsdf_integrate_f32(const float* depth, const float* weight, const float* feat, int C, int Hs, int Ws, int scale, int top,
                                     int left, const float* cam_src, const float* pose, float near, const int* dims, const float* origin,
                                     const float* voxel, float trunc, int32_t* sw, int64_t* swd, int64_t* swf, void* stream) {
    BE_REQUIRE(depth && cam_src && pose && sw && swd, "be_tsdf_integrate_f32: null pointer");
    BE_REQUIRE(C >= 0 && C <= BE_FUSE_MAX_CHANNELS && (C == 0 || (feat && swf)),
               "be_tsdf_integrate_f32: C must be in [0, %d], and feat / swf given when C > 0", BE_FUSE_MAX_CHANNELS);
    Vol vol;
    if (const int rc = make_vol("be_tsdf_integrate_f32", dims, origin, voxel, trunc, &vol)) return rc;
    for (int i = 0; i < 12; ++i) BE_REQUIRE(pose[i] == pose[i], "be_tsdf_integrate_f32: pose must be finite");
    // the inverse pose, R^T and -R^T t, in double from the float32 numbers, each sum left to right, rounded to float once
    float q[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) q[3 * i + j] = pose[3 * j + i];
        q[9 + i] = (float)-(((double)pose[i] * (double)pose[9] + (double)pose[3 + i] * (double)pose[10]) + (double)pose[6 + i] * (double)pose[11]);
    }
    Geom g;
    if (const int rc = make_geom("be_tsdf_integrate_f32", Hs, Ws, scale, top, left, cam_src, cam_src, q, near, Hs, Ws, &g)) return rc;
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)((vol.n + 255) / 256)), dim3(256), 0, be::as_stream(stream), g, vol, depth, weight,
                       C > 0 ? feat : nullptr, C, sw, reinterpret_cast<long long*>(swd), reinterpret_cast<long long*>(swf));
    return be::check_launch("be_tsdf_integrate_f32");
}

extern "C" int be_tsdf_mean_f32(const int* dims, int C, const int32_t* sw, const int64_t* swd, const int64_t* swf, float* D, float* W,
                                float* Fm, void* stream) {
    BE_REQUIRE(sw && swd && D && W, "be_tsdf_mean_f32: null pointer");
    BE_REQUIRE(C >= 0 && C <= BE_FUSE_MAX_CHANNELS && (C == 0 || (swf && Fm)),
               "be_tsdf_mean_f32: C must be in [0, %d], and swf / Fm given when C > 0", BE_FUSE_MAX_CHANNELS);
    const float zero[3] = {0.0f, 0.0f, 0.0f}, one[3] = {1.0f, 1.0f, 1.0f};
    Vol vol;
    if (const int rc = make_vol("be_tsdf_mean_f32", dims, zero, one, 1.0f, &vol)) return rc;
    hipLaunchKernelGGL(k_tsdf_mean, dim3((unsigned)((vol.n + 255) / 256)), dim3(256), 0, be::as_stream(stream), vol.n, C, sw,
                       reinterpret_cast<const long long*>(swd), reinterpret_cast<const long long*>(swf), D, W, Fm);
    return be::check_launch("be_tsdf_mean_f32");
}

extern "C" int be_tsdf_raycast_f32(const float* D, const float* W, const float* Fm, int C, const int* dims, const float* origin,
                                   const float* voxel, const float* cam_dst, const float* pose, int Ho, int Wo, float z_near, float step,
                                   int n, float* depth_out, float* weight_out, float* feat_out, void* stream) {
    BE_REQUIRE(D && W && cam_dst && pose && depth_out && weight_out, "be_tsdf_raycast_f32: null pointer");
    BE_REQUIRE(C >= 0 && C <= BE_FUSE_MAX_CHANNELS && (C == 0 || (Fm && feat_out)),
               "be_tsdf_raycast_f32: C must be in [0, %d], and Fm / feat_out given when C > 0", BE_FUSE_MAX_CHANNELS);
    Vol vol;
    if (const int rc = make_vol("be_tsdf_raycast_f32", dims, origin, voxel, 1.0f, &vol)) return rc;
    BE_REQUIRE(z_near > 0.0f && z_near < __builtin_inff(), "be_tsdf_raycast_f32: z_near must be a finite number > 0");
    BE_REQUIRE(step > 0.0f && step < __builtin_inff(), "be_tsdf_raycast_f32: step must be a finite number > 0");
    BE_REQUIRE(n >= 1 && n <= BE_TSDF_MAX_STEPS, "be_tsdf_raycast_f32: n must be in [1, %d], got %d", BE_TSDF_MAX_STEPS, n);
    Geom g;
    if (const int rc = make_geom("be_tsdf_raycast_f32", Ho, Wo, 1, 0, 0, cam_dst, cam_dst, pose, 0.0f, Ho, Wo, &g)) return rc;
    hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned)(((int64_t)Ho * Wo + 255) / 256)), dim3(256), 0, be::as_stream(stream), g, vol, D, W,
                       C > 0 ? Fm : nullptr, C, z_near, step, n, depth_out, weight_out, feat_out);
    return be::check_launch("be_tsdf_raycast_f32");
}
