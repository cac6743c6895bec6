// Forward, depth-dependent reprojection: the depth map of one pinhole camera, and maps that ride on it, seen from another
// (be_unproject_f32, be_reproject_f32).  A source sample lands where its own depth sends it, two samples may land
// on one target pixel and the nearer must win: a z-buffer of 64-bit keys (depth bits : source index) under an unsigned atomicMin.
// The minimum of a set does not depend on the order its members arrive in, so the outputs are a function of the inputs alone.
//
// All arithmetic is float32 with one rounding per written operation (no contraction): be_hip/camera.py restates it in numpy,
// operation by operation, and the tests hold the kernels to that statement bit for bit.
#include <cstdint>
#include "be_common.h"
#include "be_projection.h"   // Geom, Proj, project, taking_part, make_geom: shared with be_fuse.hip

#pragma clang fp contract(off)

namespace {

// one thread per source sample: xyz [3,Ns] in the target frame; 0 where the sample's depth is invalid
__global__ __launch_bounds__(256) void k_unproject(Geom g, const float* __restrict__ depth, float* __restrict__ xyz) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.Ns) return;
    const Proj p = project(g, i, depth[i]);
    xyz[i] = p.z_ok ? p.Xd : 0.0f;
    xyz[g.Ns + i] = p.z_ok ? p.Yd : 0.0f;
    xyz[2 * g.Ns + i] = p.z_ok ? p.Zd : 0.0f;
}

// one thread per source sample: a sample that takes part issues one no-return 64-bit unsigned minimum on its target pixel.
// near < Zd < inf (a huge finite Z may overflow Zd), and a positive float orders as its bit pattern: the nearest surface wins,
// the lowest source index on a tie.
__global__ __launch_bounds__(256) void k_splat_zbuf(Geom g, const float* __restrict__ depth, unsigned long long* __restrict__ zbuf) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.Ns) return;
    const Proj p = project(g, i, depth[i]);
    if (!taking_part(g, p)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(p.Zd) << 32) | (unsigned long long)(uint32_t)i;
    atomicMin(&zbuf[(int64_t)(int)p.fv * g.Wo + (int)p.fu], key);
}

// one thread per target pixel: the winner's depth (the key's high word), its source index, and C channels gathered from
// feat [C,Ns]; +0 / -1 where nothing landed.  Every output element is written exactly once.
__global__ __launch_bounds__(256) void k_resolve_zbuf(const unsigned long long* __restrict__ zbuf, int64_t No, int64_t Ns,
                                                      const float* __restrict__ feat, int C, float* __restrict__ depth_out,
                                                      int32_t* __restrict__ index, float* __restrict__ feat_out) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= No) return;
    const unsigned long long key = zbuf[o];
    const bool hit = key != ~0ull;
    const uint32_t src = (uint32_t)key;
    depth_out[o] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
    index[o] = hit ? (int32_t)src : -1;
    for (int c = 0; c < C; ++c) feat_out[(int64_t)c * No + o] = hit ? feat[(int64_t)c * Ns + src] : 0.0f;
}

}  // namespace

extern "C" int be_unproject_f32(const float* depth, int Hs, int Ws, int scale, int top, int left, const float* cam_src,
                                const float* pose, float* xyz, void* stream) {
    BE_REQUIRE(depth && xyz, "be_unproject_f32: null pointer");
    Geom g;
    if (const int rc = make_geom("be_unproject_f32", Hs, Ws, scale, top, left, cam_src, cam_src, pose, 0.0f, 1, 1, &g)) return rc;
    hipLaunchKernelGGL(k_unproject, dim3((unsigned)((g.Ns + 255) / 256)), dim3(256), 0, be::as_stream(stream), g, depth, xyz);
    return be::check_launch("be_unproject_f32");
}

extern "C" int be_reproject_f32(const float* depth, int Hs, int Ws, int scale, int top, int left, const float* cam_src,
                                const float* cam_dst, const float* pose, float near, int Ho, int Wo, const float* feat, int C,
                                uint64_t* zbuf, float* depth_out, int32_t* index, float* feat_out, void* stream) {
    BE_REQUIRE(depth && zbuf && depth_out && index, "be_reproject_f32: null pointer");
    BE_REQUIRE(C >= 0 && (C == 0 || (feat && feat_out)), "be_reproject_f32: C must be >= 0, and feat / feat_out given when C > 0");
    Geom g;
    if (const int rc = make_geom("be_reproject_f32", Hs, Ws, scale, top, left, cam_src, cam_dst, pose, near, Ho, Wo, &g)) return rc;
    const int64_t No = (int64_t)Ho * Wo;
    hipStream_t s = be::as_stream(stream);
    const hipError_t e = hipMemsetAsync(zbuf, 0xff, (size_t)No * sizeof(uint64_t), s);
    if (e != hipSuccess) return be::fail(BE_ELAUNCH, "be_reproject_f32: hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_splat_zbuf, dim3((unsigned)((g.Ns + 255) / 256)), dim3(256), 0, s, g, depth,
                       reinterpret_cast<unsigned long long*>(zbuf));
    if (const int rc = be::check_launch("be_reproject_f32(splat)")) return rc;
    hipLaunchKernelGGL(k_resolve_zbuf, dim3((unsigned)((No + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(zbuf), No, g.Ns, feat, C, depth_out, index, feat_out);
    return be::check_launch("be_reproject_f32(resolve)");
}
