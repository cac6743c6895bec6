// A z-buffered triangle rasteriser: an indexed triangle mesh, with the maps that ride on its vertices, seen by a pinhole camera
// (be_mesh_raster_f32).  Vertices are projected in float32 and snapped to a 1/256 pixel lattice; coverage is decided
// on those integers alone, exactly, with the top-left rule; depth is interpolated perspective-correctly and the nearest fragment
// wins under an unsigned atomicMin of 64-bit keys (depth bits : face index), as in be_reproject.hip: the minimum of a set does not
// depend on the order its members arrive in, so the outputs are a function of the inputs alone.
//
// All float arithmetic is float32 with one rounding per written operation (no contraction): be_hip/raster.py restates it in numpy,
// operation by operation, and the tests hold the kernels to that statement bit for bit.
#include <cstdint>
#include "be_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SUB_BITS = 8;                                              // BE_RASTER_SUB = 1 << 8 sub-pixel positions per pixel
constexpr float GUARD = (float)BE_RASTER_GUARD;

// kernel arguments by value: the camera, the pose (row-major R, then t: mesh frame -> camera frame) and the target frame
struct View {
    float fy, fx, cy, cx;
    float r[9], t[3];
    float near;
    int Ho, Wo, cull;
};

// one thread per vertex: the record (xs, ys, bits of q = 1 / Zc, usable) the two other kernels read with one 16-byte load
__global__ __launch_bounds__(256) void k_raster_vertices(View g, const float* __restrict__ vertices, int64_t V, int4* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const float X = vertices[3 * i], Y = vertices[3 * i + 1], Z = vertices[3 * i + 2];
    const float Xc = ((g.r[0] * X + g.r[1] * Y) + g.r[2] * Z) + g.t[0];
    const float Yc = ((g.r[3] * X + g.r[4] * Y) + g.r[5] * Z) + g.t[1];
    const float Zc = ((g.r[6] * X + g.r[7] * Y) + g.r[8] * Z) + g.t[2];
    const float u = (g.fx * Xc) / Zc + g.cx;
    const float v = (g.fy * Yc) / Zc + g.cy;
    const float xs = floorf(u * (float)BE_RASTER_SUB + 0.5f);
    const float ys = floorf(v * (float)BE_RASTER_SUB + 0.5f);
    const float q = 1.0f / Zc;
    // tested in float, before any conversion to int: NaN and the infinities fail
    const bool usable = Zc > g.near && Zc < __builtin_inff() && fabsf(xs) <= GUARD && fabsf(ys) <= GUARD;
    rec[i] = make_int4(usable ? (int)xs : 0, usable ? (int)ys : 0, (int)__float_as_uint(q), usable ? 1 : 0);
}

// a triangle after the integer setup: its vertices in the positive orientation (1 and 2 exchanged when A was negative)
struct Tri {
    int32_t i[3];
    int64_t x[3], y[3], A;
    float q[3];
    bool ok, swapped;
};

// a face whose index leaves [0, V) is dropped here: the statement refuses it, a kernel cannot without a read-back
__device__ __forceinline__ Tri tri_setup(const int4* __restrict__ rec, const int32_t* __restrict__ faces, int64_t V, int64_t f, int cull) {
    Tri t;
    t.ok = false;
    t.swapped = false;
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return t;
    const int4 a = rec[i0], b = rec[i1], c = rec[i2];
    if (!(a.w && b.w && c.w)) return t;
    const int64_t A = (int64_t)(b.x - a.x) * (c.y - a.y) - (int64_t)(b.y - a.y) * (c.x - a.x);
    if (A == 0 || (cull == 1 && A > 0) || (cull == 2 && A < 0)) return t;
    t.ok = true;
    t.swapped = A < 0;
    const int4 p = t.swapped ? c : b, s = t.swapped ? b : c;
    t.i[0] = i0; t.i[1] = t.swapped ? i2 : i1; t.i[2] = t.swapped ? i1 : i2;
    t.x[0] = a.x; t.x[1] = p.x; t.x[2] = s.x;
    t.y[0] = a.y; t.y[1] = p.y; t.y[2] = s.y;
    t.q[0] = __uint_as_float((uint32_t)a.z); t.q[1] = __uint_as_float((uint32_t)p.z); t.q[2] = __uint_as_float((uint32_t)s.z);
    t.A = t.swapped ? -A : A;
    return t;
}

// edge e runs from vertex e + 1 to vertex e + 2 (mod 3), opposite vertex e
__device__ __forceinline__ void edge_of(const Tri& t, int e, int64_t& dx, int64_t& dy, int64_t& xa, int64_t& ya) {
    const int a = e == 2 ? 0 : e + 1, b = e == 0 ? 2 : e - 1;
    dx = t.x[b] - t.x[a];
    dy = t.y[b] - t.y[a];
    xa = t.x[a];
    ya = t.y[a];
}

__device__ __forceinline__ int64_t lo64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t hi64(int64_t a, int64_t b) { return a > b ? a : b; }

__device__ __forceinline__ bool top_left(int64_t dx, int64_t dy) { return dy < 0 || (dy == 0 && dx > 0); }

// 1 / z at a pixel from its three edge functions: w_i = (float) E_i / (float) A, iz = (w0 q0 + w1 q1) + w2 q2
__device__ __forceinline__ float depth_at(const Tri& t, float fA, const int64_t E[3], float w[3]) {
    w[0] = (float)E[0] / fA;
    w[1] = (float)E[1] / fA;
    w[2] = (float)E[2] / fA;
    const float iz = (w[0] * t.q[0] + w[1] * t.q[1]) + w[2] * t.q[2];
    return 1.0f / iz;
}

// one wave per triangle, four per workgroup.  The wave does the integer setup once, on values the compiler can keep in scalar
// registers, and walks the clipped bounding box in 8 x 8 pixel blocks, one lane per pixel; a block wholly outside one edge is
// skipped by a test of the edge function's largest corner value.  Each fragment issues one no-return 64-bit unsigned minimum.
__global__ __launch_bounds__(256) void k_raster_faces(const int4* __restrict__ rec, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                      int cull, int Ho, int Wo, unsigned long long* __restrict__ zbuf) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t f = (int64_t)blockIdx.x * 4 + wave;
    if (f >= T) return;
    const Tri t = tri_setup(rec, faces, V, f, cull);
    if (!t.ok) return;
    const int minx = (int)lo64(t.x[0], lo64(t.x[1], t.x[2])), maxx = (int)hi64(t.x[0], hi64(t.x[1], t.x[2]));
    const int miny = (int)lo64(t.y[0], lo64(t.y[1], t.y[2])), maxy = (int)hi64(t.y[0], hi64(t.y[1], t.y[2]));
    const int xlo = max((minx + BE_RASTER_SUB - 1) >> SUB_BITS, 0), xhi = min(maxx >> SUB_BITS, Wo - 1);   // >> of a negative: floor
    const int ylo = max((miny + BE_RASTER_SUB - 1) >> SUB_BITS, 0), yhi = min(maxy >> SUB_BITS, Ho - 1);
    if (xlo > xhi || ylo > yhi) return;
    int64_t sx[3], sy[3], Erow[3], reach[3];                             // the steps of E per pixel along x and y; E at the row's first block
    bool tl[3];
    for (int e = 0; e < 3; ++e) {
        int64_t dx, dy, xa, ya;
        edge_of(t, e, dx, dy, xa, ya);
        tl[e] = top_left(dx, dy);
        sx[e] = -dy * BE_RASTER_SUB;
        sy[e] = dx * BE_RASTER_SUB;
        Erow[e] = dx * ((int64_t)ylo * BE_RASTER_SUB - ya) - dy * ((int64_t)xlo * BE_RASTER_SUB - xa);
        reach[e] = 7 * (hi64(sx[e], 0) + hi64(sy[e], 0));  // the largest E over a block, less E at its origin
    }
    const float fA = (float)t.A;
    const int lane = threadIdx.x & 63, lx = lane & 7, ly = lane >> 3;
    for (int by = ylo; by <= yhi; by += 8) {
        int64_t Eb[3] = {Erow[0], Erow[1], Erow[2]};
        for (int bx = xlo; bx <= xhi; bx += 8) {
            if (Eb[0] + reach[0] >= 0 && Eb[1] + reach[1] >= 0 && Eb[2] + reach[2] >= 0) {
                const int px = bx + lx, py = by + ly;
                if (px <= xhi && py <= yhi) {
                    int64_t E[3];
                    bool inside = true;
                    for (int e = 0; e < 3; ++e) {
                        E[e] = Eb[e] + lx * sx[e] + ly * sy[e];
                        inside = inside && (E[e] > 0 || (E[e] == 0 && tl[e]));
                    }
                    if (inside) {
                        float w[3];
                        const float z = depth_at(t, fA, E, w);
                        if (z > 0.0f && z < __builtin_inff())
                            atomicMin(&zbuf[(int64_t)py * Wo + px], ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(uint32_t)f);
                    }
                }
            }
            for (int e = 0; e < 3; ++e) Eb[e] += 8 * sx[e];
        }
        for (int e = 0; e < 3; ++e) Erow[e] += 8 * sy[e];
    }
}

// one thread per pixel: the winner's depth (the key's high word) and face, and, from the winner's arithmetic recomputed by the
// same operations, the barycentric coordinates and the interpolated maps; +0 / -1 / 0 where nothing landed.  Every output element
// is written exactly once.
__global__ __launch_bounds__(256) void k_raster_resolve(View g, const unsigned long long* __restrict__ zbuf, const int4* __restrict__ rec,
                                                        const int32_t* __restrict__ faces, int64_t V, const float* __restrict__ weight,
                                                        const float* __restrict__ feat, int C, const float* __restrict__ normal,
                                                        const uint8_t* __restrict__ normal_valid, float* __restrict__ depth_out,
                                                        int32_t* __restrict__ face_out, float* __restrict__ weight_out,
                                                        float* __restrict__ feat_out, float* __restrict__ normal_out,
                                                        uint8_t* __restrict__ normal_valid_out, float* __restrict__ bary_out) {
    const int64_t No = (int64_t)g.Ho * g.Wo;
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= No) return;
    const unsigned long long key = zbuf[o];
    bool hit = key != ~0ull;
    const int64_t f = (int64_t)(uint32_t)key;
    depth_out[o] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
    face_out[o] = hit ? (int32_t)f : -1;
    if (!(weight_out || feat_out || normal_out || bary_out)) return;
    Tri t;
    float l[3] = {0.0f, 0.0f, 0.0f};
    if (hit) {
        t = tri_setup(rec, faces, V, f, 0);
        hit = t.ok;                                                      // always: the face put a fragment here
    }
    if (hit) {
        const int py = (int)(o / g.Wo), px = (int)(o - (int64_t)py * g.Wo);
        int64_t E[3];
        for (int e = 0; e < 3; ++e) {
            int64_t dx, dy, xa, ya;
            edge_of(t, e, dx, dy, xa, ya);
            E[e] = dx * ((int64_t)py * BE_RASTER_SUB - ya) - dy * ((int64_t)px * BE_RASTER_SUB - xa);
        }
        float w[3];
        const float z = depth_at(t, (float)t.A, E, w);
        for (int e = 0; e < 3; ++e) l[e] = (w[e] * t.q[e]) * z;
    }
    const int64_t i0 = hit ? t.i[0] : 0, i1 = hit ? t.i[1] : 0, i2 = hit ? t.i[2] : 0;
    if (bary_out) {
        bary_out[o] = l[0];
        bary_out[No + o] = hit && t.swapped ? l[2] : l[1];
        bary_out[2 * No + o] = hit && t.swapped ? l[1] : l[2];
    }
    if (weight_out) weight_out[o] = hit ? (l[0] * weight[i0] + l[1] * weight[i1]) + l[2] * weight[i2] : 0.0f;
    if (feat_out)
        for (int c = 0; c < C; ++c) {
            const float* a = feat + (int64_t)c * V;
            feat_out[(int64_t)c * No + o] = hit ? (l[0] * a[i0] + l[1] * a[i1]) + l[2] * a[i2] : 0.0f;
        }
    if (normal_out) {
        float m[3] = {0.0f, 0.0f, 0.0f};
        bool ok = false;
        if (hit) {
            float n[3];
            for (int k = 0; k < 3; ++k) n[k] = (l[0] * normal[3 * i0 + k] + l[1] * normal[3 * i1 + k]) + l[2] * normal[3 * i2 + k];
            for (int k = 0; k < 3; ++k) m[k] = (g.r[3 * k] * n[0] + g.r[3 * k + 1] * n[1]) + g.r[3 * k + 2] * n[2];
            const float len = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            ok = (!normal_valid || (normal_valid[i0] && normal_valid[i1] && normal_valid[i2])) && len > 0.0f && len < __builtin_inff();
            for (int k = 0; k < 3; ++k) m[k] = ok ? m[k] / len : 0.0f;
        }
        for (int k = 0; k < 3; ++k) normal_out[k * No + o] = m[k];
        normal_valid_out[o] = ok ? 1 : 0;
    }
}

size_t records_bytes(int64_t V) { return (size_t)V * sizeof(int4); }

bool finite(const float* a, int n) {
    for (int i = 0; i < n; ++i)
        if (!(a[i] > -__builtin_inff() && a[i] < __builtin_inff())) return false;
    return true;
}

}  // namespace

extern "C" size_t be_mesh_raster_workspace_bytes(int64_t V, int Ho, int Wo) {
    if (V < 0 || V >= ((int64_t)1 << 31) || Ho < 1 || Wo < 1 || Ho > BE_RASTER_MAX_SIZE || Wo > BE_RASTER_MAX_SIZE) return 0;
    return records_bytes(V) + (size_t)Ho * Wo * sizeof(uint64_t);
}

extern "C" int be_mesh_raster_f32(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const float* weight, const float* feat, int C,
                                  const float* normal, const uint8_t* normal_valid, const float* cam_dst, const float* pose, float near, int cull,
                                  int Ho, int Wo, float* depth_out, int32_t* face_out, float* weight_out, float* feat_out, float* normal_out,
                                  uint8_t* normal_valid_out, float* bary_out, void* workspace, size_t workspace_bytes, void* stream) {
    BE_REQUIRE(V >= 0 && T >= 0 && V < ((int64_t)1 << 31) && T < ((int64_t)1 << 31),
               "be_mesh_raster_f32: V = %lld vertices and T = %lld triangles; both must be in [0, 2^31)", (long long)V, (long long)T);
    BE_REQUIRE(Ho >= 1 && Wo >= 1 && Ho <= BE_RASTER_MAX_SIZE && Wo <= BE_RASTER_MAX_SIZE, "be_mesh_raster_f32: size must be in [1, %d], got %d x %d",
               BE_RASTER_MAX_SIZE, Ho, Wo);
    BE_REQUIRE(cam_dst && pose && depth_out && face_out && workspace, "be_mesh_raster_f32: null pointer");
    BE_REQUIRE((V == 0 || vertices) && (T == 0 || faces), "be_mesh_raster_f32: null vertices with V > 0 or null faces with T > 0");
    BE_REQUIRE(finite(cam_dst, 4) && cam_dst[0] > 0.0f && cam_dst[1] > 0.0f, "be_mesh_raster_f32: cam_dst must be finite with focal lengths > 0");
    BE_REQUIRE(finite(pose, 12), "be_mesh_raster_f32: pose must be finite");
    BE_REQUIRE(near >= 0.0f && near < __builtin_inff(), "be_mesh_raster_f32: near must be a finite number >= 0");
    BE_REQUIRE(cull >= 0 && cull <= 2, "be_mesh_raster_f32: cull must be 0 (none), 1 (back) or 2 (front), got %d", cull);
    BE_REQUIRE(C >= 0 && C <= BE_FUSE_MAX_CHANNELS && (C == 0 || !feat_out || V == 0 || feat),
               "be_mesh_raster_f32: C must be in [0, %d], and feat given when feat_out is", BE_FUSE_MAX_CHANNELS);
    BE_REQUIRE(!weight_out || V == 0 || weight, "be_mesh_raster_f32: weight_out needs weight");
    BE_REQUIRE((normal_out == nullptr) == (normal_valid_out == nullptr) && (!normal_out || V == 0 || normal),
               "be_mesh_raster_f32: normal_out and normal_valid_out are given together or not at all, and need normal");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0 && workspace_bytes >= be_mesh_raster_workspace_bytes(V, Ho, Wo),
               "be_mesh_raster_f32: workspace must be 16-byte aligned and hold be_mesh_raster_workspace_bytes(V, Ho, Wo) = %zu bytes, got %zu",
               be_mesh_raster_workspace_bytes(V, Ho, Wo), workspace_bytes);
    View g;
    g.fy = cam_dst[0]; g.fx = cam_dst[1]; g.cy = cam_dst[2]; g.cx = cam_dst[3];
    for (int i = 0; i < 9; ++i) g.r[i] = pose[i];
    for (int i = 0; i < 3; ++i) g.t[i] = pose[9 + i];
    g.near = near;
    g.Ho = Ho; g.Wo = Wo; g.cull = cull;
    const int64_t No = (int64_t)Ho * Wo;
    int4* rec = static_cast<int4*>(workspace);
    unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + records_bytes(V));
    hipStream_t s = be::as_stream(stream);
    const hipError_t e = hipMemsetAsync(zbuf, 0xff, (size_t)No * sizeof(uint64_t), s);
    if (e != hipSuccess) return be::fail(BE_ELAUNCH, "be_mesh_raster_f32: hipMemsetAsync: %s", hipGetErrorString(e));
    if (V > 0 && T > 0) {
        hipLaunchKernelGGL(k_raster_vertices, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, g, vertices, V, rec);
        if (const int rc = be::check_launch("be_mesh_raster_f32(vertices)")) return rc;
        hipLaunchKernelGGL(k_raster_faces, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, rec, faces, V, T, cull, Ho, Wo, zbuf);
        if (const int rc = be::check_launch("be_mesh_raster_f32(faces)")) return rc;
    }
    hipLaunchKernelGGL(k_raster_resolve, dim3((unsigned)((No + 255) / 256)), dim3(256), 0, s, g, zbuf, rec, faces, V, weight,
                       C > 0 ? feat : nullptr, C, normal, normal_valid, depth_out, face_out, weight_out, C > 0 ? feat_out : nullptr, normal_out,
                       normal_valid_out, bary_out);
    return be::check_launch("be_mesh_raster_f32(resolve)");
}
