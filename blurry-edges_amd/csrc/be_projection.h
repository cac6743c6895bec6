// The projection arithmetic of the forward reprojection, shared by be_reproject.hip (the z-buffer) and be_fuse.hip (the multi-view
// merge): one statement, so that a sample lands on the same target pixel with the same Zd bits in both.
//
// All arithmetic is float32 with one rounding per written operation (no contraction): be_hip/camera.py restates it in numpy,
// operation by operation (camera.project_f32), and the tests hold the kernels to that statement bit for bit.
#pragma once
#include <cstdint>
#include "be_common.h"

#pragma clang fp contract(off)

namespace {

// kernel arguments by value: the two cameras, the pose (row-major R, then t: X' = R X + t, source frame -> target frame), the
// source lattice (sample (iy, ix) of Ws columns sits at (top + iy / k, left + ix / k) in source pixels) and the target frame
struct Geom {
    float fy, fx, cy, cx;
    float fyd, fxd, cyd, cxd;
    float r[9], t[3];
    float near;
    int top, left, k, Ws;
    int Ho, Wo;
    int64_t Ns;
};

struct Proj { float Xd, Yd, Zd, fu, fv; bool z_ok; };

__device__ __forceinline__ Proj project(const Geom& g, int64_t i, float Z) {
    Proj p;
    const int iy = (int)(i / g.Ws), ix = (int)(i - (int64_t)iy * g.Ws);
    const float y = (float)g.top + (float)iy / (float)g.k;
    const float x = (float)g.left + (float)ix / (float)g.k;
    const float xn = (x - g.cx) / g.fx;
    const float yn = (y - g.cy) / g.fy;
    const float X = xn * Z;
    const float Y = yn * Z;
    p.Xd = ((g.r[0] * X + g.r[1] * Y) + g.r[2] * Z) + g.t[0];
    p.Yd = ((g.r[3] * X + g.r[4] * Y) + g.r[5] * Z) + g.t[1];
    p.Zd = ((g.r[6] * X + g.r[7] * Y) + g.r[8] * Z) + g.t[2];
    const float u = (g.fxd * p.Xd) / p.Zd + g.cxd;
    const float v = (g.fyd * p.Yd) / p.Zd + g.cyd;
    p.fu = floorf(u + 0.5f);
    p.fv = floorf(v + 0.5f);
    p.z_ok = Z > 0.0f && Z < __builtin_inff();                  // NaN fails both
    return p;
}

// which samples splat: Z valid, near < Zd < inf (a huge finite Z may overflow Zd) and the rounded target inside the frame - tested
// in float, before any conversion to int: NaN and the infinities fail it (camera.taking_part)
__device__ __forceinline__ bool taking_part(const Geom& g, const Proj& p) {
    return p.z_ok && p.Zd > g.near && p.Zd < __builtin_inff() && p.fu >= 0.0f && p.fu < (float)g.Wo && p.fv >= 0.0f &&
           p.fv < (float)g.Ho;
}

constexpr int64_t SAMPLES_MAX = 0x7fffffff;        // the index map is int32 and -1 means "nothing landed"

inline int make_geom(const char* who, int Hs, int Ws, int scale, int top, int left, const float* cam_src, const float* cam_dst,
                     const float* pose, float near, int Ho, int Wo, Geom* g) {
    BE_REQUIRE(cam_src && cam_dst && pose, "%s: null pointer", who);
    BE_REQUIRE(Hs >= 1 && Ws >= 1, "%s: the source must hold at least one sample, got %d x %d", who, Hs, Ws);
    BE_REQUIRE((int64_t)Hs * Ws <= SAMPLES_MAX, "%s: %lld source samples; at most 2^31 - 1 (the index map is int32)", who,
               (long long)Hs * Ws);
    BE_REQUIRE(scale >= 1 && scale <= BE_RENDER_AT_MAX_SCALE, "%s: scale must be in [1, %d], got %d", who, BE_RENDER_AT_MAX_SCALE, scale);
    BE_REQUIRE(top >= 0 && left >= 0 && top <= (1 << 24) && left <= (1 << 24), "%s: bad window origin (%d, %d)", who, top, left);
    BE_REQUIRE(Ho >= 1 && Wo >= 1 && (int64_t)Ho * Wo <= SAMPLES_MAX && Ho <= (1 << 24) && Wo <= (1 << 24),
               "%s: bad target size %d x %d", who, Ho, Wo);
    BE_REQUIRE(near >= 0.0f, "%s: near must be >= 0", who);
    g->fy = cam_src[0]; g->fx = cam_src[1]; g->cy = cam_src[2]; g->cx = cam_src[3];
    g->fyd = cam_dst[0]; g->fxd = cam_dst[1]; g->cyd = cam_dst[2]; g->cxd = cam_dst[3];
    for (int i = 0; i < 9; ++i) g->r[i] = pose[i];
    for (int i = 0; i < 3; ++i) g->t[i] = pose[9 + i];
    g->near = near;
    g->top = top; g->left = left; g->k = scale; g->Ws = Ws;
    g->Ho = Ho; g->Wo = Wo;
    g->Ns = (int64_t)Hs * Ws;
    return BE_OK;
}

}  // namespace
