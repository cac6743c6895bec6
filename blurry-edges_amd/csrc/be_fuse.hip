// Multi-view depth fusion: the depth maps of V views, each with its own camera and pose, merged in one target camera
// (be_fuse_views_f32).  Every sample is projected as be_reproject.hip projects it (be_projection.h); per target pixel
// the samples within tau behind the nearest one are averaged with their weights, a pixel is kept when enough distinct views agree,
// and a front cluster that too few views confirm is peeled off so that the next round looks behind it.
//
// Nothing is accumulated in floating point: the front is an unsigned minimum over the bits of Zd, the sums are 64-bit integers of
// fixed-point terms (weights in units of 2^-16, depth offsets in units of 2^-20 m), the view set is a bit mask under OR.  Integer
// min / add / or are associative and commutative, so every output is a function of the inputs alone: independent of the order of
// execution and of the order of the views.  be_hip/fusion.py restates the whole schedule in numpy and the tests hold the kernels
// to it bit for bit.  The sums are exact while fewer than 2^16 samples agree on one pixel (wq <= 2^20, dq <= 2^23, |fq| <= 2^27).
//
// All float arithmetic is float32 with one rounding per written operation (no contraction); the means are formed in double from
// the integer sums and rounded to float once.
#include <cstdint>
#include "be_common.h"
#include "be_projection.h"   // Geom, Proj, project, taking_part, make_geom: shared with be_reproject.hip

#pragma clang fp contract(off)

namespace {

constexpr uint32_t EMPTY = 0xffffffffu;             // no sample: as a float a NaN, which fails every test of k_fuse_add
constexpr uint32_t DONE = 0xffffffffu;              // a finalised pixel's floor: a NaN, behind which no sample lies (Zd > NaN is false)

// the per-pixel state in the caller's scratch: 64-bit arrays first, all [No] except swf [C,No]
struct State {
    unsigned long long* sw;                         // sum of wq
    unsigned long long* swd;                        // sum of wq * dq
    unsigned long long* swf;                        // sums of wq * fq_c, two's complement
    uint32_t* zmin;                                 // bits of the nearest Zd behind the floor
    float* floor;
    float* base;                                    // the recentred pass measures offsets from here
    uint32_t* cnt;
    uint32_t* mask;
};

// wq = floorf(min(w, 16) * 65536 + 0.5) for w > 0, else 0 (NaN fails w > 0): at most 2^20
__device__ __forceinline__ uint32_t quantise_weight(const float* __restrict__ weight, int64_t i) {
    if (!weight) return 65536u;
    const float w = weight[i];
    if (!(w > 0.0f)) return 0u;
    return (uint32_t)floorf(fminf(w, 16.0f) * 65536.0f + 0.5f);
}

// the target pixel of sample i, or -1 when it does not take part; its Zd and quantised weight
__device__ __forceinline__ int64_t land(const Geom& g, const float* __restrict__ depth, const float* __restrict__ weight, int64_t i,
                                        float* Zd, uint32_t* wq) {
    const Proj p = project(g, i, depth[i]);
    if (!taking_part(g, p)) return -1;
    *wq = quantise_weight(weight, i);
    if (*wq == 0u) return -1;
    *Zd = p.Zd;
    return (int64_t)(int)p.fv * g.Wo + (int)p.fu;   // 0 <= fv < Ho, 0 <= fu < Wo: inside [0, Ho * Wo)
}

// one thread per sample: a sample that takes part and lies behind its pixel's floor issues one no-return 32-bit unsigned minimum
// (a positive float orders as its bit pattern)
__global__ __launch_bounds__(256) void k_fuse_front(Geom g, const float* __restrict__ depth, const float* __restrict__ weight,
                                                    const float* __restrict__ floor, uint32_t* __restrict__ zmin) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.Ns) return;
    float Zd;
    uint32_t wq;
    const int64_t o = land(g, depth, weight, i, &Zd, &wq);
    if (o < 0 || !(Zd > floor[o])) return;
    atomicMin(&zmin[o], __float_as_uint(Zd));
}

// one thread per sample: a sample within [base, base + span] of its pixel adds its fixed-point terms with no-return integer atomics.
// swf == nullptr: a pass whose mean only recentres the window carries no channels.
__global__ __launch_bounds__(256) void k_fuse_add(Geom g, const float* __restrict__ depth, const float* __restrict__ weight,
                                                  const float* __restrict__ feat, int C, int view, const float* base, float span,
                                                  unsigned long long* sw, unsigned long long* swd, unsigned long long* swf,
                                                  uint32_t* cnt, uint32_t* mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.Ns) return;
    float Zd;
    uint32_t wq;
    const int64_t o = land(g, depth, weight, i, &Zd, &wq);
    if (o < 0) return;
    const float d = Zd - base[o];
    if (!(d >= 0.0f && d <= span)) return;                              // NaN (no front on this pixel) fails
    const unsigned long long dq = (unsigned long long)floorf(d * 1048576.0f + 0.5f);
    atomicAdd(&sw[o], (unsigned long long)wq);
    atomicAdd(&swd[o], (unsigned long long)wq * dq);
    atomicAdd(&cnt[o], 1u);
    atomicOr(&mask[o], 1u << view);
    if (!swf) return;
    const int64_t No = (int64_t)g.Ho * g.Wo;
    for (int c = 0; c < C; ++c) {
        const float f = feat[(int64_t)c * g.Ns + i];
        const float fc = f != f ? 0.0f : fminf(fmaxf(f, -2048.0f), 2048.0f);
        const long long fq = (long long)floorf(fc * 65536.0f + 0.5f);
        atomicAdd(&swf[(int64_t)c * No + o], (unsigned long long)((long long)wq * fq));
    }
}

struct Out {
    float* depth;
    float* weight;
    int32_t* views;
    int32_t* count;
    int32_t* layer;
    float* feat;                                    // [C,No]
};

// one thread per pixel, after an add pass: the mean from the integer sums, then either the recentred window (decide = 0:
// base = m - tau) or the decision of round `layer` (decide = 1): finalise, peel or give up.  Clears the sums it read; the decision
// also resets the front.  last: the pixels still open take the empty value, so that every output element is written exactly once.
__global__ __launch_bounds__(256) void k_fuse_step(State s, Out out, int64_t No, int C, const float* base_in, float tau, float span,
                                                   int decide, int min_views, int layer, int last) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= No) return;
    const unsigned long long sw = s.sw[o], swd = s.swd[o];
    const uint32_t cnt = s.cnt[o], mask = s.mask[o];
    const float base = base_in[o];
    const bool any = cnt > 0u;
    const float m = any ? (float)((double)base + (double)swd / (double)sw * 0x1p-20) : __uint_as_float(EMPTY);
    s.sw[o] = 0ull;
    s.swd[o] = 0ull;
    s.cnt[o] = 0u;
    s.mask[o] = 0u;
    if (!decide) {
        s.base[o] = any ? m - tau : __uint_as_float(EMPTY);
        return;
    }
    s.zmin[o] = EMPTY;
    const float fl = s.floor[o];
    const bool done = fl != fl;
    const int nv = __popc(mask);
    const bool fin = !done && any && nv >= min_views;
    if (fin) {
        out.depth[o] = m;
        out.weight[o] = (float)((double)sw * 0x1p-16);
        out.views[o] = nv;
        out.count[o] = (int32_t)cnt;
        out.layer[o] = layer;
        s.floor[o] = __uint_as_float(DONE);
    } else if (!done) {
        s.floor[o] = any ? base + span : __builtin_inff();
        if (last) {
            out.depth[o] = 0.0f;
            out.weight[o] = 0.0f;
            out.views[o] = 0;
            out.count[o] = 0;
            out.layer[o] = -1;
        }
    }
    for (int c = 0; c < C; ++c) {
        const int64_t j = (int64_t)c * No + o;
        const long long swf = (long long)s.swf[j];
        s.swf[j] = 0ull;
        if (fin) out.feat[j] = (float)((double)swf / (double)sw * 0x1p-16);
        else if (!done && last) out.feat[j] = 0.0f;
    }
}

constexpr int64_t PIXEL_BYTES = 2 * 8 + 5 * 4;     // sw, swd; zmin, floor, base, cnt, mask

}  // namespace

extern "C" int64_t be_fuse_scratch_bytes(int Ho, int Wo, int C) {
    if (Ho < 1 || Wo < 1 || Ho > (1 << 24) || Wo > (1 << 24) || (int64_t)Ho * Wo > SAMPLES_MAX || C < 0 || C > BE_FUSE_MAX_CHANNELS) return -1;
    return (int64_t)Ho * Wo * (PIXEL_BYTES + 8 * (int64_t)C);
}

extern "C" int be_fuse_views_f32(int V, const float* const* depth, const float* const* weight, const float* const* feat, int C,
                                 const int* Hs, const int* Ws, const int* scale, const int* top, const int* left,
                                 const float* cam_src, const float* pose, const float* cam_dst, float near, int Ho, int Wo, float tau,
                                 int min_views, int recentre, int peel, void* scratch, float* depth_out, float* weight_out,
                                 int32_t* views_out, int32_t* count_out, int32_t* layer_out, float* feat_out, void* stream) {
    BE_REQUIRE(V >= 1 && V <= BE_FUSE_MAX_VIEWS, "be_fuse_views_f32: the number of views must be in [1, %d], got %d", BE_FUSE_MAX_VIEWS, V);
    BE_REQUIRE(depth && Hs && Ws && scale && top && left && cam_src && pose && cam_dst, "be_fuse_views_f32: null pointer");
    BE_REQUIRE(scratch && depth_out && weight_out && views_out && count_out && layer_out, "be_fuse_views_f32: null pointer");
    BE_REQUIRE(C >= 0 && C <= BE_FUSE_MAX_CHANNELS && (C == 0 || (feat && feat_out)),
               "be_fuse_views_f32: C must be in [0, %d], and feat / feat_out given when C > 0", BE_FUSE_MAX_CHANNELS);
    BE_REQUIRE(tau >= 0.0f && tau <= 4.0f, "be_fuse_views_f32: tau must be a finite number in [0, 4]");
    BE_REQUIRE(min_views >= 1 && min_views <= V, "be_fuse_views_f32: min_views must be in [1, %d], got %d", V, min_views);
    BE_REQUIRE(peel >= 0 && peel <= BE_FUSE_MAX_PEEL, "be_fuse_views_f32: peel must be in [0, %d], got %d", BE_FUSE_MAX_PEEL, peel);
    BE_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "be_fuse_views_f32: scratch must be 8-byte aligned");
    Geom g[BE_FUSE_MAX_VIEWS];
    for (int v = 0; v < V; ++v) {
        BE_REQUIRE(depth[v] && (C == 0 || feat[v]), "be_fuse_views_f32: view %d: null pointer", v);
        if (const int rc = make_geom("be_fuse_views_f32", Hs[v], Ws[v], scale[v], top[v], left[v], cam_src + 4 * v, cam_dst, pose + 12 * v,
                                     near, Ho, Wo, &g[v]))
            return rc;
    }
    const int64_t No = (int64_t)Ho * Wo;
    State s;
    s.sw = static_cast<unsigned long long*>(scratch);
    s.swd = s.sw + No;
    s.swf = s.swd + No;
    s.zmin = reinterpret_cast<uint32_t*>(s.swf + (int64_t)C * No);
    s.floor = reinterpret_cast<float*>(s.zmin + No);
    s.base = s.floor + No;
    s.cnt = reinterpret_cast<uint32_t*>(s.base + No);
    s.mask = s.cnt + No;
    const Out out{depth_out, weight_out, views_out, count_out, layer_out, feat_out};
    hipStream_t st = be::as_stream(stream);
    // the initial clear: every sum 0, every floor +0, every front empty
    hipError_t e = hipMemsetAsync(scratch, 0, (size_t)(No * (PIXEL_BYTES + 8 * (int64_t)C)), st);
    if (e == hipSuccess) e = hipMemsetAsync(s.zmin, 0xff, (size_t)No * sizeof(uint32_t), st);
    if (e != hipSuccess) return be::fail(BE_ELAUNCH, "be_fuse_views_f32: hipMemsetAsync: %s", hipGetErrorString(e));
    const float* zmin_f = reinterpret_cast<const float*>(s.zmin);
    const float span2 = tau + tau;
    const dim3 pixels((unsigned)((No + 255) / 256));
    auto add = [&](const float* base, float span, bool with_feat) {
        for (int v = 0; v < V; ++v)
            hipLaunchKernelGGL(k_fuse_add, dim3((unsigned)((g[v].Ns + 255) / 256)), dim3(256), 0, st, g[v], depth[v], weight ? weight[v] : nullptr,
                               C > 0 ? feat[v] : nullptr, C, v, base, span, s.sw, s.swd, with_feat && C > 0 ? s.swf : nullptr, s.cnt, s.mask);
    };
    // the schedule is a function of (V, recentre, peel) alone
    for (int r = 0; r <= peel; ++r) {
        const int last = r == peel;
        for (int v = 0; v < V; ++v)
            hipLaunchKernelGGL(k_fuse_front, dim3((unsigned)((g[v].Ns + 255) / 256)), dim3(256), 0, st, g[v], depth[v], weight ? weight[v] : nullptr,
                               s.floor, s.zmin);
        if (const int rc = be::check_launch("be_fuse_views_f32(front)")) return rc;
        add(zmin_f, tau, !recentre);
        if (const int rc = be::check_launch("be_fuse_views_f32(add)")) return rc;
        if (recentre) {
            hipLaunchKernelGGL(k_fuse_step, pixels, dim3(256), 0, st, s, out, No, 0, zmin_f, tau, tau, 0, min_views, r, last);
            add(s.base, span2, true);
            if (const int rc = be::check_launch("be_fuse_views_f32(recentred add)")) return rc;
            hipLaunchKernelGGL(k_fuse_step, pixels, dim3(256), 0, st, s, out, No, C, s.base, tau, span2, 1, min_views, r, last);
        } else {
            hipLaunchKernelGGL(k_fuse_step, pixels, dim3(256), 0, st, s, out, No, C, zmin_f, tau, tau, 1, min_views, r, last);
        }
        if (const int rc = be::check_launch("be_fuse_views_f32(step)")) return rc;
    }
    return BE_OK;
}
