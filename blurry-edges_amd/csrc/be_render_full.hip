// Full render pass ("pass B") + owner-computes fold, gfx950.
//
// Replaces PostProcess.get_patches(colors_only=False) and the six nn.Fold aggregations of
// blurry_edges_test.py:36-79,93-99 / utils/postprocessing_loss.py:151-173 (and the per-block patch-tensor
// stitching of blurry_edges_test_big.py:166-189) with two steps and NO per-patch tensors in HBM:
//
//   k_render_records   one wavefront per patch position: both aperture images are read once (gather-on-read
//                      through a strided patch view: an image pair, an unfolded tensor or flat patches),
//                      the 882-row ridge system is reduced with wave shuffles, solved in fp64, the two
//                      wedge depths come from etas2depth, the refocus radii from depth2sigma and a wave
//                      ballot of the depth mask; result = one 128-byte record per patch.
//   the folds          one thread per output sample ("owner computes"): walks the <= 11x11 patches that cover the
//                      sample in a fixed order and re-evaluates the wedges from the records.  Deterministic (no
//                      atomics), divides by the number of patches visited.  A fold is a sampler (k_fold_pixels,
//                      k_fold_lattice, k_fold_points: where the samples are) instantiated with an accumulator
//                      (MapsAcc: the six maps of the four blur sets - aperture 1, aperture 2, sharpened, refocused -
//                      boundary, depth and confidence; StackAcc: a focal stack); see the fold section.
//
// Every kernel is templated on how a patch's origin is obtained: UNIFORM (origin = stride * index, the grid of
// nn.Unfold) or ORIGIN TABLES ys[HP] / xs[WP] (a separable grid whose last line may sit flush with the image edge, so an
// image of any size is covered).
//
// The reference materialises 26.5 KB per patch pair and folds it six times; here the per-patch state is
// 128 B and every output byte is written once.
#include "be_common.h"
#include "be_wedge.h"

namespace {

constexpr int NPIX = BE_NPIX;
constexpr int R = BE_R;
constexpr int PASSES = (NPIX + 63) / 64;
constexpr int WAVES_PER_BLOCK = 4;
constexpr int REC = BE_RECORD_FLOATS;   // 32

// record layout (floats)
enum { R_GEOM = 0 /* x0,y0,x1,y1,s11,c11,s12,c12,s21,c21,s22,c22,sg1,sg2 */, R_RAD1 = 14, R_RAD2 = 16, R_RADF = 18,
       R_COL = 20, R_DEPTH = 29, R_FLAGS = 31 };

struct FullArgs {
    const float* params12;   // [P,12]
    be_patch_view v;
    float* records;          // [P,32]
    float* patches;          // [P,2,3,441] or null
    float* shpd;             // [P,3,441] or null
    float* refoc;            // [P,3,441] or null
    float* boundary;         // [P,441] or null
    float* depth_map;        // [P,441] or null
    int32_t* depth_mask;     // [P,441] or null
    float rho_prime;
    int densify_w;
    int64_t n;
    const int32_t* ys;       // [HP] / [WP] patch origins (pixels), k_render_records<true> only
    const int32_t* xs;
    int y_max, x_max;        // H - R, W - R: an origin outside [0, max] is clamped (no read leaves the image)
};

__device__ __forceinline__ void composite3(const float* col, float u0, float u1, float u2, float* out, int pix) {
#pragma clang fp contract(off)
    out[pix]            = u0 * col[0] + u1 * col[1] + u2 * col[2];
    out[NPIX + pix]     = u0 * col[3] + u1 * col[4] + u2 * col[5];
    out[2 * NPIX + pix] = u0 * col[6] + u1 * col[7] + u2 * col[8];
}

template <bool TABLES>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK)
void k_render_records(be_render_opts o, be_depth_consts dc, FullArgs a) {
    __shared__ float lin[R];
    if (threadIdx.x < R) lin[threadIdx.x] = o.lin[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t patch = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (patch >= a.n) return;

    const float* p = a.params12 + patch * 12;
    const be::WedgeGeom g = be::make_geom(p, o.wrap_angles != 0);
    float eta[4], rad[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma clang fp contract(off)
        eta[k] = be::param2eta(p[8 + k]);              // (w1,img1) (w2,img1) (w1,img2) (w2,img2)
        rad[k] = be::kRoot2 * eta[k];
    }
    const int pi = (int)(patch / a.v.wp), pj = (int)(patch % a.v.wp);
    const float* img1;
    if constexpr (TABLES) {
        const int oy = min(max(a.ys[pi], 0), a.y_max), ox = min(max(a.xs[pj], 0), a.x_max);
        img1 = a.v.base + oy * a.v.s_row + ox * a.v.s_col;
    } else {
        img1 = a.v.base + pi * a.v.s_pi + pj * a.v.s_pj;
    }
    const float* img2 = img1 + a.v.s_aperture;

    float d1s[PASSES], d2s[PASSES];
    float gs[6] = {0, 0, 0, 0, 0, 0};
    float bs[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool any1 = false, any2 = false;
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int pix = it * 64 + lane;
        const bool live = pix < NPIX;
        const int pc = live ? pix : 0;
        const int row = pc / R, col = pc - row * R;
        float d1, d2;
        be::wedge_dists(g, lin[col], lin[row], o.w, d1, d2);
        d1s[it] = d1; d2s[it] = d2;
        const int64_t off = row * a.v.s_row + col * a.v.s_col;
#pragma unroll
        for (int im = 0; im < 2; ++im) {
            float u0, u1, u2;
            be::indicators(d1, d2, rad[2 * im], rad[2 * im + 1], u0, u1, u2);
            if (!live) { u0 = 0.f; u1 = 0.f; u2 = 0.f; }
            const float* src = (im ? img2 : img1) + off;
            const float yr = live ? src[0] : 0.f, yg = live ? src[a.v.s_chan] : 0.f, yb = live ? src[2 * a.v.s_chan] : 0.f;
            gs[0] = fmaf(u0, u0, gs[0]); gs[1] = fmaf(u0, u1, gs[1]); gs[2] = fmaf(u0, u2, gs[2]);
            gs[3] = fmaf(u1, u1, gs[3]); gs[4] = fmaf(u1, u2, gs[4]); gs[5] = fmaf(u2, u2, gs[5]);
            bs[0] = fmaf(u0, yr, bs[0]); bs[1] = fmaf(u0, yg, bs[1]); bs[2] = fmaf(u0, yb, bs[2]);
            bs[3] = fmaf(u1, yr, bs[3]); bs[4] = fmaf(u1, yg, bs[4]); bs[5] = fmaf(u1, yb, bs[5]);
            bs[6] = fmaf(u2, yr, bs[6]); bs[7] = fmaf(u2, yg, bs[7]); bs[8] = fmaf(u2, yb, bs[8]);
        }
        if (live) {
            const int m = be::depth_mask(d1, d2, o.delta_sq, a.densify_w != 0);
            any1 |= (m == 1); any2 |= (m == 2);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) gs[k] = be::wave_sum(gs[k]);
#pragma unroll
    for (int k = 0; k < 9; ++k) bs[k] = be::wave_sum(bs[k]);
    const be::Colors9 col = be::solve_colors(gs[0] + o.lambda_ridge, gs[1], gs[2], gs[3] + o.lambda_ridge, gs[4],
                                             gs[5] + o.lambda_ridge, bs);
    int br;
    const float z1 = be::etas2depth(dc, eta[0], eta[2], br);      // blurry_edges_test.py:44
    const float z2 = be::etas2depth(dc, eta[1], eta[3], br);      // :45
    const bool has1 = __ballot(any1) != 0ull, has2 = __ballot(any2) != 0ull;
    float radf[2];
    {
#pragma clang fp contract(off)
        const float s1 = has1 ? be::depth2sigma(dc, z1, a.rho_prime) : 1e-4f;     // :66-71
        const float s2 = has2 ? be::depth2sigma(dc, z2, a.rho_prime) : 1e-4f;
        radf[0] = be::kRoot2 * s1; radf[1] = be::kRoot2 * s2;
    }
    if (lane == 0) {
        float* r = a.records + patch * REC;
        r[0] = g.x0; r[1] = g.y0; r[2] = g.x1; r[3] = g.y1;
        r[4] = g.s11; r[5] = g.c11; r[6] = g.s12; r[7] = g.c12; r[8] = g.s21; r[9] = g.c21; r[10] = g.s22; r[11] = g.c22;
        r[12] = g.sg1; r[13] = g.sg2;
        r[R_RAD1] = rad[0]; r[R_RAD1 + 1] = rad[1]; r[R_RAD2] = rad[2]; r[R_RAD2 + 1] = rad[3];
        r[R_RADF] = radf[0]; r[R_RADF + 1] = radf[1];
#pragma unroll
        for (int k = 0; k < 9; ++k) r[R_COL + k] = col.c[k];
        r[R_DEPTH] = z1; r[R_DEPTH + 1] = z2;
        r[R_FLAGS] = (float)((has1 ? 1 : 0) | (has2 ? 2 : 0));
    }
    // ---- optional materialised per-patch outputs (parity tests / callers that want the reference's tensors)
    const bool want = a.patches || a.shpd || a.refoc || a.boundary || a.depth_map || a.depth_mask;
    if (!want) return;
    const float rs = be::kRoot2 * 1e-4f;                              // sharpened: eta = 1e-4 for both wedges (:63)
#pragma unroll
    for (int it = 0; it < PASSES; ++it) {
        const int pix = it * 64 + lane;
        if (pix >= NPIX) continue;
        const float d1 = d1s[it], d2 = d2s[it];
        float u0, u1, u2;
        if (a.patches) {
            be::indicators(d1, d2, rad[0], rad[1], u0, u1, u2);
            composite3(col.c, u0, u1, u2, a.patches + patch * 6 * NPIX, pix);
            be::indicators(d1, d2, rad[2], rad[3], u0, u1, u2);
            composite3(col.c, u0, u1, u2, a.patches + patch * 6 * NPIX + 3 * NPIX, pix);
        }
        if (a.shpd) { be::indicators(d1, d2, rs, rs, u0, u1, u2); composite3(col.c, u0, u1, u2, a.shpd + patch * 3 * NPIX, pix); }
        if (a.refoc) { be::indicators(d1, d2, radf[0], radf[1], u0, u1, u2);
                       composite3(col.c, u0, u1, u2, a.refoc + patch * 3 * NPIX, pix); }
        if (a.boundary) a.boundary[patch * NPIX + pix] = be::boundary_value(d1, d2, o.delta_sq);
        const int m = be::depth_mask(d1, d2, o.delta_sq, a.densify_w != 0);
        if (a.depth_mask) a.depth_mask[patch * NPIX + pix] = m;
        if (a.depth_map) a.depth_map[patch * NPIX + pix] = m == 1 ? z1 : (m == 2 ? z2 : 0.0f);
    }
}

// ------------------------------------------------------------------------------------------------ fold
// Every fold is  sampler -> run -> visit -> accumulator, each written once:
//
//   sampler      where the output samples are.  k_fold_pixels (one thread per image pixel), k_fold_lattice (a lattice `scale`
//                times finer, over a window), k_fold_points (a list of real-valued positions).  A sampler turns its sample into
//                one Axis per image axis, picks the output index and says where the grid lines come from (*Lines, below).
//   run          fold_run: the contiguous run of grid lines covering the sample on either axis, visited i outer, j inner,
//                ascending; returns the number of patches visited.
//   visit        visit_record: one record -> registers -> WedgeGeom -> wedge_dists -> accumulator.
//   accumulator  what is summed per visit and how it is stored: MapsAcc (the six folded maps) or StackAcc (a chunk of
//                focal-stack planes).
//
// The equalities the entry points promise (every scale-th lattice sample == the pixel fold; a point on a pixel centre == the
// pixel fold; a dyadic point == the lattice fold; stack plane k == render + fold at rho_k) hold bit for bit because the
// siblings run the SAME statements after the coordinate, not copies of them.  What decides bits:
//   - `#pragma clang fp contract(off)` is lexically scoped and does not reach into a callee: each function below that needs
//     it carries its own (lattice_coord, blend_add, MapsAcc::add, StackAcc::add); visit_record and wedge_dists are outside it.
//   - the visiting order and the single division by (float)cnt in Acc::store.
struct FoldGrid {            // the record grid a fold reads
    const float* records;    // [hp*wp,32]
    int hp, wp, H, W, stride;
    const int32_t* ys;       // [hp] / [wp] patch origins, strictly increasing (TABLES instantiations only; stride is then 0)
    const int32_t* xs;
};

constexpr int FOLD_TILE = 16;                       // output samples per workgroup and axis (pixel and lattice samplers)
constexpr int FOLD_LINES = FOLD_TILE + R - 1;       // strictly increasing integer origins: at most one grid line per pixel
                                                    // of [tile_first - (R-1), tile_last] can cover a pixel of the tile
constexpr int LINE_NONE = 0x7fffffff;
constexpr int FOLD_KC = BE_REFOCUS_STACK_KC;        // focal-stack planes per workgroup (the last chunk may be short)

// first index in t[0..n) with t[i] >= v (t increasing)
__device__ __forceinline__ int lower_bound(const int32_t* __restrict__ t, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (t[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

// One colour accumulator.  A 3-vector, not float[3]: as a member of an accumulator struct a float[3] is split into scalars, the
// compiler then packs fewer of the blends and of the indicator arithmetic into v_pk_* than it does for a kernel-local array,
// and the map folds pay about ten more instructions per visited record.  With the vector the packing is the local array's.
typedef float Rgb __attribute__((ext_vector_type(3)));

// acc[c] += the three wedge colours of channel c blended by the indicators (no FMA: the bits of the reference's mul + add)
__device__ __forceinline__ void blend_add(Rgb& acc, const float* col, float u0, float u1, float u2) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
}

// ---- accumulators.  Interface: Acc(o, a, z); add(r, d1, d2) per visited record; store(n, plane_stride, at) with n = (float)cnt;
// store_zero(plane_stride, at) for a sample outside the domain - it writes exactly the outputs store writes.  `z` is the launch's
// extra grid index: the plane chunk for StackAcc; MapsAcc has none (the pixel sampler alone uses it, to pick the image of a
// batch).  Everything lives in registers: the kernels keep 0 bytes of scratch (check the compiler's resource report after a
// change here: r[REC] and the accumulators pass through three inlined calls).
struct FoldArgs {
    FoldGrid g;
    int densify_w;
    float* image;            // [2,3,*] or null        (* = H,W | Ho,Wo | N: plane_stride elements)
    float* shpd;             // [3,*] or null
    float* refoc;            // [3,*] or null
    float* bndry;            // [*] or null
    float* depth;            // [*] or null
    float* conf;             // [*] or null
    int64_t rec_stride;      // batched form (pixel sampler only, grid.z = image): floats between the records of consecutive images
    __device__ __forceinline__ void select_image(unsigned b) {  // image b of a batch; maps are [B,...,H,W]
        if (!b) return;
        const size_t hw = (size_t)g.H * g.W;
        g.records += b * rec_stride;
        if (image) image += b * 6 * hw;
        if (shpd) shpd += b * 3 * hw;
        if (refoc) refoc += b * 3 * hw;
        if (bndry) bndry += b * hw;
        if (depth) depth += b * hw;
        if (conf) conf += b * hw;
    }
};

struct MapsAcc {
    using Args = FoldArgs;
    static constexpr bool BATCHED = true;
    const be_render_opts& o;
    const FoldArgs& a;
    Rgb acc1 = 0.f, acc2 = 0.f, accs = 0.f, accf = 0.f;
    float accb = 0.f, accz = 0.f;
    int cntz = 0;
    __device__ __forceinline__ MapsAcc(const be_render_opts& o_, const FoldArgs& a_, unsigned) : o(o_), a(a_) {}

    __device__ __forceinline__ void add(const float* r, float d1, float d2) {
#pragma clang fp contract(off)
        const float rs = be::kRoot2 * 1e-4f;                    // sharpened: eta = 1e-4 for both wedges
        const float* col = r + R_COL;
        float u0, u1, u2;
        if (a.image) {
            be::indicators(d1, d2, r[R_RAD1], r[R_RAD1 + 1], u0, u1, u2);
            blend_add(acc1, col, u0, u1, u2);
            be::indicators(d1, d2, r[R_RAD2], r[R_RAD2 + 1], u0, u1, u2);
            blend_add(acc2, col, u0, u1, u2);
        }
        if (a.shpd) { be::indicators(d1, d2, rs, rs, u0, u1, u2); blend_add(accs, col, u0, u1, u2); }
        if (a.refoc) { be::indicators(d1, d2, r[R_RADF], r[R_RADF + 1], u0, u1, u2); blend_add(accf, col, u0, u1, u2); }
        if (a.bndry) accb += be::boundary_value(d1, d2, o.delta_sq);
        if (a.depth || a.conf) {
            const int m = be::depth_mask(d1, d2, o.delta_sq, a.densify_w != 0);
            // m is 0, 1 or 2: the depth of wedge m joins the sum.  One arm, not `if (m == 1) .. else if (m == 2) ..`: inlined into
            // the samplers the two arms were merged by the compiler anyway, into a dozen more exec-mask instructions per visit
            if (m != 0) { accz += m == 1 ? r[R_DEPTH] : r[R_DEPTH + 1]; ++cntz; }
        }
    }
    // n = nn.Fold(ones) at the sample: the patches visited (0 only where a uniform grid stops short of the edge)
    template <bool ZERO = false>
    __device__ __forceinline__ void store(float n, size_t hw, size_t at) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.image) { a.image[c * hw + at] = ZERO ? 0.f : acc1[c] / n; a.image[(3 + c) * hw + at] = ZERO ? 0.f : acc2[c] / n; }
            if (a.shpd) a.shpd[c * hw + at] = ZERO ? 0.f : accs[c] / n;
            if (a.refoc) a.refoc[c * hw + at] = ZERO ? 0.f : accf[c] / n;
        }
        if (a.bndry) a.bndry[at] = ZERO ? 0.f : accb / n;
        if (a.depth) a.depth[at] = ZERO ? 0.f : accz / (cntz > 0 ? (float)cntz : 1.0f);       // postprocessing_loss.py:170-172
        if (a.conf) a.conf[at] = ZERO ? 0.f : (float)cntz / n;
    }
    __device__ __forceinline__ void store_zero(size_t hw, size_t at) const { store<true>(0.f, hw, at); }
};

// K refocused images from ONE record grid: the refocus radius of a wedge is sqrt(2) * depth2sigma(z, rho') (or sqrt(2) * 1e-4
// when the wedge owns no mask pixel), a function of the record's R_DEPTH / R_FLAGS and the plane's optical power alone, so the
// record visit and the run search are done once per covering patch and shared by the planes of a chunk.  Plane k is
// k_render_records(rho_prime = rho_k) + the `refoc` map of MapsAcc bit for bit: same radius expression, same indicators /
// blend_add under contract(off), same visiting order, one division by the number of patches visited.
struct StackArgs {
    FoldGrid g;
    be_depth_consts dc;
    const float* rho_primes; // [K] optical powers, device
    float* out;              // [K,3,*]
    int K;
};

struct StackAcc {
    using Args = StackArgs;
    static constexpr bool BATCHED = false;
    const StackArgs& a;
    const int k0, nk;                                           // first plane and planes of this chunk (uniform over the workgroup)
    float rho[FOLD_KC];
    Rgb acc[FOLD_KC];
    __device__ __forceinline__ StackAcc(const be_render_opts&, const StackArgs& a_, unsigned chunk)
        : a(a_), k0((int)chunk * FOLD_KC), nk(min(FOLD_KC, a_.K - k0)) {
#pragma unroll
        for (int k = 0; k < FOLD_KC; ++k) {
            rho[k] = a.rho_primes[k0 + min(k, nk - 1)];
            acc[k] = 0.f;
        }
    }
    __device__ __forceinline__ void add(const float* r, float d1, float d2) {
        const float* col = r + R_COL;
        const float z1 = r[R_DEPTH], z2 = r[R_DEPTH + 1];
        const int flags = (int)r[R_FLAGS];
        const bool has1 = (flags & 1) != 0, has2 = (flags & 2) != 0;
#pragma unroll
        for (int k = 0; k < FOLD_KC; ++k) {
            if (k < nk) {
#pragma clang fp contract(off)
                const float s1 = has1 ? be::depth2sigma(a.dc, z1, rho[k]) : 1e-4f;       // as k_render_records writes R_RADF
                const float s2 = has2 ? be::depth2sigma(a.dc, z2, rho[k]) : 1e-4f;
                float u0, u1, u2;
                be::indicators(d1, d2, be::kRoot2 * s1, be::kRoot2 * s2, u0, u1, u2);
                blend_add(acc[k], col, u0, u1, u2);
            }
        }
    }
    template <bool ZERO = false>
    __device__ __forceinline__ void store(float n, size_t hw, size_t at) const {
#pragma unroll
        for (int k = 0; k < FOLD_KC; ++k) {
            if (k < nk) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.out[((size_t)(k0 + k) * 3 + c) * hw + at] = ZERO ? 0.f : acc[k][c] / n;
            }
        }
    }
    __device__ __forceinline__ void store_zero(size_t hw, size_t at) const { store<true>(0.f, hw, at); }
};

// ---- visit: one record at the patch-local position (px, py).  NOT under contract(off): wedge_dists never was.
template <class Acc>
__device__ __forceinline__ void visit_record(const float* rec, float px, float py, float w, Acc& acc) {
    const float4* rp = reinterpret_cast<const float4*>(rec);
    float r[REC];
#pragma unroll
    for (int k = 0; k < REC / 4; ++k) { const float4 t = rp[k]; r[4 * k] = t.x; r[4 * k + 1] = t.y; r[4 * k + 2] = t.z; r[4 * k + 3] = t.w; }
    be::WedgeGeom g;
    g.x0 = r[0]; g.y0 = r[1]; g.x1 = r[2]; g.y1 = r[3];
    g.s11 = r[4]; g.c11 = r[5]; g.s12 = r[6]; g.c12 = r[7]; g.s21 = r[8]; g.c21 = r[9]; g.s22 = r[10]; g.c22 = r[11];
    g.sg1 = r[12]; g.sg2 = r[13];
    float d1, d2;
    be::wedge_dists(g, px, py, w, d1, d2);
    acc.add(r, d1, d2);
}

// ---- run.  The record grid is a continuous description: wedge_dists, indicators, boundary_value and depth_mask take a real
// position.  A sample sits, per axis, at q + f pixels (Axis: q whole, 0 <= f < 1, r != 0 iff f > 0).  A grid line of origin oy
// covers it iff oy <= q + f <= oy + 20, i.e. iff q + (r != 0) - 20 <= oy <= q: integer arithmetic and a contiguous run of lines.
// The origins being whole pixels, r and f are the same for every covering line.  The patch-local coordinate is lin[q - oy]
// (READ, not computed) when r == 0 and lin[q - oy] + f * (lin[q - oy + 1] - lin[q - oy]) otherwise (then q - oy <= 19); a
// sample on a pixel therefore gets the pixel sampler's coordinate whatever sampler produced it.
struct Axis { int q, r; float f; };

__device__ __forceinline__ float lattice_coord(const float* lin, int q, int pr, float frac) {
#pragma clang fp contract(off)
    const float l0 = lin[q];
    if (pr == 0) return l0;                                     // an input pixel: lin[q + 1] is not read (q may be 20)
    return l0 + frac * (lin[q + 1] - l0);
}

// How a line index becomes an origin and a record row / column, and how the run [lo, hi] of lines with
// first <= origin <= last is found (hi < lo: none).
struct StagedLines {         // origin tables, the FOLD_LINES lines that can cover a tile staged in LDS; slot 0 is line `base`
    const int* s; int base;
    __device__ __forceinline__ int origin(int i) const { return s[i]; }
    __device__ __forceinline__ int line(int i) const { return base + i; }
    __device__ __forceinline__ void run(int first, int last, int& lo, int& hi) const {
        lo = 0; while (lo < FOLD_LINES && s[lo] < first) ++lo;
        hi = lo - 1; while (hi + 1 < FOLD_LINES && s[hi + 1] <= last) ++hi;
    }
};
struct TableLines {          // origin tables t[0..n) searched in global memory (samples that are not tiled)
    const int32_t* __restrict__ t; int n;
    __device__ __forceinline__ int origin(int i) const { return t[i]; }
    __device__ __forceinline__ int line(int i) const { return i; }
    __device__ __forceinline__ void run(int first, int last, int& lo, int& hi) const {
        lo = lower_bound(t, n, first);
        hi = lo - 1; while (hi + 1 < n && t[hi + 1] <= last) ++hi;
    }
};
struct StrideLines {         // the uniform grid of nn.Unfold: origin = stride * index, n lines
    int s, n;
    __device__ __forceinline__ int origin(int i) const { return s * i; }
    __device__ __forceinline__ int line(int i) const { return i; }
    __device__ __forceinline__ void run(int first, int last, int& lo, int& hi) const {
        lo = first > 0 ? (first + s - 1) / s : 0;
        hi = last / s; if (hi > n - 1) hi = n - 1;
    }
};

// visits the patches covering the sample (y, x), i outer, j inner, ascending (the order is part of the result); returns how many
template <class Lines, class Acc>
__device__ __forceinline__ int fold_run(const float* lin, float w, const FoldGrid& g, const Lines& ly, const Lines& lx, const Axis& y,
                                        const Axis& x, Acc& acc) {
    int i_lo, j_lo, i_hi, j_hi;
    ly.run(y.q + (y.r ? 1 : 0) - (R - 1), y.q, i_lo, i_hi);
    lx.run(x.q + (x.r ? 1 : 0) - (R - 1), x.q, j_lo, j_hi);
    int cnt = 0;
    for (int i = i_lo; i <= i_hi; ++i) {
        const float py = lattice_coord(lin, y.q - ly.origin(i), y.r, y.f);
        for (int j = j_lo; j <= j_hi; ++j) {
            const float px = lattice_coord(lin, x.q - lx.origin(j), x.r, x.f);
            visit_record(g.records + (size_t)(ly.line(i) * g.wp + lx.line(j)) * REC, px, py, w, acc);
            ++cnt;
        }
    }
    return cnt;
}

// ---- samplers
// What the two tiled samplers do before their threads part: lin -> LDS and, with origin tables, the grid lines that can cover
// the tile (the first is the first with origin >= first_y / first_x) staged once per workgroup; absent slots hold LINE_NONE.
// i0 / j0: the grid line held by sy[0] / sx[0].
template <bool TABLES>
__device__ __forceinline__ void stage_tile(const be_render_opts& o, const FoldGrid& g, int first_y, int first_x, float* lin, int* sy,
                                           int* sx, int& i0, int& j0) {
    const int t = threadIdx.x;
    if (t < R) lin[t] = o.lin[t];
    i0 = 0; j0 = 0;
    if constexpr (TABLES) {
        i0 = lower_bound(g.ys, g.hp, first_y);
        j0 = lower_bound(g.xs, g.wp, first_x);
        if (t < FOLD_LINES) sy[t] = i0 + t < g.hp ? g.ys[i0 + t] : LINE_NONE;
        else if (t >= 64 && t < 64 + FOLD_LINES) sx[t - 64] = j0 + t - 64 < g.wp ? g.xs[j0 + t - 64] : LINE_NONE;
    }
    __syncthreads();
}

// one tiled sample: fold the covering run into a fresh accumulator and store it
template <class Acc, bool TABLES>
__device__ __forceinline__ void fold_tile_sample(const be_render_opts& o, const typename Acc::Args& a, const float* lin, const int* sy,
                                                 const int* sx, int i0, int j0, const Axis& y, const Axis& x, size_t hw, size_t at) {
    Acc acc(o, a, blockIdx.z);
    int cnt;
    if constexpr (TABLES) cnt = fold_run(lin, o.w, a.g, StagedLines{sy, i0}, StagedLines{sx, j0}, y, x, acc);
    else cnt = fold_run(lin, o.w, a.g, StrideLines{a.g.stride, a.g.hp}, StrideLines{a.g.stride, a.g.wp}, y, x, acc);
    acc.store((float)cnt, hw, at);
}

// whole pixels: one thread per pixel of the H x W image ("owner computes": deterministic, no atomics).  blockIdx.z = image of
// a batch (MapsAcc) / plane chunk (StackAcc).  r == 0: lattice_coord returns lin[q], no division anywhere.
template <class Acc, bool TABLES>
__global__ __launch_bounds__(256)
void k_fold_pixels(be_render_opts o, typename Acc::Args a) {
    __shared__ float lin[R];
    __shared__ int sy[TABLES ? FOLD_LINES : 1], sx[TABLES ? FOLD_LINES : 1];
    int i0, j0;
    stage_tile<TABLES>(o, a.g, (int)blockIdx.y * FOLD_TILE - (R - 1), (int)blockIdx.x * FOLD_TILE - (R - 1), lin, sy, sx, i0, j0);
    const int x = blockIdx.x * FOLD_TILE + (threadIdx.x & 15);
    const int y = blockIdx.y * FOLD_TILE + (threadIdx.x >> 4);
    if (x >= a.g.W || y >= a.g.H) return;
    if constexpr (Acc::BATCHED) a.select_image(blockIdx.z);
    fold_tile_sample<Acc, TABLES>(o, a, lin, sy, sx, i0, j0, Axis{y, 0, 0.f}, Axis{x, 0, 0.f}, (size_t)a.g.H * a.g.W, (size_t)y * a.g.W + x);
}

// a lattice `scale` (k) times finer, over a window of the image: output sample (iy, ix) sits at Y = top * k + iy,
// X = left * k + ix in units of 1/k pixel; Y = yq * k + yr (0 <= yr < k) gives the Axis with f = yr / k - one division by k
// per thread and axis, not per patch.  Every k-th sample has r == 0 and equals the pixel sampler's pixel bit for bit.
struct Lattice {
    int scale;               // k, 1..16
    int top, left;           // window origin, input pixels
    int Ho, Wo;              // (h - 1) * k + 1, (w - 1) * k + 1
};

// first grid line a 16-sample tile starting at sample P0 (units of 1/k pixel) can be covered by; a tile spans at most 16
// pixels, so at most FOLD_LINES distinct origins lie in [tile_first, (P0 + 15) / k]
__device__ __forceinline__ int lattice_tile_first(int P0, int k) { return P0 / k + (P0 % k ? 1 : 0) - (R - 1); }

template <class Acc, bool TABLES>
__global__ __launch_bounds__(256)
void k_fold_lattice(be_render_opts o, typename Acc::Args a, Lattice l) {
    __shared__ float lin[R];
    __shared__ int sy[TABLES ? FOLD_LINES : 1], sx[TABLES ? FOLD_LINES : 1];
    const int k = l.scale;
    int i0, j0;
    stage_tile<TABLES>(o, a.g, lattice_tile_first(l.top * k + (int)blockIdx.y * FOLD_TILE, k),
                       lattice_tile_first(l.left * k + (int)blockIdx.x * FOLD_TILE, k), lin, sy, sx, i0, j0);
    const int ix = blockIdx.x * FOLD_TILE + (threadIdx.x & 15);
    const int iy = blockIdx.y * FOLD_TILE + (threadIdx.x >> 4);
    if (ix >= l.Wo || iy >= l.Ho) return;
    const int Y = l.top * k + iy, X = l.left * k + ix;
    const int yq = Y / k, yr = Y - yq * k, xq = X / k, xr = X - xq * k;
    fold_tile_sample<Acc, TABLES>(o, a, lin, sy, sx, i0, j0, Axis{yq, yr, (float)yr / (float)k}, Axis{xq, xr, (float)xr / (float)k},
                                  (size_t)l.Ho * l.Wo, (size_t)iy * l.Wo + ix);
}

// a list of N real-valued positions (y, x) in input-pixel coordinates (pixel centres at the integers, the coordinate
// top + iy / k of the lattice), one thread per point.  Per axis q = floor(y), f = y - q (exact in float32), r = (f > 0): a point
// with fy == fx == 0 equals the pixel sampler bit for bit and a dyadic point equals the lattice sampler bit for bit.  Points are
// not tiled: origin tables are searched in global memory (TableLines), not staged.  Outputs are channel-major over the points
// ([C,N]), so a point grid [Ho,Wo] reshapes to the lattice layout without a transpose.  A point outside the closed domain
// [0, H-1] x [0, W-1] (NaN included) gets 0 in every requested output.  blockIdx.y = plane chunk (StackAcc).
struct Points {
    const float* pts;        // [N,2] (y, x), device
    int64_t N;
};

// the point's position, split per axis; false (outside the closed domain, or not a number): the caller writes zeros
__device__ __forceinline__ bool point_split(const float* __restrict__ pts, int64_t p, int H, int W, Axis& ay, Axis& ax) {
    const float y = pts[2 * p], x = pts[2 * p + 1];
    if (!(y >= 0.f && y <= (float)(H - 1) && x >= 0.f && x <= (float)(W - 1))) return false;
    const int yq = (int)floorf(y), xq = (int)floorf(x);
    const float fy = y - (float)yq, fx = x - (float)xq;
    ay = Axis{yq, fy > 0.f, fy}; ax = Axis{xq, fx > 0.f, fx};
    return true;
}

template <class Acc, bool TABLES>
__global__ __launch_bounds__(256)
void k_fold_points(be_render_opts o, typename Acc::Args a, Points l) {
    __shared__ float lin[R];
    if (threadIdx.x < R) lin[threadIdx.x] = o.lin[threadIdx.x];
    __syncthreads();
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= l.N) return;
    Acc acc(o, a, blockIdx.y);
    Axis y, x;
    if (!point_split(l.pts, at, a.g.H, a.g.W, y, x)) { acc.store_zero((size_t)l.N, at); return; }
    int cnt;
    if constexpr (TABLES) cnt = fold_run(lin, o.w, a.g, TableLines{a.g.ys, a.g.hp}, TableLines{a.g.xs, a.g.wp}, y, x, acc);
    else cnt = fold_run(lin, o.w, a.g, StrideLines{a.g.stride, a.g.hp}, StrideLines{a.g.stride, a.g.wp}, y, x, acc);
    acc.store((float)cnt, (size_t)l.N, at);
}

// ------------------------------------------------------------------------------------------------ glue
__global__ void k_unfold(const float* __restrict__ img, float* __restrict__ out, int B, int C, int H, int W, int hp,
                         int wp, int stride) {
    const int64_t total = (int64_t)B * hp * wp * C * NPIX;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        int64_t t = idx;
        const int pix = (int)(t % NPIX); t /= NPIX;
        const int c = (int)(t % C); t /= C;
        const int j = (int)(t % wp); t /= wp;
        const int i = (int)(t % hp);
        const int64_t b = t / hp;
        const int r = pix / R, cc = pix - r * R;
        out[idx] = img[((b * C + c) * H + (stride * i + r)) * W + stride * j + cc];
    }
}

// blurry_edges_test.py:123-132: [2,P,10] CNN outputs + [2,P,9] colours -> normalised 38-feature rows
__global__ void k_local_features(const float* __restrict__ params10, const float* __restrict__ colors, float* __restrict__ pm,
                                 int64_t P) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * 38) return;
    const int64_t p = idx / 38;
    const int f = (int)(idx % 38);
    const int im = f / 19, k = f % 19;
    float v;
    if (k < 10) {
        const float q = params10[(im * P + p) * 10 + k];
        if (k < 4) v = q / 3.0f;
        else if (k < 8) v = (be::remainder_2pi(q) - be::kPi) / be::kPi;
        else v = q - 0.5f;
    } else {
        v = (colors[(im * P + p) * 9 + (k - 10)] - 0.5f) * 2.0f;
    }
    pm[idx] = v;
}

// blurry_edges_test.py:134-138: transformer output [P,12] -> wedge parameters
__global__ void k_global_denorm(const float* __restrict__ y, float* __restrict__ est, int64_t P) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * 12) return;
    const int k = (int)(idx % 12);
    const float v = y[idx];
    est[idx] = k < 4 ? v * 3.0f : (k < 8 ? be::remainder_2pi((v + 1.0f) * be::kPi) : v + 0.5f);
}

}  // namespace

extern "C" int be_render_full_f32(const be_render_opts* o, const be_depth_consts* dc, float rho_prime, int densify_w,
                                  const float* params12, const be_patch_view* view, float* records, float* patches,
                                  float* shpd, float* refoc, float* boundary, float* depth_map, int32_t* depth_mask,
                                  int64_t n, void* stream) {
    BE_REQUIRE(n >= 0, "be_render_full_f32: n < 0");
    if (n == 0) return BE_OK;
    BE_REQUIRE(o && dc && params12 && view && view->base && records, "be_render_full_f32: null pointer");
    BE_REQUIRE(view->wp > 0, "be_render_full_f32: view.wp must be > 0");
    BE_REQUIRE(be::aligned16(records), "be_render_full_f32: records must be 16-byte aligned");
    FullArgs a{params12, *view, records, patches, shpd, refoc, boundary, depth_map, depth_mask, rho_prime, densify_w, n,
               nullptr, nullptr, 0, 0};
    const int64_t blocks = (n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    BE_REQUIRE(blocks <= 0x7fffffff, "be_render_full_f32: n too large");
    hipLaunchKernelGGL(k_render_records<false>, dim3((unsigned)blocks), dim3(64 * WAVES_PER_BLOCK), 0, be::as_stream(stream),
                       *o, *dc, a);
    return be::check_launch("be_render_full_f32");
}

// ---- the fold entries.  Each checks its own arguments in its own order (BE_REQUIRE returns on the first failure, so the order
// decides which message a doubly-wrong call gets); what they share is below.

// the rule every fold entry ends its grid checks with: the grid lies in the image.  With origin tables the lines are distinct
// pixels whose patches fit (HP <= H-20, WP <= W-20); without, stride > 0 and the last patch ends inside the image.
static int check_fold_grid(const char* who, int HP, int WP, int H, int W, int stride, const int32_t* ys) {
    if (ys) {
        BE_REQUIRE(HP > 0 && WP > 0 && HP <= H - R + 1 && WP <= W - R + 1,
                   "%s: HP / WP must be in [1, H-20] / [1, W-20] (origins are distinct pixels)", who);
    } else {
        BE_REQUIRE(stride > 0, "%s: bad sizes", who);
        BE_REQUIRE((int64_t)stride * (HP - 1) + R <= H && (int64_t)stride * (WP - 1) + R <= W, "%s: patch grid exceeds the image", who);
    }
    return BE_OK;
}

static FoldGrid fold_grid(const float* records, int HP, int WP, int H, int W, int stride, const int32_t* ys, const int32_t* xs) {
    return FoldGrid{records, HP, WP, H, W, ys ? 0 : stride, ys, xs};
}

static dim3 tile_grid(int Wo, int Ho, int z = 1) { return dim3((Wo + FOLD_TILE - 1) / FOLD_TILE, (Ho + FOLD_TILE - 1) / FOLD_TILE, z); }
static int stack_chunks(int K) { return (K + FOLD_KC - 1) / FOLD_KC; }

template <class... P, class... A>
static int launch_fold(const char* who, void (*k)(P...), dim3 grid, void* stream, const A&... args) {
    hipLaunchKernelGGL(k, grid, dim3(256), 0, be::as_stream(stream), args...);
    return be::check_launch(who);
}
// an entry that takes either grid: the instantiation that matches it, kt with origin tables, ku without (uniform)
template <class... P, class... A>
static int launch_fold(const char* who, bool tables, void (*kt)(P...), void (*ku)(P...), dim3 grid, void* stream, const A&... args) {
    return launch_fold(who, tables ? kt : ku, grid, stream, args...);
}

extern "C" int be_fold_records_f32(const be_render_opts* o, const float* records, int hp, int wp, int H, int W,
                                   int stride, int densify_w, float* image, float* shpd, float* refoc, float* bndry,
                                   float* depth, float* conf, void* stream) {
    const char* who = "be_fold_records_f32";
    BE_REQUIRE(o && records, "%s: null pointer", who);
    BE_REQUIRE(hp > 0 && wp > 0 && H > 0 && W > 0, "%s: bad sizes", who);
    if (const int rc = check_fold_grid(who, hp, wp, H, W, stride, nullptr)) return rc;
    BE_REQUIRE(be::aligned16(records), "%s: records must be 16-byte aligned", who);
    const FoldArgs a{fold_grid(records, hp, wp, H, W, stride, nullptr, nullptr), densify_w, image, shpd, refoc, bndry, depth, conf, 0};
    return launch_fold(who, k_fold_pixels<MapsAcc, false>, tile_grid(W, H), stream, *o, a);
}

extern "C" int be_fold_records_batch_f32(const be_render_opts* o, const float* records, int B, int hp, int wp, int H, int W,
                                         int stride, int densify_w, float* image, float* shpd, float* refoc, float* bndry,
                                         float* depth, float* conf, void* stream) {
    const char* who = "be_fold_records_batch_f32";
    BE_REQUIRE(o && records, "%s: null pointer", who);
    BE_REQUIRE(B > 0 && B <= 65535 && hp > 0 && wp > 0 && H > 0 && W > 0, "%s: bad sizes", who);
    if (const int rc = check_fold_grid(who, hp, wp, H, W, stride, nullptr)) return rc;
    BE_REQUIRE(be::aligned16(records), "%s: records must be 16-byte aligned", who);
    const FoldArgs a{fold_grid(records, hp, wp, H, W, stride, nullptr, nullptr), densify_w, image, shpd, refoc, bndry, depth, conf,
                     (int64_t)hp * wp * REC};
    return launch_fold(who, k_fold_pixels<MapsAcc, false>, tile_grid(W, H, B), stream, *o, a);
}

extern "C" int be_render_full_grid_f32(const be_render_opts* o, const be_depth_consts* dc, float rho_prime, int densify_w,
                                       const float* params12, const float* img, int H, int W, const int32_t* ys,
                                       const int32_t* xs, int HP, int WP, float* records, void* stream) {
    BE_REQUIRE(o && dc && params12 && img && ys && xs && records, "be_render_full_grid_f32: null pointer");
    BE_REQUIRE(H >= R && W >= R, "be_render_full_grid_f32: the image is smaller than one patch");
    BE_REQUIRE(HP > 0 && WP > 0 && HP <= H - R + 1 && WP <= W - R + 1,
               "be_render_full_grid_f32: HP / WP must be in [1, H-20] / [1, W-20] (origins are distinct pixels)");
    BE_REQUIRE(be::aligned16(records), "be_render_full_grid_f32: records must be 16-byte aligned");
    const int64_t n = (int64_t)HP * WP, hw = (int64_t)H * W;
    const be_patch_view v{img, 3 * hw, hw, W, 1, 0, 0, WP};
    FullArgs a{params12, v, records, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rho_prime, densify_w, n,
               ys, xs, H - R, W - R};
    const int64_t blocks = (n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    BE_REQUIRE(blocks <= 0x7fffffff, "be_render_full_grid_f32: grid too large");
    hipLaunchKernelGGL(k_render_records<true>, dim3((unsigned)blocks), dim3(64 * WAVES_PER_BLOCK), 0, be::as_stream(stream),
                       *o, *dc, a);
    return be::check_launch("be_render_full_grid_f32");
}

extern "C" int be_fold_records_grid_f32(const be_render_opts* o, const float* records, int HP, int WP, int H, int W,
                                        const int32_t* ys, const int32_t* xs, int densify_w, float* image, float* shpd,
                                        float* refoc, float* bndry, float* depth, float* conf, void* stream) {
    const char* who = "be_fold_records_grid_f32";
    BE_REQUIRE(o && records && ys && xs, "%s: null pointer", who);
    BE_REQUIRE(H >= R && W >= R, "%s: the image is smaller than one patch", who);
    if (const int rc = check_fold_grid(who, HP, WP, H, W, 0, ys)) return rc;
    BE_REQUIRE((H + FOLD_TILE - 1) / FOLD_TILE <= 65535 && (int64_t)HP * WP <= 0x7fffffff, "%s: image too large", who);
    BE_REQUIRE(be::aligned16(records), "%s: records must be 16-byte aligned", who);
    const FoldArgs a{fold_grid(records, HP, WP, H, W, 0, ys, xs), densify_w, image, shpd, refoc, bndry, depth, conf, 0};
    return launch_fold(who, k_fold_pixels<MapsAcc, true>, tile_grid(W, H), stream, *o, a);
}

extern "C" int be_refocus_stack_chunk(void) { return FOLD_KC; }

extern "C" int be_fold_refocus_stack_f32(const be_render_opts* o, const be_depth_consts* dc, const float* records, int HP, int WP,
                                         int H, int W, int stride, const int32_t* ys, const int32_t* xs, const float* rho_primes,
                                         int K, float* out, void* stream) {
    const char* who = "be_fold_refocus_stack_f32";
    BE_REQUIRE(o && dc && records && rho_primes && out, "%s: null pointer", who);
    BE_REQUIRE((ys == nullptr) == (xs == nullptr), "%s: ys and xs must both be given (origin tables) or both be null (uniform grid)", who);
    BE_REQUIRE(K >= 1 && stack_chunks(K) <= 65535, "%s: K must be in [1, 65535 * BE_REFOCUS_STACK_KC]", who);
    BE_REQUIRE(HP > 0 && WP > 0 && H >= R && W >= R, "%s: bad sizes", who);
    BE_REQUIRE((H + FOLD_TILE - 1) / FOLD_TILE <= 65535 && (int64_t)HP * WP <= 0x7fffffff, "%s: image too large", who);
    BE_REQUIRE(be::aligned16(records), "%s: records must be 16-byte aligned", who);
    if (const int rc = check_fold_grid(who, HP, WP, H, W, stride, ys)) return rc;
    const StackArgs a{fold_grid(records, HP, WP, H, W, stride, ys, xs), *dc, rho_primes, out, K};
    return launch_fold(who, ys != nullptr, k_fold_pixels<StackAcc, true>, k_fold_pixels<StackAcc, false>,
                       tile_grid(W, H, stack_chunks(K)), stream, *o, a);
}

// the host checks the two lattice entries share: the grid (uniform or tables), the scale and the window -> the lattice
static int check_lattice(const char* who, int HP, int WP, int H, int W, int stride, const int32_t* ys, const int32_t* xs, int scale,
                         int top, int left, int h, int w, Lattice* l) {
    BE_REQUIRE((ys == nullptr) == (xs == nullptr), "%s: ys and xs must both be given (origin tables) or both be null (uniform grid)", who);
    BE_REQUIRE(scale >= 1 && scale <= BE_RENDER_AT_MAX_SCALE, "%s: scale must be in [1, %d], got %d", who, BE_RENDER_AT_MAX_SCALE, scale);
    BE_REQUIRE(HP > 0 && WP > 0 && H >= R && W >= R, "%s: bad sizes", who);
    BE_REQUIRE((int64_t)HP * WP <= 0x7fffffff && (int64_t)H * scale <= 0x7fffffff && (int64_t)W * scale <= 0x7fffffff,
               "%s: image too large (HP * WP, H * scale and W * scale must fit 31 bits)", who);
    BE_REQUIRE(top >= 0 && left >= 0 && h >= 1 && w >= 1 && (int64_t)top + h <= H && (int64_t)left + w <= W,
               "%s: window (%d, %d, %d, %d) leaves the %d x %d image", who, top, left, h, w, H, W);
    if (const int rc = check_fold_grid(who, HP, WP, H, W, stride, ys)) return rc;
    const int64_t Ho = (int64_t)(h - 1) * scale + 1, Wo = (int64_t)(w - 1) * scale + 1;
    BE_REQUIRE(Ho * Wo <= 0x7fffffff && (Ho + FOLD_TILE - 1) / FOLD_TILE <= 65535,
               "%s: lattice %lld x %lld too large (Ho * Wo must fit 31 bits, Ho <= 16 * 65535)", who, (long long)Ho, (long long)Wo);
    *l = Lattice{scale, top, left, (int)Ho, (int)Wo};
    return BE_OK;
}

extern "C" int be_fold_records_at_f32(const be_render_opts* o, const float* records, int HP, int WP, int H, int W, int stride,
                                      const int32_t* ys, const int32_t* xs, int scale, int top, int left, int h, int w,
                                      int densify_w, float* image, float* shpd, float* refoc, float* bndry, float* depth,
                                      float* conf, void* stream) {
    const char* who = "be_fold_records_at_f32";
    BE_REQUIRE(o && records, "%s: null pointer", who);
    BE_REQUIRE(be::aligned16(records), "%s: records must be 16-byte aligned", who);
    Lattice l;
    if (const int rc = check_lattice(who, HP, WP, H, W, stride, ys, xs, scale, top, left, h, w, &l)) return rc;
    const FoldArgs a{fold_grid(records, HP, WP, H, W, stride, ys, xs), densify_w, image, shpd, refoc, bndry, depth, conf, 0};
    return launch_fold(who, ys != nullptr, k_fold_lattice<MapsAcc, true>, k_fold_lattice<MapsAcc, false>, tile_grid(l.Wo, l.Ho), stream,
                       *o, a, l);
}

extern "C" int be_fold_refocus_stack_at_f32(const be_render_opts* o, const be_depth_consts* dc, const float* records, int HP, int WP,
                                            int H, int W, int stride, const int32_t* ys, const int32_t* xs, int scale, int top,
                                            int left, int h, int w, const float* rho_primes, int K, float* out, void* stream) {
    const char* who = "be_fold_refocus_stack_at_f32";
    BE_REQUIRE(o && dc && records && rho_primes && out, "%s: null pointer", who);
    BE_REQUIRE(be::aligned16(records), "%s: records must be 16-byte aligned", who);
    BE_REQUIRE(K >= 1 && stack_chunks(K) <= 65535, "%s: K must be in [1, 65535 * BE_REFOCUS_STACK_KC]", who);
    Lattice l;
    if (const int rc = check_lattice(who, HP, WP, H, W, stride, ys, xs, scale, top, left, h, w, &l)) return rc;
    const StackArgs a{fold_grid(records, HP, WP, H, W, stride, ys, xs), *dc, rho_primes, out, K};
    return launch_fold(who, ys != nullptr, k_fold_lattice<StackAcc, true>, k_fold_lattice<StackAcc, false>,
                       tile_grid(l.Wo, l.Ho, stack_chunks(K)), stream, *o, a, l);
}

// the host checks the two point entries share: the grid (uniform or tables) and the point list
constexpr int64_t POINTS_MAX = (int64_t)0x00ffffff * 256;      // workgroups * 256 threads stay below 2^32

static int check_points(const char* who, int HP, int WP, int H, int W, int stride, const int32_t* ys, const int32_t* xs,
                        const float* points, int64_t N) {
    BE_REQUIRE((ys == nullptr) == (xs == nullptr), "%s: ys and xs must both be given (origin tables) or both be null (uniform grid)", who);
    BE_REQUIRE(points, "%s: null pointer", who);
    BE_REQUIRE(HP > 0 && WP > 0 && H >= R && W >= R, "%s: bad sizes", who);
    BE_REQUIRE((int64_t)HP * WP <= 0x7fffffff && H <= (1 << 24) && W <= (1 << 24),
               "%s: image too large (HP * WP must fit 31 bits, H and W 24 bits: positions are float32)", who);
    BE_REQUIRE(N >= 1 && N <= POINTS_MAX, "%s: N must be in [1, %lld], got %lld", who, (long long)POINTS_MAX, (long long)N);
    return check_fold_grid(who, HP, WP, H, W, stride, ys);
}

extern "C" int be_fold_records_points_f32(const be_render_opts* o, const float* records, int HP, int WP, int H, int W, int stride,
                                          const int32_t* ys, const int32_t* xs, const float* points, int64_t N, int densify_w,
                                          float* image, float* shpd, float* refoc, float* bndry, float* depth, float* conf,
                                          void* stream) {
    const char* who = "be_fold_records_points_f32";
    BE_REQUIRE(o && records, "%s: null pointer", who);
    BE_REQUIRE(be::aligned16(records), "%s: records must be 16-byte aligned", who);
    if (const int rc = check_points(who, HP, WP, H, W, stride, ys, xs, points, N)) return rc;
    const FoldArgs a{fold_grid(records, HP, WP, H, W, stride, ys, xs), densify_w, image, shpd, refoc, bndry, depth, conf, 0};
    return launch_fold(who, ys != nullptr, k_fold_points<MapsAcc, true>, k_fold_points<MapsAcc, false>, dim3((unsigned)((N + 255) / 256)),
                       stream, *o, a, Points{points, N});
}

extern "C" int be_fold_refocus_stack_points_f32(const be_render_opts* o, const be_depth_consts* dc, const float* records, int HP, int WP,
                                                int H, int W, int stride, const int32_t* ys, const int32_t* xs, const float* points,
                                                int64_t N, const float* rho_primes, int K, float* out, void* stream) {
    const char* who = "be_fold_refocus_stack_points_f32";
    BE_REQUIRE(o && dc && records && rho_primes && out, "%s: null pointer", who);
    BE_REQUIRE(be::aligned16(records), "%s: records must be 16-byte aligned", who);
    BE_REQUIRE(K >= 1 && stack_chunks(K) <= 65535, "%s: K must be in [1, 65535 * BE_REFOCUS_STACK_KC]", who);
    if (const int rc = check_points(who, HP, WP, H, W, stride, ys, xs, points, N)) return rc;
    const StackArgs a{fold_grid(records, HP, WP, H, W, stride, ys, xs), *dc, rho_primes, out, K};
    return launch_fold(who, ys != nullptr, k_fold_points<StackAcc, true>, k_fold_points<StackAcc, false>,
                       dim3((unsigned)((N + 255) / 256), stack_chunks(K)), stream, *o, a, Points{points, N});
}

extern "C" int be_unfold_patches_f32(const float* img, float* out, int B, int C, int H, int W, int stride, void* stream) {
    BE_REQUIRE(img && out, "be_unfold_patches_f32: null pointer");
    BE_REQUIRE(B > 0 && C > 0 && H >= R && W >= R && stride > 0, "be_unfold_patches_f32: bad sizes");
    const int hp = (H - R) / stride + 1, wp = (W - R) / stride + 1;
    const int64_t total = (int64_t)B * hp * wp * C * NPIX;
    int64_t g = (total + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(k_unfold, dim3((unsigned)g), dim3(256), 0, be::as_stream(stream), img, out, B, C, H, W, hp, wp, stride);
    return be::check_launch("be_unfold_patches_f32");
}

extern "C" int be_local_features_f32(const float* params10, const float* colors, float* pm, int64_t P, void* stream) {
    BE_REQUIRE(P >= 0, "be_local_features_f32: P < 0");
    if (P == 0) return BE_OK;
    BE_REQUIRE(params10 && colors && pm, "be_local_features_f32: null pointer");
    hipLaunchKernelGGL(k_local_features, dim3((unsigned)((P * 38 + 255) / 256)), dim3(256), 0, be::as_stream(stream),
                       params10, colors, pm, P);
    return be::check_launch("be_local_features_f32");
}

extern "C" int be_global_denorm_f32(const float* y, float* est, int64_t P, void* stream) {
    BE_REQUIRE(P >= 0, "be_global_denorm_f32: P < 0");
    if (P == 0) return BE_OK;
    BE_REQUIRE(y && est, "be_global_denorm_f32: null pointer");
    hipLaunchKernelGGL(k_global_denorm, dim3((unsigned)((P * 12 + 255) / 256)), dim3(256), 0, be::as_stream(stream), y, est, P);
    return be::check_launch("be_global_denorm_f32");
}
