// Full render pass ("pass B") + owner-computes fold, gfx950.
//
// Replaces PostProcess.get_patches(colors_only=False) and the six nn.Fold aggregations of
// blurry_edges_test.py:36-79,93-99 / utils/postprocessing_loss.py:151-173 (and the per-block patch-tensor
// stitching of blurry_edges_test_big.py:166-189) with two kernels and NO per-patch tensors in HBM:
//
//   k_render_records   one wavefront per patch position: both aperture images are read once (gather-on-read
//                      through a strided patch view: an image pair, an unfolded tensor or flat patches),
//                      the 882-row ridge system is reduced with wave shuffles, solved in fp64, the two
//                      wedge depths come from etas2depth, the refocus radii from depth2sigma and a wave
//                      ballot of the depth mask; result = one 128-byte record per patch.
//   k_fold_records     one thread per output pixel ("owner computes"): walks the <= 11x11 patches that
//                      cover the pixel in a fixed order, re-evaluates the wedges from the record for the four
//                      blur sets (aperture 1, aperture 2, sharpened, refocused) and accumulates the six maps.
//                      Deterministic (no atomics), divides by the analytic overlap count.
//
// Both kernels are templated on how a patch's origin is obtained: UNIFORM (origin = stride * index, the grid of
// nn.Unfold) or ORIGIN TABLES ys[HP] / xs[WP] (a separable grid whose last line may sit flush with the image edge, so an
// image of any size is covered; the fold then divides by the number of patches it visited).  The uniform instantiation
// is the code path every existing entry point takes.
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
struct FoldArgs {
    const float* records;    // [Hp*Wp,32]
    int hp, wp, H, W, stride;
    int densify_w;
    float* image;            // [2,3,H,W] or null
    float* shpd;             // [3,H,W] or null
    float* refoc;            // [3,H,W] or null
    float* bndry;            // [H,W] or null
    float* depth;            // [H,W] or null
    float* conf;             // [H,W] or null
    int64_t rec_stride;      // batched form (grid.z = image): floats between the records / maps of consecutive images
    const int32_t* ys;       // [hp] / [wp] patch origins, strictly increasing (k_fold_records<true> only)
    const int32_t* xs;
};

constexpr int FOLD_TILE = 16;                       // output pixels per workgroup and axis
constexpr int FOLD_LINES = FOLD_TILE + R - 1;       // strictly increasing integer origins: at most one grid line per pixel
                                                    // of [tile_first - (R-1), tile_last] can cover a pixel of the tile
constexpr int LINE_NONE = 0x7fffffff;

// first index in t[0..n) with t[i] >= v (t increasing)
__device__ __forceinline__ int lower_bound(const int32_t* __restrict__ t, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (t[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

template <bool TABLES>
__global__ __launch_bounds__(256)
void k_fold_records(be_render_opts o, FoldArgs a) {
    __shared__ float lin[R];
    __shared__ int sy[TABLES ? FOLD_LINES : 1], sx[TABLES ? FOLD_LINES : 1];
    if (threadIdx.x < R) lin[threadIdx.x] = o.lin[threadIdx.x];
    int i0 = 0, j0 = 0;                                         // grid line held by sy[0] / sx[0]
    if constexpr (TABLES) {
        // the grid lines that can cover this tile, staged once per workgroup; absent slots hold LINE_NONE
        i0 = lower_bound(a.ys, a.hp, (int)blockIdx.y * FOLD_TILE - (R - 1));
        j0 = lower_bound(a.xs, a.wp, (int)blockIdx.x * FOLD_TILE - (R - 1));
        const int t = threadIdx.x;
        if (t < FOLD_LINES) sy[t] = i0 + t < a.hp ? a.ys[i0 + t] : LINE_NONE;
        else if (t >= 64 && t < 64 + FOLD_LINES) sx[t - 64] = j0 + t - 64 < a.wp ? a.xs[j0 + t - 64] : LINE_NONE;
    }
    __syncthreads();
    const int x = blockIdx.x * FOLD_TILE + (threadIdx.x & 15);
    const int y = blockIdx.y * FOLD_TILE + (threadIdx.x >> 4);
    if (x >= a.W || y >= a.H) return;
    if (blockIdx.z) {                                           // image blockIdx.z of a batch
        const size_t b = blockIdx.z, hw = (size_t)a.H * a.W;
        a.records += b * a.rec_stride;
        if (a.image) a.image += b * 6 * hw;
        if (a.shpd) a.shpd += b * 3 * hw;
        if (a.refoc) a.refoc += b * 3 * hw;
        if (a.bndry) a.bndry += b * hw;
        if (a.depth) a.depth += b * hw;
        if (a.conf) a.conf += b * hw;
    }
    // patches covering (y,x): origin(i) <= y <= origin(i) + 20, a contiguous run of grid lines on either axis
    const int s = a.stride;
    int i_lo, j_lo, i_hi, j_hi;
    if constexpr (TABLES) {
        i_lo = 0; while (i_lo < FOLD_LINES && sy[i_lo] < y - (R - 1)) ++i_lo;
        j_lo = 0; while (j_lo < FOLD_LINES && sx[j_lo] < x - (R - 1)) ++j_lo;
        i_hi = i_lo - 1; while (i_hi + 1 < FOLD_LINES && sy[i_hi + 1] <= y) ++i_hi;
        j_hi = j_lo - 1; while (j_hi + 1 < FOLD_LINES && sx[j_hi + 1] <= x) ++j_hi;
    } else {
        i_lo = (y - (R - 1) + s - 1) / s; if (y - (R - 1) < 0) i_lo = 0;
        j_lo = (x - (R - 1) + s - 1) / s; if (x - (R - 1) < 0) j_lo = 0;
        i_hi = y / s; if (i_hi > a.hp - 1) i_hi = a.hp - 1;
        j_hi = x / s; if (j_hi > a.wp - 1) j_hi = a.wp - 1;
    }
    float acc1[3] = {0, 0, 0}, acc2[3] = {0, 0, 0}, accs[3] = {0, 0, 0}, accf[3] = {0, 0, 0};
    float accb = 0.f, accz = 0.f;
    int cnt = 0, cntz = 0;
    const float rs = be::kRoot2 * 1e-4f;
    for (int i = i_lo; i <= i_hi; ++i) {
        const float py = lin[y - (TABLES ? sy[i] : s * i)];
        for (int j = j_lo; j <= j_hi; ++j) {
            const float px = lin[x - (TABLES ? sx[j] : s * j)];
            const float4* rp = reinterpret_cast<const float4*>(a.records + (size_t)((i0 + i) * a.wp + (j0 + j)) * REC);
            float r[REC];
#pragma unroll
            for (int k = 0; k < REC / 4; ++k) { const float4 t = rp[k]; r[4 * k] = t.x; r[4 * k + 1] = t.y; r[4 * k + 2] = t.z; r[4 * k + 3] = t.w; }
            be::WedgeGeom g;
            g.x0 = r[0]; g.y0 = r[1]; g.x1 = r[2]; g.y1 = r[3];
            g.s11 = r[4]; g.c11 = r[5]; g.s12 = r[6]; g.c12 = r[7]; g.s21 = r[8]; g.c21 = r[9]; g.s22 = r[10]; g.c22 = r[11];
            g.sg1 = r[12]; g.sg2 = r[13];
            float d1, d2;
            be::wedge_dists(g, px, py, o.w, d1, d2);
            const float* col = r + R_COL;
            float u0, u1, u2;
            {
#pragma clang fp contract(off)
                if (a.image) {
                    be::indicators(d1, d2, r[R_RAD1], r[R_RAD1 + 1], u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc1[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                    be::indicators(d1, d2, r[R_RAD2], r[R_RAD2 + 1], u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc2[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
                if (a.shpd) {
                    be::indicators(d1, d2, rs, rs, u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) accs[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
                if (a.refoc) {
                    be::indicators(d1, d2, r[R_RADF], r[R_RADF + 1], u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) accf[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
                if (a.bndry) accb += be::boundary_value(d1, d2, o.delta_sq);
                if (a.depth || a.conf) {
                    const int m = be::depth_mask(d1, d2, o.delta_sq, a.densify_w != 0);
                    if (m == 1) { accz += r[R_DEPTH]; ++cntz; }
                    else if (m == 2) { accz += r[R_DEPTH + 1]; ++cntz; }
                }
            }
            ++cnt;
        }
    }
    const size_t hw = (size_t)a.H * a.W, at = (size_t)y * a.W + x;
    const float n = (float)cnt;                         // = nn.Fold(ones) at this pixel (>= 1): the patches visited
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (a.image) { a.image[c * hw + at] = acc1[c] / n; a.image[(3 + c) * hw + at] = acc2[c] / n; }
        if (a.shpd) a.shpd[c * hw + at] = accs[c] / n;
        if (a.refoc) a.refoc[c * hw + at] = accf[c] / n;
    }
    if (a.bndry) a.bndry[at] = accb / n;
    if (a.depth) a.depth[at] = accz / (cntz > 0 ? (float)cntz : 1.0f);      // postprocessing_loss.py:170-172
    if (a.conf) a.conf[at] = (float)cntz / n;
}

// ------------------------------------------------------------------------------------------------ focal stack
// K refocused images from ONE record grid: the refocus radius of a wedge is sqrt(2) * depth2sigma(z, rho') (or sqrt(2) * 1e-4
// when the wedge owns no mask pixel), a function of the record's R_DEPTH / R_FLAGS and the plane's optical power alone, so the
// record fetch, wedge_dists and the run search of k_fold_records are done once per covering patch and shared by the planes of a
// chunk.  Plane k is k_render_records(rho_prime = rho_k) + k_fold_records(refoc) bit for bit: same radius expression, same
// indicators / composite under contract(off), same visiting order, one division by the number of patches visited.
struct StackArgs {
    const float* records;    // [hp*wp,32]
    const float* rho_primes; // [K] optical powers, device
    float* out;              // [K,3,H,W]
    int hp, wp, H, W, stride, K;
    const int32_t* ys;       // [hp] / [wp] patch origins (k_fold_refocus_stack<true> only)
    const int32_t* xs;
};

constexpr int FOLD_KC = BE_REFOCUS_STACK_KC;        // planes per workgroup (blockIdx.z = chunk; the last chunk may be short)

template <bool TABLES>
__global__ __launch_bounds__(256)
void k_fold_refocus_stack(be_render_opts o, be_depth_consts dc, StackArgs a) {
    __shared__ float lin[R];
    __shared__ int sy[TABLES ? FOLD_LINES : 1], sx[TABLES ? FOLD_LINES : 1];
    if (threadIdx.x < R) lin[threadIdx.x] = o.lin[threadIdx.x];
    int i0 = 0, j0 = 0;                                         // grid line held by sy[0] / sx[0]
    if constexpr (TABLES) {
        i0 = lower_bound(a.ys, a.hp, (int)blockIdx.y * FOLD_TILE - (R - 1));
        j0 = lower_bound(a.xs, a.wp, (int)blockIdx.x * FOLD_TILE - (R - 1));
        const int t = threadIdx.x;
        if (t < FOLD_LINES) sy[t] = i0 + t < a.hp ? a.ys[i0 + t] : LINE_NONE;
        else if (t >= 64 && t < 64 + FOLD_LINES) sx[t - 64] = j0 + t - 64 < a.wp ? a.xs[j0 + t - 64] : LINE_NONE;
    }
    __syncthreads();
    const int x = blockIdx.x * FOLD_TILE + (threadIdx.x & 15);
    const int y = blockIdx.y * FOLD_TILE + (threadIdx.x >> 4);
    if (x >= a.W || y >= a.H) return;
    const int k0 = blockIdx.z * FOLD_KC;
    const int nk = min(FOLD_KC, a.K - k0);                      // planes of this chunk (uniform over the workgroup)
    float rho[FOLD_KC];
#pragma unroll
    for (int k = 0; k < FOLD_KC; ++k) rho[k] = a.rho_primes[k0 + min(k, nk - 1)];
    const int s = a.stride;
    int i_lo, j_lo, i_hi, j_hi;
    if constexpr (TABLES) {
        i_lo = 0; while (i_lo < FOLD_LINES && sy[i_lo] < y - (R - 1)) ++i_lo;
        j_lo = 0; while (j_lo < FOLD_LINES && sx[j_lo] < x - (R - 1)) ++j_lo;
        i_hi = i_lo - 1; while (i_hi + 1 < FOLD_LINES && sy[i_hi + 1] <= y) ++i_hi;
        j_hi = j_lo - 1; while (j_hi + 1 < FOLD_LINES && sx[j_hi + 1] <= x) ++j_hi;
    } else {
        i_lo = (y - (R - 1) + s - 1) / s; if (y - (R - 1) < 0) i_lo = 0;
        j_lo = (x - (R - 1) + s - 1) / s; if (x - (R - 1) < 0) j_lo = 0;
        i_hi = y / s; if (i_hi > a.hp - 1) i_hi = a.hp - 1;
        j_hi = x / s; if (j_hi > a.wp - 1) j_hi = a.wp - 1;
    }
    float acc[FOLD_KC][3];
#pragma unroll
    for (int k = 0; k < FOLD_KC; ++k) { acc[k][0] = 0.f; acc[k][1] = 0.f; acc[k][2] = 0.f; }
    int cnt = 0;
    for (int i = i_lo; i <= i_hi; ++i) {
        const float py = lin[y - (TABLES ? sy[i] : s * i)];
        for (int j = j_lo; j <= j_hi; ++j) {
            const float px = lin[x - (TABLES ? sx[j] : s * j)];
            const float4* rp = reinterpret_cast<const float4*>(a.records + (size_t)((i0 + i) * a.wp + (j0 + j)) * REC);
            float r[REC];
#pragma unroll
            for (int k = 0; k < REC / 4; ++k) { const float4 t = rp[k]; r[4 * k] = t.x; r[4 * k + 1] = t.y; r[4 * k + 2] = t.z; r[4 * k + 3] = t.w; }
            be::WedgeGeom g;
            g.x0 = r[0]; g.y0 = r[1]; g.x1 = r[2]; g.y1 = r[3];
            g.s11 = r[4]; g.c11 = r[5]; g.s12 = r[6]; g.c12 = r[7]; g.s21 = r[8]; g.c21 = r[9]; g.s22 = r[10]; g.c22 = r[11];
            g.sg1 = r[12]; g.sg2 = r[13];
            float d1, d2;
            be::wedge_dists(g, px, py, o.w, d1, d2);
            const float* col = r + R_COL;
            const float z1 = r[R_DEPTH], z2 = r[R_DEPTH + 1];
            const int flags = (int)r[R_FLAGS];
            const bool has1 = (flags & 1) != 0, has2 = (flags & 2) != 0;
#pragma unroll
            for (int k = 0; k < FOLD_KC; ++k) {
                if (k < nk) {
#pragma clang fp contract(off)
                    const float s1 = has1 ? be::depth2sigma(dc, z1, rho[k]) : 1e-4f;       // as k_render_records writes R_RADF
                    const float s2 = has2 ? be::depth2sigma(dc, z2, rho[k]) : 1e-4f;
                    float u0, u1, u2;
                    be::indicators(d1, d2, be::kRoot2 * s1, be::kRoot2 * s2, u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[k][c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
            }
            ++cnt;
        }
    }
    const size_t hw = (size_t)a.H * a.W, at = (size_t)y * a.W + x;
    const float n = (float)cnt;
#pragma unroll
    for (int k = 0; k < FOLD_KC; ++k) {
        if (k < nk) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.out[((size_t)(k0 + k) * 3 + c) * hw + at] = acc[k][c] / n;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the folds on a finer lattice
// The record grid is a continuous description: wedge_dists, indicators, boundary_value and depth_mask take a real position.
// The two kernels below are k_fold_records and k_fold_refocus_stack evaluated on a lattice `scale` (k) times finer, over a
// window of the image: output sample (iy, ix) sits at Y = top * k + iy, X = left * k + ix in units of 1/k pixel.  With
// Y = yq * k + yr (0 <= yr < k) a grid line of origin oy covers the sample iff oy * k <= Y <= (oy + 20) * k, i.e. iff
// yq + (yr > 0) - 20 <= oy <= yq: integer arithmetic, a contiguous run of lines, and - the origins being whole pixels - the
// remainder yr is the same for every covering line, so the one division by k is per thread and axis, not per patch.  The
// patch-local coordinate is lin[q] (q = yq - oy, READ, not computed) when yr == 0 and lin[q] + (yr / k) * (lin[q+1] - lin[q])
// otherwise (then q <= 19).  Everything after the coordinate is the body of the integer-pixel kernel, so every k-th sample
// equals that kernel's pixel bit for bit.
struct Lattice {
    int scale;               // k, 1..16
    int top, left;           // window origin, input pixels
    int Ho, Wo;              // (h - 1) * k + 1, (w - 1) * k + 1
};

// the run of grid lines covering a sample at pq + pr / k: staged origins sl[0..FOLD_LINES) (TABLES) or stride * index
template <bool TABLES>
__device__ __forceinline__ void lattice_run(const int* sl, int s, int n, int pq, int pr, int& lo, int& hi) {
    const int first = pq + (pr ? 1 : 0) - (R - 1);              // the smallest origin that still covers the sample
    if constexpr (TABLES) {
        lo = 0; while (lo < FOLD_LINES && sl[lo] < first) ++lo;
        hi = lo - 1; while (hi + 1 < FOLD_LINES && sl[hi + 1] <= pq) ++hi;
    } else {
        lo = first > 0 ? (first + s - 1) / s : 0;
        hi = pq / s; if (hi > n - 1) hi = n - 1;
    }
}

// first grid line a 16-sample tile starting at sample P0 (units of 1/k pixel) can be covered by
__device__ __forceinline__ int lattice_tile_first(int P0, int k) { return P0 / k + (P0 % k ? 1 : 0) - (R - 1); }

__device__ __forceinline__ float lattice_coord(const float* lin, int q, int pr, float frac) {
#pragma clang fp contract(off)
    const float l0 = lin[q];
    if (pr == 0) return l0;                                     // an input pixel: lin[q + 1] is not read (q may be 20)
    return l0 + frac * (lin[q + 1] - l0);
}

template <bool TABLES>
__global__ __launch_bounds__(256)
void k_fold_records_at(be_render_opts o, FoldArgs a, Lattice l) {
    __shared__ float lin[R];
    __shared__ int sy[TABLES ? FOLD_LINES : 1], sx[TABLES ? FOLD_LINES : 1];
    if (threadIdx.x < R) lin[threadIdx.x] = o.lin[threadIdx.x];
    const int k = l.scale;
    const int Y0 = l.top * k + (int)blockIdx.y * FOLD_TILE, X0 = l.left * k + (int)blockIdx.x * FOLD_TILE;
    int i0 = 0, j0 = 0;                                         // grid line held by sy[0] / sx[0]
    if constexpr (TABLES) {
        // a tile spans at most 16 pixels, so at most FOLD_LINES distinct origins lie in [tile_first, (P0 + 15) / k]
        i0 = lower_bound(a.ys, a.hp, lattice_tile_first(Y0, k));
        j0 = lower_bound(a.xs, a.wp, lattice_tile_first(X0, k));
        const int t = threadIdx.x;
        if (t < FOLD_LINES) sy[t] = i0 + t < a.hp ? a.ys[i0 + t] : LINE_NONE;
        else if (t >= 64 && t < 64 + FOLD_LINES) sx[t - 64] = j0 + t - 64 < a.wp ? a.xs[j0 + t - 64] : LINE_NONE;
    }
    __syncthreads();
    const int ix = blockIdx.x * FOLD_TILE + (threadIdx.x & 15);
    const int iy = blockIdx.y * FOLD_TILE + (threadIdx.x >> 4);
    if (ix >= l.Wo || iy >= l.Ho) return;
    const int Y = l.top * k + iy, X = l.left * k + ix;
    const int yq = Y / k, yr = Y - yq * k, xq = X / k, xr = X - xq * k;
    const float fy = (float)yr / (float)k, fx = (float)xr / (float)k;
    const int s = a.stride;
    int i_lo, j_lo, i_hi, j_hi;
    lattice_run<TABLES>(sy, s, a.hp, yq, yr, i_lo, i_hi);
    lattice_run<TABLES>(sx, s, a.wp, xq, xr, j_lo, j_hi);
    float acc1[3] = {0, 0, 0}, acc2[3] = {0, 0, 0}, accs[3] = {0, 0, 0}, accf[3] = {0, 0, 0};
    float accb = 0.f, accz = 0.f;
    int cnt = 0, cntz = 0;
    const float rs = be::kRoot2 * 1e-4f;
    for (int i = i_lo; i <= i_hi; ++i) {
        const float py = lattice_coord(lin, yq - (TABLES ? sy[i] : s * i), yr, fy);
        for (int j = j_lo; j <= j_hi; ++j) {
            const float px = lattice_coord(lin, xq - (TABLES ? sx[j] : s * j), xr, fx);
            const float4* rp = reinterpret_cast<const float4*>(a.records + (size_t)((i0 + i) * a.wp + (j0 + j)) * REC);
            float r[REC];
#pragma unroll
            for (int q = 0; q < REC / 4; ++q) { const float4 t = rp[q]; r[4 * q] = t.x; r[4 * q + 1] = t.y; r[4 * q + 2] = t.z; r[4 * q + 3] = t.w; }
            be::WedgeGeom g;
            g.x0 = r[0]; g.y0 = r[1]; g.x1 = r[2]; g.y1 = r[3];
            g.s11 = r[4]; g.c11 = r[5]; g.s12 = r[6]; g.c12 = r[7]; g.s21 = r[8]; g.c21 = r[9]; g.s22 = r[10]; g.c22 = r[11];
            g.sg1 = r[12]; g.sg2 = r[13];
            float d1, d2;
            be::wedge_dists(g, px, py, o.w, d1, d2);
            const float* col = r + R_COL;
            float u0, u1, u2;
            {
#pragma clang fp contract(off)
                if (a.image) {
                    be::indicators(d1, d2, r[R_RAD1], r[R_RAD1 + 1], u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc1[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                    be::indicators(d1, d2, r[R_RAD2], r[R_RAD2 + 1], u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc2[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
                if (a.shpd) {
                    be::indicators(d1, d2, rs, rs, u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) accs[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
                if (a.refoc) {
                    be::indicators(d1, d2, r[R_RADF], r[R_RADF + 1], u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) accf[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
                if (a.bndry) accb += be::boundary_value(d1, d2, o.delta_sq);
                if (a.depth || a.conf) {
                    const int m = be::depth_mask(d1, d2, o.delta_sq, a.densify_w != 0);
                    if (m == 1) { accz += r[R_DEPTH]; ++cntz; }
                    else if (m == 2) { accz += r[R_DEPTH + 1]; ++cntz; }
                }
            }
            ++cnt;
        }
    }
    const size_t hw = (size_t)l.Ho * l.Wo, at = (size_t)iy * l.Wo + ix;
    const float n = (float)cnt;                         // the patches visited (0 only where a uniform grid stops short of the edge)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (a.image) { a.image[c * hw + at] = acc1[c] / n; a.image[(3 + c) * hw + at] = acc2[c] / n; }
        if (a.shpd) a.shpd[c * hw + at] = accs[c] / n;
        if (a.refoc) a.refoc[c * hw + at] = accf[c] / n;
    }
    if (a.bndry) a.bndry[at] = accb / n;
    if (a.depth) a.depth[at] = accz / (cntz > 0 ? (float)cntz : 1.0f);
    if (a.conf) a.conf[at] = (float)cntz / n;
}

template <bool TABLES>
__global__ __launch_bounds__(256)
void k_fold_refocus_stack_at(be_render_opts o, be_depth_consts dc, StackArgs a, Lattice l) {
    __shared__ float lin[R];
    __shared__ int sy[TABLES ? FOLD_LINES : 1], sx[TABLES ? FOLD_LINES : 1];
    if (threadIdx.x < R) lin[threadIdx.x] = o.lin[threadIdx.x];
    const int sc = l.scale;
    const int Y0 = l.top * sc + (int)blockIdx.y * FOLD_TILE, X0 = l.left * sc + (int)blockIdx.x * FOLD_TILE;
    int i0 = 0, j0 = 0;
    if constexpr (TABLES) {
        i0 = lower_bound(a.ys, a.hp, lattice_tile_first(Y0, sc));
        j0 = lower_bound(a.xs, a.wp, lattice_tile_first(X0, sc));
        const int t = threadIdx.x;
        if (t < FOLD_LINES) sy[t] = i0 + t < a.hp ? a.ys[i0 + t] : LINE_NONE;
        else if (t >= 64 && t < 64 + FOLD_LINES) sx[t - 64] = j0 + t - 64 < a.wp ? a.xs[j0 + t - 64] : LINE_NONE;
    }
    __syncthreads();
    const int ix = blockIdx.x * FOLD_TILE + (threadIdx.x & 15);
    const int iy = blockIdx.y * FOLD_TILE + (threadIdx.x >> 4);
    if (ix >= l.Wo || iy >= l.Ho) return;
    const int Y = l.top * sc + iy, X = l.left * sc + ix;
    const int yq = Y / sc, yr = Y - yq * sc, xq = X / sc, xr = X - xq * sc;
    const float fy = (float)yr / (float)sc, fx = (float)xr / (float)sc;
    const int k0 = blockIdx.z * FOLD_KC;
    const int nk = min(FOLD_KC, a.K - k0);                      // planes of this chunk (uniform over the workgroup)
    float rho[FOLD_KC];
#pragma unroll
    for (int k = 0; k < FOLD_KC; ++k) rho[k] = a.rho_primes[k0 + min(k, nk - 1)];
    const int s = a.stride;
    int i_lo, j_lo, i_hi, j_hi;
    lattice_run<TABLES>(sy, s, a.hp, yq, yr, i_lo, i_hi);
    lattice_run<TABLES>(sx, s, a.wp, xq, xr, j_lo, j_hi);
    float acc[FOLD_KC][3];
#pragma unroll
    for (int k = 0; k < FOLD_KC; ++k) { acc[k][0] = 0.f; acc[k][1] = 0.f; acc[k][2] = 0.f; }
    int cnt = 0;
    for (int i = i_lo; i <= i_hi; ++i) {
        const float py = lattice_coord(lin, yq - (TABLES ? sy[i] : s * i), yr, fy);
        for (int j = j_lo; j <= j_hi; ++j) {
            const float px = lattice_coord(lin, xq - (TABLES ? sx[j] : s * j), xr, fx);
            const float4* rp = reinterpret_cast<const float4*>(a.records + (size_t)((i0 + i) * a.wp + (j0 + j)) * REC);
            float r[REC];
#pragma unroll
            for (int q = 0; q < REC / 4; ++q) { const float4 t = rp[q]; r[4 * q] = t.x; r[4 * q + 1] = t.y; r[4 * q + 2] = t.z; r[4 * q + 3] = t.w; }
            be::WedgeGeom g;
            g.x0 = r[0]; g.y0 = r[1]; g.x1 = r[2]; g.y1 = r[3];
            g.s11 = r[4]; g.c11 = r[5]; g.s12 = r[6]; g.c12 = r[7]; g.s21 = r[8]; g.c21 = r[9]; g.s22 = r[10]; g.c22 = r[11];
            g.sg1 = r[12]; g.sg2 = r[13];
            float d1, d2;
            be::wedge_dists(g, px, py, o.w, d1, d2);
            const float* col = r + R_COL;
            const float z1 = r[R_DEPTH], z2 = r[R_DEPTH + 1];
            const int flags = (int)r[R_FLAGS];
            const bool has1 = (flags & 1) != 0, has2 = (flags & 2) != 0;
#pragma unroll
            for (int k = 0; k < FOLD_KC; ++k) {
                if (k < nk) {
#pragma clang fp contract(off)
                    const float s1 = has1 ? be::depth2sigma(dc, z1, rho[k]) : 1e-4f;       // as k_render_records writes R_RADF
                    const float s2 = has2 ? be::depth2sigma(dc, z2, rho[k]) : 1e-4f;
                    float u0, u1, u2;
                    be::indicators(d1, d2, be::kRoot2 * s1, be::kRoot2 * s2, u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[k][c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
            }
            ++cnt;
        }
    }
    const size_t hw = (size_t)l.Ho * l.Wo, at = (size_t)iy * l.Wo + ix;
    const float n = (float)cnt;
#pragma unroll
    for (int k = 0; k < FOLD_KC; ++k) {
        if (k < nk) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.out[((size_t)(k0 + k) * 3 + c) * hw + at] = acc[k][c] / n;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the folds at arbitrary positions
// The lattice kernels above sample on an axis-aligned lattice with an integer scale; nothing after the coordinate needs that.
// The two kernels below take a list of N real-valued positions (y, x) in input-pixel coordinates (pixel centres at the integers,
// the coordinate top + iy / k of the lattice), one thread per point.  Per axis yq = floor(y), fy = y - yq (exact in float32); a
// grid line of origin oy covers the point iff oy <= y <= oy + 20, i.e. iff yq + (fy > 0) - 20 <= oy <= yq: the lattice rule
// with `yr > 0` replaced by `fy > 0`.  The coordinate is lattice_coord, so a point with fy == fx == 0 equals the pixel kernels
// bit for bit and a dyadic point equals the lattice kernels bit for bit.  Points are not tiled: origin tables are searched in
// global memory (lower_bound, then a forward scan), not staged.  Outputs are channel-major over the points ([C,N]), so a point
// grid [Ho,Wo] reshapes to the lattice layout without a transpose.  A point outside the closed domain [0, H-1] x [0, W-1]
// (NaN included) gets 0 in every requested output.
struct Points {
    const float* pts;        // [N,2] (y, x), device
    int64_t N;
};

// the run of grid lines covering a position pq + f (0 <= f < 1): the global origin table t[0..n) (TABLES) or stride * index
template <bool TABLES>
__device__ __forceinline__ void point_run(const int32_t* __restrict__ t, int s, int n, int pq, bool frac, int& lo, int& hi) {
    const int first = pq + (frac ? 1 : 0) - (R - 1);            // the smallest origin that still covers the position
    if constexpr (TABLES) {
        lo = lower_bound(t, n, first);
        hi = lo - 1; while (hi + 1 < n && t[hi + 1] <= pq) ++hi;
    } else {
        lo = first > 0 ? (first + s - 1) / s : 0;
        hi = pq / s; if (hi > n - 1) hi = n - 1;
    }
}

// the point's position, split per axis; false (outside the closed domain, or not a number): the caller writes zeros
__device__ __forceinline__ bool point_split(const float* __restrict__ pts, int64_t p, int H, int W, int& yq, int& xq, float& fy, float& fx) {
    const float y = pts[2 * p], x = pts[2 * p + 1];
    if (!(y >= 0.f && y <= (float)(H - 1) && x >= 0.f && x <= (float)(W - 1))) return false;
    yq = (int)floorf(y); xq = (int)floorf(x);
    fy = y - (float)yq; fx = x - (float)xq;
    return true;
}

template <bool TABLES>
__global__ __launch_bounds__(256)
void k_fold_records_points(be_render_opts o, FoldArgs a, Points l) {
    __shared__ float lin[R];
    if (threadIdx.x < R) lin[threadIdx.x] = o.lin[threadIdx.x];
    __syncthreads();
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= l.N) return;
    const size_t hw = (size_t)l.N;
    int yq, xq;
    float fy, fx;
    if (!point_split(l.pts, at, a.H, a.W, yq, xq, fy, fx)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.image) { a.image[c * hw + at] = 0.f; a.image[(3 + c) * hw + at] = 0.f; }
            if (a.shpd) a.shpd[c * hw + at] = 0.f;
            if (a.refoc) a.refoc[c * hw + at] = 0.f;
        }
        if (a.bndry) a.bndry[at] = 0.f;
        if (a.depth) a.depth[at] = 0.f;
        if (a.conf) a.conf[at] = 0.f;
        return;
    }
    const int yr = fy > 0.f, xr = fx > 0.f;
    const int s = a.stride;
    int i_lo, j_lo, i_hi, j_hi;
    point_run<TABLES>(a.ys, s, a.hp, yq, yr, i_lo, i_hi);
    point_run<TABLES>(a.xs, s, a.wp, xq, xr, j_lo, j_hi);
    float acc1[3] = {0, 0, 0}, acc2[3] = {0, 0, 0}, accs[3] = {0, 0, 0}, accf[3] = {0, 0, 0};
    float accb = 0.f, accz = 0.f;
    int cnt = 0, cntz = 0;
    const float rs = be::kRoot2 * 1e-4f;
    for (int i = i_lo; i <= i_hi; ++i) {
        const float py = lattice_coord(lin, yq - (TABLES ? a.ys[i] : s * i), yr, fy);
        for (int j = j_lo; j <= j_hi; ++j) {
            const float px = lattice_coord(lin, xq - (TABLES ? a.xs[j] : s * j), xr, fx);
            const float4* rp = reinterpret_cast<const float4*>(a.records + (size_t)(i * a.wp + j) * REC);
            float r[REC];
#pragma unroll
            for (int q = 0; q < REC / 4; ++q) { const float4 t = rp[q]; r[4 * q] = t.x; r[4 * q + 1] = t.y; r[4 * q + 2] = t.z; r[4 * q + 3] = t.w; }
            be::WedgeGeom g;
            g.x0 = r[0]; g.y0 = r[1]; g.x1 = r[2]; g.y1 = r[3];
            g.s11 = r[4]; g.c11 = r[5]; g.s12 = r[6]; g.c12 = r[7]; g.s21 = r[8]; g.c21 = r[9]; g.s22 = r[10]; g.c22 = r[11];
            g.sg1 = r[12]; g.sg2 = r[13];
            float d1, d2;
            be::wedge_dists(g, px, py, o.w, d1, d2);
            const float* col = r + R_COL;
            float u0, u1, u2;
            {
#pragma clang fp contract(off)
                if (a.image) {
                    be::indicators(d1, d2, r[R_RAD1], r[R_RAD1 + 1], u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc1[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                    be::indicators(d1, d2, r[R_RAD2], r[R_RAD2 + 1], u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc2[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
                if (a.shpd) {
                    be::indicators(d1, d2, rs, rs, u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) accs[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
                if (a.refoc) {
                    be::indicators(d1, d2, r[R_RADF], r[R_RADF + 1], u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) accf[c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
                if (a.bndry) accb += be::boundary_value(d1, d2, o.delta_sq);
                if (a.depth || a.conf) {
                    const int m = be::depth_mask(d1, d2, o.delta_sq, a.densify_w != 0);
                    if (m == 1) { accz += r[R_DEPTH]; ++cntz; }
                    else if (m == 2) { accz += r[R_DEPTH + 1]; ++cntz; }
                }
            }
            ++cnt;
        }
    }
    const float n = (float)cnt;                         // the patches visited (0 only where a uniform grid stops short of the edge)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (a.image) { a.image[c * hw + at] = acc1[c] / n; a.image[(3 + c) * hw + at] = acc2[c] / n; }
        if (a.shpd) a.shpd[c * hw + at] = accs[c] / n;
        if (a.refoc) a.refoc[c * hw + at] = accf[c] / n;
    }
    if (a.bndry) a.bndry[at] = accb / n;
    if (a.depth) a.depth[at] = accz / (cntz > 0 ? (float)cntz : 1.0f);
    if (a.conf) a.conf[at] = (float)cntz / n;
}

template <bool TABLES>
__global__ __launch_bounds__(256)
void k_fold_refocus_stack_points(be_render_opts o, be_depth_consts dc, StackArgs a, Points l) {
    __shared__ float lin[R];
    if (threadIdx.x < R) lin[threadIdx.x] = o.lin[threadIdx.x];
    __syncthreads();
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= l.N) return;
    const size_t hw = (size_t)l.N;
    const int k0 = blockIdx.y * FOLD_KC;
    const int nk = min(FOLD_KC, a.K - k0);                      // planes of this chunk (uniform over the workgroup)
    int yq, xq;
    float fy, fx;
    if (!point_split(l.pts, at, a.H, a.W, yq, xq, fy, fx)) {
#pragma unroll
        for (int k = 0; k < FOLD_KC; ++k) {
            if (k < nk) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.out[((size_t)(k0 + k) * 3 + c) * hw + at] = 0.f;
            }
        }
        return;
    }
    const int yr = fy > 0.f, xr = fx > 0.f;
    float rho[FOLD_KC];
#pragma unroll
    for (int k = 0; k < FOLD_KC; ++k) rho[k] = a.rho_primes[k0 + min(k, nk - 1)];
    const int s = a.stride;
    int i_lo, j_lo, i_hi, j_hi;
    point_run<TABLES>(a.ys, s, a.hp, yq, yr, i_lo, i_hi);
    point_run<TABLES>(a.xs, s, a.wp, xq, xr, j_lo, j_hi);
    float acc[FOLD_KC][3];
#pragma unroll
    for (int k = 0; k < FOLD_KC; ++k) { acc[k][0] = 0.f; acc[k][1] = 0.f; acc[k][2] = 0.f; }
    int cnt = 0;
    for (int i = i_lo; i <= i_hi; ++i) {
        const float py = lattice_coord(lin, yq - (TABLES ? a.ys[i] : s * i), yr, fy);
        for (int j = j_lo; j <= j_hi; ++j) {
            const float px = lattice_coord(lin, xq - (TABLES ? a.xs[j] : s * j), xr, fx);
            const float4* rp = reinterpret_cast<const float4*>(a.records + (size_t)(i * a.wp + j) * REC);
            float r[REC];
#pragma unroll
            for (int q = 0; q < REC / 4; ++q) { const float4 t = rp[q]; r[4 * q] = t.x; r[4 * q + 1] = t.y; r[4 * q + 2] = t.z; r[4 * q + 3] = t.w; }
            be::WedgeGeom g;
            g.x0 = r[0]; g.y0 = r[1]; g.x1 = r[2]; g.y1 = r[3];
            g.s11 = r[4]; g.c11 = r[5]; g.s12 = r[6]; g.c12 = r[7]; g.s21 = r[8]; g.c21 = r[9]; g.s22 = r[10]; g.c22 = r[11];
            g.sg1 = r[12]; g.sg2 = r[13];
            float d1, d2;
            be::wedge_dists(g, px, py, o.w, d1, d2);
            const float* col = r + R_COL;
            const float z1 = r[R_DEPTH], z2 = r[R_DEPTH + 1];
            const int flags = (int)r[R_FLAGS];
            const bool has1 = (flags & 1) != 0, has2 = (flags & 2) != 0;
#pragma unroll
            for (int k = 0; k < FOLD_KC; ++k) {
                if (k < nk) {
#pragma clang fp contract(off)
                    const float s1 = has1 ? be::depth2sigma(dc, z1, rho[k]) : 1e-4f;       // as k_render_records writes R_RADF
                    const float s2 = has2 ? be::depth2sigma(dc, z2, rho[k]) : 1e-4f;
                    float u0, u1, u2;
                    be::indicators(d1, d2, be::kRoot2 * s1, be::kRoot2 * s2, u0, u1, u2);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[k][c] += u0 * col[3 * c] + u1 * col[3 * c + 1] + u2 * col[3 * c + 2];
                }
            }
            ++cnt;
        }
    }
    const float n = (float)cnt;
#pragma unroll
    for (int k = 0; k < FOLD_KC; ++k) {
        if (k < nk) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.out[((size_t)(k0 + k) * 3 + c) * hw + at] = acc[k][c] / n;
        }
    }
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

extern "C" int be_fold_records_f32(const be_render_opts* o, const float* records, int hp, int wp, int H, int W,
                                   int stride, int densify_w, float* image, float* shpd, float* refoc, float* bndry,
                                   float* depth, float* conf, void* stream) {
    BE_REQUIRE(o && records, "be_fold_records_f32: null pointer");
    BE_REQUIRE(hp > 0 && wp > 0 && H > 0 && W > 0 && stride > 0, "be_fold_records_f32: bad sizes");
    BE_REQUIRE(stride * (hp - 1) + R <= H && stride * (wp - 1) + R <= W, "be_fold_records_f32: patch grid exceeds the image");
    BE_REQUIRE(be::aligned16(records), "be_fold_records_f32: records must be 16-byte aligned");
    FoldArgs a{records, hp, wp, H, W, stride, densify_w, image, shpd, refoc, bndry, depth, conf, 0, nullptr, nullptr};
    hipLaunchKernelGGL(k_fold_records<false>, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, be::as_stream(stream), *o, a);
    return be::check_launch("be_fold_records_f32");
}

extern "C" int be_fold_records_batch_f32(const be_render_opts* o, const float* records, int B, int hp, int wp, int H, int W,
                                         int stride, int densify_w, float* image, float* shpd, float* refoc, float* bndry,
                                         float* depth, float* conf, void* stream) {
    BE_REQUIRE(o && records, "be_fold_records_batch_f32: null pointer");
    BE_REQUIRE(B > 0 && B <= 65535 && hp > 0 && wp > 0 && H > 0 && W > 0 && stride > 0, "be_fold_records_batch_f32: bad sizes");
    BE_REQUIRE(stride * (hp - 1) + R <= H && stride * (wp - 1) + R <= W, "be_fold_records_batch_f32: patch grid exceeds the image");
    BE_REQUIRE(be::aligned16(records), "be_fold_records_batch_f32: records must be 16-byte aligned");
    FoldArgs a{records, hp, wp, H, W, stride, densify_w, image, shpd, refoc, bndry, depth, conf, (int64_t)hp * wp * REC, nullptr, nullptr};
    hipLaunchKernelGGL(k_fold_records<false>, dim3((W + 15) / 16, (H + 15) / 16, B), dim3(256), 0, be::as_stream(stream), *o, a);
    return be::check_launch("be_fold_records_batch_f32");
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
    BE_REQUIRE(o && records && ys && xs, "be_fold_records_grid_f32: null pointer");
    BE_REQUIRE(H >= R && W >= R, "be_fold_records_grid_f32: the image is smaller than one patch");
    BE_REQUIRE(HP > 0 && WP > 0 && HP <= H - R + 1 && WP <= W - R + 1,
               "be_fold_records_grid_f32: HP / WP must be in [1, H-20] / [1, W-20] (origins are distinct pixels)");
    BE_REQUIRE((H + FOLD_TILE - 1) / FOLD_TILE <= 65535 && (int64_t)HP * WP <= 0x7fffffff, "be_fold_records_grid_f32: image too large");
    BE_REQUIRE(be::aligned16(records), "be_fold_records_grid_f32: records must be 16-byte aligned");
    FoldArgs a{records, HP, WP, H, W, 0, densify_w, image, shpd, refoc, bndry, depth, conf, 0, ys, xs};
    hipLaunchKernelGGL(k_fold_records<true>, dim3((W + FOLD_TILE - 1) / FOLD_TILE, (H + FOLD_TILE - 1) / FOLD_TILE), dim3(256), 0,
                       be::as_stream(stream), *o, a);
    return be::check_launch("be_fold_records_grid_f32");
}

extern "C" int be_refocus_stack_chunk(void) { return FOLD_KC; }

extern "C" int be_fold_refocus_stack_f32(const be_render_opts* o, const be_depth_consts* dc, const float* records, int HP, int WP,
                                         int H, int W, int stride, const int32_t* ys, const int32_t* xs, const float* rho_primes,
                                         int K, float* out, void* stream) {
    BE_REQUIRE(o && dc && records && rho_primes && out, "be_fold_refocus_stack_f32: null pointer");
    BE_REQUIRE((ys == nullptr) == (xs == nullptr), "be_fold_refocus_stack_f32: ys and xs must both be given (origin tables) or both be null (uniform grid)");
    BE_REQUIRE(K >= 1 && (K + FOLD_KC - 1) / FOLD_KC <= 65535, "be_fold_refocus_stack_f32: K must be in [1, 65535 * BE_REFOCUS_STACK_KC]");
    BE_REQUIRE(HP > 0 && WP > 0 && H >= R && W >= R, "be_fold_refocus_stack_f32: bad sizes");
    BE_REQUIRE((H + FOLD_TILE - 1) / FOLD_TILE <= 65535 && (int64_t)HP * WP <= 0x7fffffff, "be_fold_refocus_stack_f32: image too large");
    BE_REQUIRE(be::aligned16(records), "be_fold_refocus_stack_f32: records must be 16-byte aligned");
    const dim3 grid((W + FOLD_TILE - 1) / FOLD_TILE, (H + FOLD_TILE - 1) / FOLD_TILE, (K + FOLD_KC - 1) / FOLD_KC);
    if (ys) {
        BE_REQUIRE(HP <= H - R + 1 && WP <= W - R + 1,
                   "be_fold_refocus_stack_f32: HP / WP must be in [1, H-20] / [1, W-20] (origins are distinct pixels)");
        StackArgs a{records, rho_primes, out, HP, WP, H, W, 0, K, ys, xs};
        hipLaunchKernelGGL(k_fold_refocus_stack<true>, grid, dim3(256), 0, be::as_stream(stream), *o, *dc, a);
    } else {
        BE_REQUIRE(stride > 0, "be_fold_refocus_stack_f32: bad sizes");
        BE_REQUIRE((int64_t)stride * (HP - 1) + R <= H && (int64_t)stride * (WP - 1) + R <= W,
                   "be_fold_refocus_stack_f32: patch grid exceeds the image");
        StackArgs a{records, rho_primes, out, HP, WP, H, W, stride, K, nullptr, nullptr};
        hipLaunchKernelGGL(k_fold_refocus_stack<false>, grid, dim3(256), 0, be::as_stream(stream), *o, *dc, a);
    }
    return be::check_launch("be_fold_refocus_stack_f32");
}

// the host checks the two *_at entries share: the grid (uniform or tables), the scale and the window -> the lattice
static int check_lattice(const char* who, int HP, int WP, int H, int W, int stride, const int32_t* ys, const int32_t* xs, int scale,
                         int top, int left, int h, int w, Lattice* l) {
    BE_REQUIRE((ys == nullptr) == (xs == nullptr), "%s: ys and xs must both be given (origin tables) or both be null (uniform grid)", who);
    BE_REQUIRE(scale >= 1 && scale <= BE_RENDER_AT_MAX_SCALE, "%s: scale must be in [1, %d], got %d", who, BE_RENDER_AT_MAX_SCALE, scale);
    BE_REQUIRE(HP > 0 && WP > 0 && H >= R && W >= R, "%s: bad sizes", who);
    BE_REQUIRE((int64_t)HP * WP <= 0x7fffffff && (int64_t)H * scale <= 0x7fffffff && (int64_t)W * scale <= 0x7fffffff,
               "%s: image too large (HP * WP, H * scale and W * scale must fit 31 bits)", who);
    BE_REQUIRE(top >= 0 && left >= 0 && h >= 1 && w >= 1 && (int64_t)top + h <= H && (int64_t)left + w <= W,
               "%s: window (%d, %d, %d, %d) leaves the %d x %d image", who, top, left, h, w, H, W);
    if (ys) {
        BE_REQUIRE(HP <= H - R + 1 && WP <= W - R + 1, "%s: HP / WP must be in [1, H-20] / [1, W-20] (origins are distinct pixels)", who);
    } else {
        BE_REQUIRE(stride > 0, "%s: bad sizes", who);
        BE_REQUIRE((int64_t)stride * (HP - 1) + R <= H && (int64_t)stride * (WP - 1) + R <= W, "%s: patch grid exceeds the image", who);
    }
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
    BE_REQUIRE(o && records, "be_fold_records_at_f32: null pointer");
    BE_REQUIRE(be::aligned16(records), "be_fold_records_at_f32: records must be 16-byte aligned");
    Lattice l;
    if (const int rc = check_lattice("be_fold_records_at_f32", HP, WP, H, W, stride, ys, xs, scale, top, left, h, w, &l)) return rc;
    FoldArgs a{records, HP, WP, H, W, ys ? 0 : stride, densify_w, image, shpd, refoc, bndry, depth, conf, 0, ys, xs};
    const dim3 grid((l.Wo + FOLD_TILE - 1) / FOLD_TILE, (l.Ho + FOLD_TILE - 1) / FOLD_TILE);
    if (ys) hipLaunchKernelGGL(k_fold_records_at<true>, grid, dim3(256), 0, be::as_stream(stream), *o, a, l);
    else hipLaunchKernelGGL(k_fold_records_at<false>, grid, dim3(256), 0, be::as_stream(stream), *o, a, l);
    return be::check_launch("be_fold_records_at_f32");
}

extern "C" int be_fold_refocus_stack_at_f32(const be_render_opts* o, const be_depth_consts* dc, const float* records, int HP, int WP,
                                            int H, int W, int stride, const int32_t* ys, const int32_t* xs, int scale, int top,
                                            int left, int h, int w, const float* rho_primes, int K, float* out, void* stream) {
    BE_REQUIRE(o && dc && records && rho_primes && out, "be_fold_refocus_stack_at_f32: null pointer");
    BE_REQUIRE(be::aligned16(records), "be_fold_refocus_stack_at_f32: records must be 16-byte aligned");
    BE_REQUIRE(K >= 1 && (K + FOLD_KC - 1) / FOLD_KC <= 65535, "be_fold_refocus_stack_at_f32: K must be in [1, 65535 * BE_REFOCUS_STACK_KC]");
    Lattice l;
    if (const int rc = check_lattice("be_fold_refocus_stack_at_f32", HP, WP, H, W, stride, ys, xs, scale, top, left, h, w, &l)) return rc;
    StackArgs a{records, rho_primes, out, HP, WP, H, W, ys ? 0 : stride, K, ys, xs};
    const dim3 grid((l.Wo + FOLD_TILE - 1) / FOLD_TILE, (l.Ho + FOLD_TILE - 1) / FOLD_TILE, (K + FOLD_KC - 1) / FOLD_KC);
    if (ys) hipLaunchKernelGGL(k_fold_refocus_stack_at<true>, grid, dim3(256), 0, be::as_stream(stream), *o, *dc, a, l);
    else hipLaunchKernelGGL(k_fold_refocus_stack_at<false>, grid, dim3(256), 0, be::as_stream(stream), *o, *dc, a, l);
    return be::check_launch("be_fold_refocus_stack_at_f32");
}

// the host checks the two *_points entries share: the grid (uniform or tables), the point list and its launch
constexpr int64_t POINTS_MAX = (int64_t)0x00ffffff * 256;      // workgroups * 256 threads stay below 2^32

static int check_points(const char* who, int HP, int WP, int H, int W, int stride, const int32_t* ys, const int32_t* xs,
                        const float* points, int64_t N) {
    BE_REQUIRE((ys == nullptr) == (xs == nullptr), "%s: ys and xs must both be given (origin tables) or both be null (uniform grid)", who);
    BE_REQUIRE(points, "%s: null pointer", who);
    BE_REQUIRE(HP > 0 && WP > 0 && H >= R && W >= R, "%s: bad sizes", who);
    BE_REQUIRE((int64_t)HP * WP <= 0x7fffffff && H <= (1 << 24) && W <= (1 << 24),
               "%s: image too large (HP * WP must fit 31 bits, H and W 24 bits: positions are float32)", who);
    BE_REQUIRE(N >= 1 && N <= POINTS_MAX, "%s: N must be in [1, %lld], got %lld", who, (long long)POINTS_MAX, (long long)N);
    if (ys) {
        BE_REQUIRE(HP <= H - R + 1 && WP <= W - R + 1, "%s: HP / WP must be in [1, H-20] / [1, W-20] (origins are distinct pixels)", who);
    } else {
        BE_REQUIRE(stride > 0, "%s: bad sizes", who);
        BE_REQUIRE((int64_t)stride * (HP - 1) + R <= H && (int64_t)stride * (WP - 1) + R <= W, "%s: patch grid exceeds the image", who);
    }
    return BE_OK;
}

extern "C" int be_fold_records_points_f32(const be_render_opts* o, const float* records, int HP, int WP, int H, int W, int stride,
                                          const int32_t* ys, const int32_t* xs, const float* points, int64_t N, int densify_w,
                                          float* image, float* shpd, float* refoc, float* bndry, float* depth, float* conf,
                                          void* stream) {
    BE_REQUIRE(o && records, "be_fold_records_points_f32: null pointer");
    BE_REQUIRE(be::aligned16(records), "be_fold_records_points_f32: records must be 16-byte aligned");
    if (const int rc = check_points("be_fold_records_points_f32", HP, WP, H, W, stride, ys, xs, points, N)) return rc;
    FoldArgs a{records, HP, WP, H, W, ys ? 0 : stride, densify_w, image, shpd, refoc, bndry, depth, conf, 0, ys, xs};
    const Points l{points, N};
    const dim3 grid((unsigned)((N + 255) / 256));
    if (ys) hipLaunchKernelGGL(k_fold_records_points<true>, grid, dim3(256), 0, be::as_stream(stream), *o, a, l);
    else hipLaunchKernelGGL(k_fold_records_points<false>, grid, dim3(256), 0, be::as_stream(stream), *o, a, l);
    return be::check_launch("be_fold_records_points_f32");
}

extern "C" int be_fold_refocus_stack_points_f32(const be_render_opts* o, const be_depth_consts* dc, const float* records, int HP, int WP,
                                                int H, int W, int stride, const int32_t* ys, const int32_t* xs, const float* points,
                                                int64_t N, const float* rho_primes, int K, float* out, void* stream) {
    BE_REQUIRE(o && dc && records && rho_primes && out, "be_fold_refocus_stack_points_f32: null pointer");
    BE_REQUIRE(be::aligned16(records), "be_fold_refocus_stack_points_f32: records must be 16-byte aligned");
    BE_REQUIRE(K >= 1 && (K + FOLD_KC - 1) / FOLD_KC <= 65535, "be_fold_refocus_stack_points_f32: K must be in [1, 65535 * BE_REFOCUS_STACK_KC]");
    if (const int rc = check_points("be_fold_refocus_stack_points_f32", HP, WP, H, W, stride, ys, xs, points, N)) return rc;
    StackArgs a{records, rho_primes, out, HP, WP, H, W, ys ? 0 : stride, K, ys, xs};
    const Points l{points, N};
    const dim3 grid((unsigned)((N + 255) / 256), (K + FOLD_KC - 1) / FOLD_KC);
    if (ys) hipLaunchKernelGGL(k_fold_refocus_stack_points<true>, grid, dim3(256), 0, be::as_stream(stream), *o, *dc, a, l);
    else hipLaunchKernelGGL(k_fold_refocus_stack_points<false>, grid, dim3(256), 0, be::as_stream(stream), *o, *dc, a, l);
    return be::check_launch("be_fold_refocus_stack_points_f32");
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
