/*
 * blurry_edges_hip.h -- C ABI of libblurry_edges_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary of the Blurry-Edges hot path: local_stage CNN -> blurred-wedge renderer with ridge
 * colour solve -> DfD depth solve (+ overlap tiling).  The reference has no FFI of its own (100 % Python on
 * ATen ops); each entry point below replaces the ATen op sequence of the reference function it cites and is
 * what a binding for that function would call (ctypes stub: INTEGRATION.md; the build's own Python host
 * side in blurry-edges_amd/{models,utils} binds exactly these symbols).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in _host; tensors are dense, fp32,
 *     row-major in the layout written next to the parameter; nothing is allocated or freed by the library
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all calls are asynchronous on
 *     it and graph-capturable (no allocation, no synchronisation inside)
 *   - return value: BE_OK (0) or a negative BE_E* code; be_last_error() gives the message of the last
 *     failure on the calling thread.  Invalid shapes are refused on the host before anything is launched.
 */
#ifndef BLURRY_EDGES_HIP_H
#define BLURRY_EDGES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BE_OK            0
#define BE_EINVAL       -1   /* bad argument (null pointer, size, alignment, unsupported shape) */
#define BE_EWORKSPACE   -2   /* workspace too small                                          */
#define BE_ELAUNCH      -3   /* HIP reported an error at launch                              */

#define BE_R             21  /* patch side, utils/args.py:11                                 */
#define BE_NPIX          441
#define BE_LOCAL_OUT     10  /* LocalStage output_dim, models/local_stage.py:31              */

int         be_version(void);
const char* be_last_error(void);

/* ---------------------------------------------------------------------------------------------------
 * DepthEtas  (utils/depth_etas.py:3-37)
 * ------------------------------------------------------------------------------------------------- */

/* Constants of DepthEtas.__init__ (utils/depth_etas.py:4-21), computed by the caller exactly as the
 * reference does (python float64 -> rounded to fp32 on use; intercept / sin / cos are the fp32 tensor
 * values) so branch decisions agree bit for bit. */
typedef struct be_depth_consts {
    float s;            /* cam_params['s']                                   */
    float numerator;    /* 2 s^2 (rho_2 - rho_1)                        :13 */
    float den_const;    /* -s (rho_1-rho_2)(rho_1 s + rho_2 s - 2)      :14 */
    float k;            /* denominator_factor_root                      :15 */
    float k2;           /* denominator_factor                           :16 */
    float intercept;    /*                                              :18 */
    float sin_w, cos_w; /* sin/cos(theta_wng = pi/4)                    :21 */
    float sin_m, cos_m; /* sin/cos(theta_mid = 3pi/4)                   :20 */
} be_depth_consts;

/* params2etas (utils/postprocessing_loss.py:88-89): eta = 10^(2 erf(p) - 2), elementwise, n elements. */
int be_params2etas_f32(const float* p, float* eta, int64_t n, void* stream);

/* DepthEtas.etas2depth (utils/depth_etas.py:23-34), elementwise over n (eta1[i], eta2[i]) pairs.
 * branch (optional, may be NULL): int32 id 0..3 of the locus segment taken. */
int be_etas2depth_f32(const be_depth_consts* consts_host, const float* eta1, const float* eta2,
                      float* depth, int32_t* branch, int64_t n, void* stream);

/* DepthEtas.depth2sigma (utils/depth_etas.py:36-37), elementwise. */
int be_depth2sigma_f32(const be_depth_consts* consts_host, const float* depth, float rho_prime,
                       float* eta, int64_t n, void* stream);

/* Config-2 composition: params10 [2P,10] image-major (rows 0..P-1 aperture 1, rows
 * P..2P-1 aperture 2, the order of blurry_edges_test.py:121); depth [P,2]:
 *   depth[i][k] = etas2depth(params2etas(params10[i][8+k]), params2etas(params10[P+i][8+k])). */
int be_local_depth_f32(const be_depth_consts* consts_host, const float* params10, float* depth,
                       int64_t n_pairs, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Blurred-wedge renderer, colours-only pass ("pass A")
 *   replaces PostProcess.forward(colors_only=True) -> get_patches -> get_colors
 *   (blurry_edges_test.py:19-34,81-92) and LocalLoss.get_patches (local_training.py:32-45):
 *   params2dists :43-86, params2etas :88-89, dists2indicators :91-95, A^T A + lambda I, A^T y,
 *   3x3 solve (utils/postprocessing_loss.py:104-112), composite.
 * ------------------------------------------------------------------------------------------------- */
typedef struct be_render_opts {
    float lambda_ridge;    /* (alpha_lambda R^2)^2, utils/postprocessing_loss.py:14                 */
    float w;               /* args.w (1.0), :71-76                                                   */
    float delta_sq;        /* normalized_gaussian delta^2 = fp32(0.07**2), :97-98                    */
    int   wrap_angles;     /* 1: params[4:8] <- remainder(., 2pi) first (blurry_edges_test.py:124)   */
    float lin[BE_R];       /* torch.linspace(-1,1,21) as fp32, :15-16                                */
} be_render_opts;

/* params10 [N,10], patches [N,3,21,21]  ->  colors [N,3(rgb),3(wedge)].
 * Optional outputs (NULL to skip): recon [N,3,21,21] composited patch, boundary [N,21,21],
 * dists [N,2,21,21], wedges [N,3,21,21], gram [N,3,3] (A^T A + lambda I), aty [N,3(wedge),3(rgb)].
 * The 3x3 system is solved in fp64 by cofactors (numerically better than the reference's fp32
 * Cayley-Hamilton inverse; parity is judged against the fp64 oracle). */
int be_render_colors_f32(const be_render_opts* opts_host, const float* params10, const float* patches,
                         float* colors, float* recon, float* boundary, float* dists, float* wedges,
                         float* gram, float* aty, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Full render pass ("pass B") + overlap aggregation
 *   replaces PostProcess.get_patches(colors_only=False) (blurry_edges_test.py:36-79) and the six nn.Fold
 *   aggregations local2global_{color,bndry,depth} (utils/postprocessing_loss.py:151-173; the big-image
 *   stitching of blurry_edges_test_big.py:166-189 is the same fold over a 284x284 record grid).
 * ------------------------------------------------------------------------------------------------- */

/* Strided view of the pixel data of a grid of patch positions, so the kernels gather on read from whatever the
 * caller has: an image pair [2,3,H,W] (s_aperture=3HW, s_chan=HW, s_row=W, s_col=1, s_pi=stride*W, s_pj=stride),
 * the reference's unfolded tensor [2,3,21,21,Hp,Wp] (s_chan=441*P, s_row=21*P, s_col=P, s_pi=Wp, s_pj=1) or
 * flat patches [2,P,3,21,21] (s_aperture=1323*P, s_chan=441, s_row=21, s_col=1, s_pi=1323*Wp, s_pj=1323).
 * Strides are in floats; patch p sits at grid position (p / wp, p % wp). */
typedef struct be_patch_view {
    const float* base;
    int64_t s_aperture, s_chan, s_row, s_col, s_pi, s_pj;
    int wp;
} be_patch_view;

/* be_render_colors_f32 reading its pixels through a view (no [N,3,21,21] copy of the unfolded pair):
 * patch n is aperture n / patches_per_image at grid position n % patches_per_image, i.e. the order of
 * img_patches.flatten(0,1) in blurry_edges_test.py:120-123. */
int be_render_colors_view_f32(const be_render_opts* opts_host, const float* params10, const be_patch_view* view_host,
                              int64_t patches_per_image, float* colors, float* recon, float* boundary, float* dists,
                              float* wedges, float* gram, float* aty, int64_t n, void* stream);

#define BE_RECORD_FLOATS 32   /* per-patch state handed from be_render_full_f32 to be_fold_records_f32 (128 B):
                                 geometry 14, sqrt2*eta for aperture 1 / aperture 2 / refocus 2+2+2, colours 9
                                 ([rgb][wedge]), wedge depths 2, mask-presence flags 1 */

/* params12 [P,12] = 8 shared geometry + eta coefficients (w1,img1),(w2,img1),(w1,img2),(w2,img2), de-normalised
 * (blurry_edges_test.py:135-138); records [P,32] out.  Optional per-patch tensors in the reference's pixel order
 * (NULL to skip): patches [P,2,3,21,21], shpd [P,3,21,21], refoc [P,3,21,21], boundary [P,21,21],
 * depth_map [P,21,21], depth_mask int32 [P,21,21].  densify_w: 1 = the '--densify w' mask rule (:47-50).
 * opts->wrap_angles is honoured (0 for de-normalised parameters, which are already in [0,2pi)). */
int be_render_full_f32(const be_render_opts* opts_host, const be_depth_consts* consts_host, float rho_prime,
                       int densify_w, const float* params12, const be_patch_view* view_host, float* records,
                       float* patches, float* shpd, float* refoc, float* boundary, float* depth_map,
                       int32_t* depth_mask, int64_t n, void* stream);

/* Owner-computes fold of a hp x wp record grid onto an H x W image (stride = patch stride, 2).  Outputs (NULL to
 * skip): image [2,3,H,W], shpd [3,H,W], refoc [3,H,W], bndry [H,W] (all / overlap count), depth [H,W] (mean
 * over patches whose mask covers the pixel) and conf [H,W] (that count / overlap count). */
int be_fold_records_f32(const be_render_opts* opts_host, const float* records, int hp, int wp, int H, int W,
                        int stride, int densify_w, float* image, float* shpd, float* refoc, float* bndry,
                        float* depth, float* conf, void* stream);
/* The same for B images in one launch (records [B][hp*wp][32], every map with a leading batch dimension): a 147 x 147 image is
 * 100 workgroups, a batch fills the chip (GlobalLoss folds the current image and boundary map of every image of a batch). */
int be_fold_records_batch_f32(const be_render_opts* o, const float* records, int B, int hp, int wp, int H, int W, int stride,
                              int densify_w, float* image, float* shpd, float* refoc, float* bndry, float* depth, float* conf,
                              void* stream);

/* The same two passes over a SEPARABLE PATCH GRID GIVEN BY ORIGIN TABLES instead of one uniform stride: patch (i, j) of the
 * HP x WP grid has its 21 x 21 window at pixel (ys[i], xs[j]) of img [2,3,H,W].  ys [HP] / xs [WP] are DEVICE int32 arrays,
 * strictly increasing, inside [0, H-21] / [0, W-21].  This generalises nn.Unfold(21, stride) (blurry_edges_test.py:120-121,
 * blurry_edges_test_big.py:116-117, defined only while (H - 21) % stride == 0) to a grid whose last line sits flush with the
 * image edge at H - 21, so every pixel of an image of any size is covered (be_hip/tiling.py builds the tables and checks
 * them; the library checks pointers and sizes, and the render clamps an origin that would leave the image).
 * Render: params12 [HP*WP,12] -> records [HP*WP,32], one launch for the whole grid, the arithmetic of the uniform entry point
 * above (with tables 0, s, 2s, .. the records are bit-identical to it). */
int be_render_full_grid_f32(const be_render_opts* opts_host, const be_depth_consts* consts_host, float rho_prime,
                            int densify_w, const float* params12, const float* img, int H, int W, const int32_t* ys,
                            const int32_t* xs, int HP, int WP, float* records, void* stream);
/* Fold (utils/postprocessing_loss.py:151-173 with nn.Fold's uniform stride replaced by the tables): pixel (y, x) visits
 * the grid lines with ys[i] <= y <= ys[i] + 20 in ascending i, then ascending j (the order of the uniform fold), and
 * divides by the number of patches it visited - the generalisation of nn.Fold(ones).  The tables must cover every pixel
 * (first origin 0, last H-21 / W-21, gaps <= 21) or the uncovered pixels are 0/0.  Owner-computes: no atomics, every
 * output written once, bit-reproducible; with tables 0, s, 2s, .. bit-identical to the uniform fold above.  Outputs as there. */
int be_fold_records_grid_f32(const be_render_opts* opts_host, const float* records, int HP, int WP, int H, int W,
                             const int32_t* ys, const int32_t* xs, int densify_w, float* image, float* shpd, float* refoc,
                             float* bndry, float* depth, float* conf, void* stream);

/* Focal stack: K refocused images from ONE record grid.  out [K,3,H,W]; plane k is, bit for bit, the `refoc` map that
 * be_render_full*_f32(rho_prime = rho_primes[k]) followed by be_fold_records*_f32 gives - the refocus radii are recomputed
 * from the record's wedge depths and mask-presence flags (sqrt2 * depth2sigma(z, rho'), or sqrt2 * 1e-4 where the flag is
 * clear; the radii stored in the record are not read), everything else of the fold is shared by the planes of a chunk.
 * rho_primes [K]: DEVICE fp32.  ys == xs == NULL: the uniform grid (origin = stride * index, as be_fold_records_f32);
 * both non-NULL: origin tables as be_fold_records_grid_f32 takes them (stride is ignored).  A workgroup accumulates
 * BE_REFOCUS_STACK_KC planes; be_refocus_stack_chunk() returns that constant. */
#define BE_REFOCUS_STACK_KC 8
int be_refocus_stack_chunk(void);
int be_fold_refocus_stack_f32(const be_render_opts* opts_host, const be_depth_consts* consts_host, const float* records,
                              int HP, int WP, int H, int W, int stride, const int32_t* ys, const int32_t* xs,
                              const float* rho_primes, int K, float* out, void* stream);

/* The folds on a lattice `scale` (k, 1..BE_RENDER_AT_MAX_SCALE) times finer than the pixels, over the window (top, left, h, w)
 * of the H x W image (input pixels; inside the image, h, w >= 1).  The maps are Ho x Wo with Ho = (h-1)*k + 1,
 * Wo = (w-1)*k + 1; output sample (iy, ix) sits at pixel position ((top*k + iy) / k, (left*k + ix) / k), so the lattice ends
 * on the window's last pixel centre and nothing is extrapolated.  be_fold_records_at_f32 restates be_fold_records_f32 /
 * be_fold_records_grid_f32 (`local2global_color / _bndry / _depth` utils/postprocessing_loss.py:151-173, with the wedge
 * functions of utils/postprocessing_loss.py evaluated at a real-valued patch coordinate): a patch of origin oy covers the
 * sample Y = top*k + iy iff oy*k <= Y <= (oy+20)*k (integers), its coordinate is lin[q] for t = Y - oy*k = q*k + r with r == 0
 * and lin[q] + ((float)r / (float)k) * (lin[q+1] - lin[q]) in fp32 otherwise, and everything after the coordinate is that
 * entry's fold - so the samples with iy % k == 0 and ix % k == 0 equal its pixels bit for bit, and scale 1 over the whole
 * image equals it entirely.  be_fold_refocus_stack_at_f32 restates be_fold_refocus_stack_f32 (out [K,3,Ho,Wo]) the same way.
 * ys == xs == NULL: the uniform grid of `stride`; both non-NULL: origin tables (stride ignored).  Every map may be NULL. */
#define BE_RENDER_AT_MAX_SCALE 16
int be_fold_records_at_f32(const be_render_opts* opts_host, const float* records, int HP, int WP, int H, int W, int stride,
                           const int32_t* ys, const int32_t* xs, int scale, int top, int left, int h, int w, int densify_w,
                           float* image, float* shpd, float* refoc, float* bndry, float* depth, float* conf, void* stream);
int be_fold_refocus_stack_at_f32(const be_render_opts* opts_host, const be_depth_consts* consts_host, const float* records,
                                 int HP, int WP, int H, int W, int stride, const int32_t* ys, const int32_t* xs, int scale,
                                 int top, int left, int h, int w, const float* rho_primes, int K, float* out, void* stream);

/* The folds at N arbitrary positions: points [N,2] float32 on the device, (y, x) in input-pixel coordinates with pixel centres
 * at the integers - the coordinate top + iy / k of the *_at entries, without the lattice.  The domain is closed,
 * 0 <= y <= H-1 and 0 <= x <= W-1; a point outside it (NaN and the infinities included) gets 0 in every requested output and
 * reads nothing.  Per axis yq = floorf(y), fy = y - yq (exact in fp32): a patch of origin oy covers the point iff
 * yq + (fy > 0) - 20 <= oy <= yq, its coordinate is lin[yq - oy] when fy == 0 and
 * lin[q] + fy * (lin[q+1] - lin[q]) in fp32 otherwise, and everything after the coordinate is the fold of
 * be_fold_records_f32 / be_fold_records_grid_f32 (be_fold_refocus_stack_f32) - so a point on a pixel centre equals that
 * entry's pixel bit for bit, and a point (top + iy / k, left + ix / k) with k a power of two equals sample (iy, ix) of the
 * *_at entries bit for bit.  Every point is evaluated on its own: the outputs do not depend on the order or the number of
 * the points.  The outputs are channel-major over the points: image [6,N] (pair image 1, then 2), shpd / refoc [3,N],
 * bndry / depth / conf [N], out [K,3,N]; a point grid [Ho,Wo] (N = Ho*Wo) then has the layout of the *_at entries.  A point
 * inside the domain but under no patch (a uniform grid that stops short of the edge) gives 0/0, as the pixel folds do.
 * ys == xs == NULL: the uniform grid of `stride`; both non-NULL: origin tables (stride ignored).  Every map may be NULL.
 * 1 <= N <= 0xffffff * 256; H, W <= 2^24 (positions are fp32). */
int be_fold_records_points_f32(const be_render_opts* opts_host, const float* records, int HP, int WP, int H, int W, int stride,
                               const int32_t* ys, const int32_t* xs, const float* points, int64_t N, int densify_w,
                               float* image, float* shpd, float* refoc, float* bndry, float* depth, float* conf, void* stream);
int be_fold_refocus_stack_points_f32(const be_render_opts* opts_host, const be_depth_consts* consts_host, const float* records,
                                     int HP, int WP, int H, int W, int stride, const int32_t* ys, const int32_t* xs,
                                     const float* points, int64_t N, const float* rho_primes, int K, float* out, void* stream);

/* Forward, depth-dependent reprojection ("align depth to colour"): the depth map of a pinhole camera, and channels that ride on
 * it, as another pinhole camera sees them.  depth [Hs,Ws] float32 on the device, metres along the optical axis, sample (iy, ix)
 * at (y, x) = (top + iy / scale, left + ix / scale) in source pixels - the coordinate of the *_at entries (scale 1: the
 * pixels).  cam_src, cam_dst: 4 host floats (fy, fx, cy, cx), pixel centres at the integers.  pose: 12 host floats, row-major R
 * [3,3] then t [3], X' = R X + t from the source frame to the target frame.  All arithmetic is fp32, one rounding per
 * operation, in this order:
 *   xn = (x - cx) / fx, yn = (y - cy) / fy;  X = xn * Z, Y = yn * Z;  Xd = ((r00 X + r01 Y) + r02 Z) + t0 (Yd, Zd likewise);
 *   u = (fxd Xd) / Zd + cxd, v = (fyd Yd) / Zd + cyd;  fu = floorf(u + 0.5f), fv = floorf(v + 0.5f).
 * be_unproject_f32: xyz [3,Ns] = (Xd, Yd, Zd), Ns = Hs * Ws; 0 in all three where Z is not a finite number > 0.
 * be_reproject_f32: a sample takes part iff Z > 0 and finite, near < Zd < inf, 0 <= fu < Wo and 0 <= fv < Ho (tested in fp32; NaN
 * fails).  Per target pixel the sample with the smallest key (bits of Zd) << 32 | source linear index wins: the nearest
 * surface, and on equal Zd the lowest source index - a minimum, so the outputs do not depend on the order of execution.
 * depth_out [Ho,Wo] its Zd, index [Ho,Wo] its linear index iy * Ws + ix, feat_out [C,Ho*Wo] gathered from feat [C,Ns]
 * (C >= 0; both may be NULL when C == 0); where nothing landed +0, -1, +0.  Every output element is written exactly once.
 * zbuf: [Ho*Wo] 64-bit words of device scratch; the entry sets it to all-ones, splats and resolves, all on `stream`.
 * 1 <= Ns, Ho*Wo <= 2^31 - 1 (the index map is int32); 1 <= scale <= BE_RENDER_AT_MAX_SCALE; near >= 0. */
int be_unproject_f32(const float* depth, int Hs, int Ws, int scale, int top, int left, const float* cam_src, const float* pose,
                     float* xyz, void* stream);
int be_reproject_f32(const float* depth, int Hs, int Ws, int scale, int top, int left, const float* cam_src, const float* cam_dst,
                     const float* pose, float near, int Ho, int Wo, const float* feat, int C, uint64_t* zbuf, float* depth_out,
                     int32_t* index, float* feat_out, void* stream);

/* Multi-view depth fusion: V views (1 <= V <= BE_FUSE_MAX_VIEWS), each a depth map with the lattice, camera and pose arguments of
 * be_reproject_f32, merged in the camera cam_dst, size Ho x Wo.  Host arrays of V entries: depth[v] [Hs[v],Ws[v]] float32 on the
 * device; weight[v] of the same shape or NULL (1 everywhere; the array itself may be NULL); feat[v] [C,Hs[v]*Ws[v]] (the array may
 * be NULL when C == 0); Hs, Ws, scale, top, left; cam_src [V,4] and pose [V,12] host floats (pose: view v's frame -> the target's);
 * cam_dst [4].  The projection is be_reproject_f32's, operation by operation.  A sample takes part iff it passes be_reproject_f32's
 * test, its weight w is > 0 (NaN fails) and wq = floorf(min(w, 16) * 65536 + 0.5) is non-zero (NULL weight: wq = 65536).
 * Per target pixel, floor = +0 at the start; in rounds r = 0 .. peel, all in fp32 without contraction:
 *   front   zmin = min over the samples on the pixel that take part with Zd > floor of the bits of Zd (uint32); all-ones = none
 *   add     base = zmin as a float, span = tau; a sample agrees iff d = Zd - base satisfies d >= 0 && d <= span; it adds
 *           wq to sw, wq * dq to swd (dq = floorf(d * 2^20 + 0.5)), 1 to cnt, bit v to mask and, per channel,
 *           wq * fq to swf (fq = floorf(min(max(f, -2048), 2048) * 65536 + 0.5); a NaN f counts as 0)
 *   mean    where cnt > 0: m = (float)((double) base + (double) swd / (double) sw * 2^-20)
 *   recentre != 0: base = m - tau (NaN where cnt == 0), span = tau + tau, the sums cleared, add and mean again
 *   decide  a pixel not yet finalised with cnt > 0 and popcount(mask) >= min_views is finalised: depth_out = m,
 *           weight_out = (float)((double) sw * 2^-16), views_out = popcount(mask), count_out = cnt, layer_out = r,
 *           feat_out[c] = (float)((double) swf[c] / (double) sw * 2^-16); with cnt > 0 and too few views floor = base + span (its
 *           front cluster is peeled off and the next round starts behind it); with cnt == 0 floor = +inf.
 * A pixel never finalised gets depth +0, weight 0, views 0, count 0, layer -1, feat +0.  Every output element is written exactly
 * once.  Every accumulation is an integer atomic (min, add, or), so the outputs depend neither on the order of execution nor on
 * the order of the views; the sums are exact in 64 bits while fewer than 2^16 samples agree on one pixel (not checked).  The
 * schedule of launches is a function of (V, recentre, peel) alone, nothing synchronises with the host, and everything runs on
 * `stream` in `scratch`: be_fuse_scratch_bytes(Ho, Wo, C) bytes of device memory, 8-byte aligned (-1 for sizes out of range).
 * 0 <= tau <= 4 (metres); 1 <= min_views <= V; 0 <= peel <= BE_FUSE_MAX_PEEL; 0 <= C <= BE_FUSE_MAX_CHANNELS. */
#define BE_FUSE_MAX_VIEWS 32
#define BE_FUSE_MAX_PEEL 8
#define BE_FUSE_MAX_CHANNELS 64
int64_t be_fuse_scratch_bytes(int Ho, int Wo, int C);
int be_fuse_views_f32(int V, const float* const* depth, const float* const* weight, const float* const* feat, int C, const int* Hs,
                      const int* Ws, const int* scale, const int* top, const int* left, const float* cam_src, const float* pose,
                      const float* cam_dst, float near, int Ho, int Wo, float tau, int min_views, int recentre, int peel,
                      void* scratch, float* depth_out, float* weight_out, int32_t* views_out, int32_t* count_out, int32_t* layer_out,
                      float* feat_out, void* stream);

/* Truncated signed distance volumes: posed depth views integrated one at a time into a regular voxel grid, and any pinhole camera
 * ray-cast out of it.  dims: 3 host ints (Nz, Ny, Nx), each in 1..BE_TSDF_MAX_DIM, product < 2^31; every volume tensor is
 * [Nz,Ny,Nx] on the device, x fastest.  origin: 3 host floats (X0, Y0, Z0), the centre of voxel (0, 0, 0); voxel: 3 host floats
 * (sX, sY, sZ) > 0, the spacing per axis; 0 < trunc <= 4; all in metres in the volume's frame.  The state is three sums, zero at
 * the start and owned by the caller: sw int32 [Nz,Ny,Nx], swd int64 [Nz,Ny,Nx], swf int64 [C,Nz,Ny,Nx] (0 <= C <=
 * BE_FUSE_MAX_CHANNELS; may be NULL when C == 0).  All float arithmetic is fp32, one rounding per operation, in the order written.
 *
 * be_tsdf_integrate_f32: one view into the sums.  depth [Hs,Ws], weight of the same shape or NULL (1 everywhere), feat [C,Hs*Ws] or
 * NULL, the lattice (scale, top, left) and cam_src as for be_reproject_f32; pose: the view's frame -> the volume's frame.  On the
 * host q = (R^T, -R^T t) is formed in double, each component of R^T t summed left to right, and rounded to 12 floats.  Per voxel
 * (iz, iy, ix), one thread each:
 *   x = X0 + (float) ix * sX, y = Y0 + (float) iy * sY, z = Z0 + (float) iz * sZ;
 *   X = ((q0 x + q1 y) + q2 z) + q9, Y = ((q3 x + q4 y) + q5 z) + q10, Z = ((q6 x + q7 y) + q8 z) + q11;
 *   u = (fx X) / Z + cx, v = (fy Y) / Z + cy;  su = floorf((u - left) * scale + 0.5f), sv = floorf((v - top) * scale + 0.5f).
 * The voxel takes part iff Z > near; 0 <= su < Ws and 0 <= sv < Hs (tested in fp32 before any conversion; NaN fails);
 * Zq = depth[sv * Ws + su] is a finite number > 0; w = weight[sv * Ws + su] > 0 (NaN fails; NULL: 1); sdf = Zq - Z >= -trunc; and
 * wq = floorf(fminf(w, 16) * 256 + 0.5f) != 0.  It then adds, with dq = floorf(fminf(sdf, trunc) / trunc * 32768 + 0.5f):
 *   sw += wq;  swd += wq * dq;  swf[c] += wq * fq[c], fq = floorf(min(max(f, -2048), 2048) * 65536 + 0.5f) (a NaN f counts as 0).
 * A voxel that does not take part is neither read nor written.  No atomics: the sums depend neither on the order of the views nor on
 * how they are grouped into calls, and are exact below 2^19 views (not checked).
 *
 * be_tsdf_mean_f32: D = (float)((double) swd / (double) sw * 2^-15) (in [-1, 1], units of trunc), W = (float)((double) sw * 2^-8),
 * Fm[c] = (float)((double) swf[c] / (double) sw * 2^-16); D and Fm are +0 where sw == 0.  D, W [Nz,Ny,Nx], Fm [C,Nz,Ny,Nx] float32.
 *
 * be_tsdf_raycast_f32: D, W, Fm as be_tsdf_mean_f32 left them, seen by camera cam_dst (fy, fx, cy, cx) of Ho x Wo pixels under
 * pose (camera frame -> volume frame).  Per pixel (v, u), one thread each:
 *   xn = ((float) u - cx) / fx, yn = ((float) v - cy) / fy;  for i = 0 .. n - 1: z = z_near + (float) i * step;
 *   X = xn * z, Y = yn * z;  Px = ((r0 X + r1 Y) + r2 z) + t0 (Py, Pz likewise);
 *   gx = (Px - X0) / sX, ix = floorf(gx), fx = gx - ix (y, z likewise).
 * The sample is valid iff 0 <= ix <= Nx - 2, 0 <= iy <= Ny - 2, 0 <= iz <= Nz - 2 (in fp32; NaN fails) and W > 0 at all 8 corners
 * (iz + dz, iy + dy, ix + dx); an invalid sample gathers nothing further.  F is the trilinear value of D: along x
 * c = a0 + fx * (a1 - a0) for the four corner pairs, then along y, then along z in the same form; Wt and the channels likewise.
 * The first i whose sample and the one before are both valid with F_prev > 0 and F <= 0 is the hit, where the loop ends:
 *   a = F_prev / (F_prev - F), depth_out = z_prev + (z - z_prev) * a, weight_out = Wt_prev + a * (Wt - Wt_prev),
 *   feat_out[c] = Fc_prev + a * (Fc - Fc_prev).  An invalid sample resets the bracket; a crossing from behind (F_prev <= 0 < F) is
 * walked through.  No hit: +0 in every output.  z_near > 0, so depth_out > 0 exactly on the hit pixels.  depth_out, weight_out
 * [Ho,Wo], feat_out [C,Ho*Wo]; every output element is written exactly once.  step > 0; 1 <= n <= BE_TSDF_MAX_STEPS.
 * Nothing synchronises with the host; everything runs on `stream`. */
#define BE_TSDF_MAX_DIM 1024
#define BE_TSDF_MAX_STEPS 4096
int be_tsdf_integrate_f32(const float* depth, const float* weight, const float* feat, int C, int Hs, int Ws, int scale, int top, int left,
                          const float* cam_src, const float* pose, float near, const int* dims, const float* origin, const float* voxel,
                          float trunc, int32_t* sw, int64_t* swd, int64_t* swf, void* stream);
int be_tsdf_mean_f32(const int* dims, int C, const int32_t* sw, const int64_t* swd, const int64_t* swf, float* D, float* W, float* Fm,
                     void* stream);
int be_tsdf_raycast_f32(const float* D, const float* W, const float* Fm, int C, const int* dims, const float* origin, const float* voxel,
                        const float* cam_dst, const float* pose, int Ho, int Wo, float z_near, float step, int n, float* depth_out,
                        float* weight_out, float* feat_out, void* stream);

/* A triangle mesh out of a volume's means (D, W, Fm as be_tsdf_mean_f32 left them): marching tetrahedra on the Kuhn split of every
 * cell into 6 tetrahedra about the body diagonal 000-111.  be_hip/mesh.py is the statement - the numbering of corners, edge types
 * and tetrahedra, the case table (csrc/be_tsdf_mesh_table.h is generated from it), the order of the outputs and every float
 * operation - and the kernels equal it bit for bit.  A voxel is observed iff W > min_weight and positive iff D > 0; a cell (8
 * voxels) is valid iff all its corners are observed; an edge (owner voxel v, type e = 0..6 with the offsets (dx, dy, dz) = (1,0,0),
 * (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1)) carries a vertex iff its endpoints differ in positivity and a valid cell
 * contains both.  Two phases, every buffer the caller's, n = Nz Ny Nx:
 *
 * be_tsdf_mesh_count_f32: nt [n] uint8 = the triangles of the cell whose origin corner is the voxel (0..12), mask [n] uint8 = bit e
 * set when the voxel's edge e carries a vertex, voff / toff [n] int32 = the exclusive prefix sums of popcount(mask) / nt in voxel
 * order (the low 32 bits where a total exceeds them), totals [2] int64 on the device = (V, T).  workspace: 8-byte aligned,
 * be_tsdf_mesh_workspace_bytes(n) bytes.  Nothing synchronises with the host: the caller reads totals (one synchronisation, the
 * cost of a result of variable length), refuses V or T >= 2^31, allocates the outputs and calls
 *
 * be_tsdf_mesh_emit_f32 with the same D, W, dims, min_weight and the four count buffers: vertices [V,3] (X, Y, Z in the volume's
 * frame), weight [V], feat [C,V] (NULL when C == 0), normal [V,3] and normal_valid [V] uint8 (both NULL: no normals), edge [V]
 * int64 = 7 * owner + e, faces [T,3] int32.  Vertex of edge a -> b: t = Da / (Da - Db), x = xa + t * (xb - xa) per axis with
 * xa = X0 + (float) ix * sX, xb = X0 + (float)(ix + dx) * sX; weight and channels likewise.  Normal: per endpoint and axis
 * (D[+1] - D[-1]) * 0.5f / s where both neighbours exist and are observed, else (D[+1] - D[p]) / s or (D[p] - D[-1]) / s;
 * g = ga + t * (gb - ga), l = sqrtf((gx gx + gy gy) + gz gz), normal = g / l where 0 < l < inf, else +0 and normal_valid 0.
 * Vertices lie in increasing (owner, e), triangles in increasing (cell, tetrahedron, table order), wound so that their normal
 * points towards D > 0.  Every output element is written exactly once; no atomics; a repeated run gives the same bits.
 *
 * be_exclusive_scan_u8_i32: offsets[i] = counts[0] + .. + counts[i - 1] (the low 32 bits) and *total = the sum of all n counts, on
 * the device; 0 <= n < 2^31 (n == 0 writes total alone).  Three launches: sums per workgroup of BE_SCAN_SPAN elements, an exclusive
 * scan of those sums in 64 bits by one workgroup, BE_SCAN_SUMS_PER_PASS at a time, and the apply pass; no workgroup waits for
 * another.  workspace: 8-byte aligned, be_exclusive_scan_workspace_bytes(n) bytes. */
#define BE_SCAN_SPAN 1024
#define BE_SCAN_SUMS_PER_PASS 256
size_t be_exclusive_scan_workspace_bytes(int64_t n);
int be_exclusive_scan_u8_i32(const uint8_t* counts, int64_t n, int32_t* offsets, int64_t* total, void* workspace, size_t workspace_bytes,
                             void* stream);
size_t be_tsdf_mesh_workspace_bytes(int64_t n);
int be_tsdf_mesh_count_f32(const float* D, const float* W, const int* dims, float min_weight, uint8_t* nt, uint8_t* mask, int32_t* voff,
                           int32_t* toff, int64_t* totals, void* workspace, size_t workspace_bytes, void* stream);
int be_tsdf_mesh_emit_f32(const float* D, const float* W, const float* Fm, int C, const int* dims, const float* origin, const float* voxel,
                          float min_weight, const uint8_t* nt, const uint8_t* mask, const int32_t* voff, const int32_t* toff, int64_t V,
                          int64_t T, float* vertices, int32_t* faces, float* weight, float* feat, float* normal, uint8_t* normal_valid,
                          int64_t* edge, void* stream);

/* A z-buffered triangle rasteriser: the mesh (vertices [V,3] = X, Y, Z, faces [T,3] int32) seen by camera cam_dst (fy, fx, cy, cx)
 * of Ho x Wo pixels under pose = the 12 numbers (row-major R, then t) that map the MESH's frame to the CAMERA's.  be_hip/raster.py
 * is the statement - every float operation, the integer coverage rule, the key - and the kernels equal it bit for bit.
 *   vertex:   Xc = ((r0 X + r1 Y) + r2 Z) + t0 (Yc, Zc likewise), u = (fx Xc) / Zc + cx, v = (fy Yc) / Zc + cy,
 *             xs = floorf(u * BE_RASTER_SUB + 0.5f), ys likewise, q = 1 / Zc; usable iff near < Zc < inf and |xs|, |ys| <=
 *             BE_RASTER_GUARD (NaN fails).  A triangle with a vertex that is not usable is dropped whole: nothing is clipped.
 *   triangle: A = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) in int64; A == 0 is dropped; the triangle faces the camera iff A < 0;
 *             cull 0 keeps both, 1 drops A > 0 (back faces), 2 drops A < 0; A < 0 exchanges vertices 1 and 2.  E_i = the edge
 *             function of the edge opposite vertex i at (BE_RASTER_SUB x, BE_RASTER_SUB y); pixel (y, x) is inside iff every
 *             E_i > 0, or E_i == 0 on a top or left edge (dy < 0, or dy == 0 and dx > 0).
 *   depth:    w_i = (float) E_i / (float) A, iz = (w0 q0 + w1 q1) + w2 q2, z = 1 / iz; a fragment iff inside and 0 < z < inf.
 *   z-buffer: the unsigned minimum of (bits of z) << 32 | face index: the nearest surface, the lowest face index on a tie.
 *   resolve:  l_i = (w_i q_i) * z; an attribute is (l0 a0 + l1 a1) + l2 a2; the normal is interpolated, rotated by R and divided
 *             by its length l = sqrtf((mx mx + my my) + mz mz), valid iff the three vertices' normal_valid and 0 < l < inf.
 * depth_out [Ho,Wo], face_out [Ho,Wo] int32 (-1: nothing landed) always; weight_out [Ho,Wo] of weight [V], feat_out [C,Ho*Wo] of
 * feat [C,V], normal_out [3,Ho*Wo] and normal_valid_out [Ho,Wo] uint8 of normal [V,3] and normal_valid [V] uint8 (NULL: all valid),
 * bary_out [3,Ho*Wo] = l in the face's own vertex order: each NULL when not wanted; +0 where nothing landed.  A face whose index
 * lies outside [0, V) is dropped.  workspace: 16-byte aligned, be_mesh_raster_workspace_bytes(V, Ho, Wo) bytes (0: bad arguments).
 * Three kernels and a memset on `stream`: one thread per vertex, one wave per triangle (8 x 8 pixel blocks, one 64-bit atomic
 * minimum per fragment), one thread per pixel; every output element is written exactly once; nothing synchronises with the host;
 * a repeated run gives the same bits.  0 <= V, T < 2^31; 1 <= Ho, Wo <= BE_RASTER_MAX_SIZE; 0 <= C <= BE_FUSE_MAX_CHANNELS. */
#define BE_RASTER_SUB 256
#define BE_RASTER_GUARD 4194304
#define BE_RASTER_MAX_SIZE 16384
size_t be_mesh_raster_workspace_bytes(int64_t V, int Ho, int Wo);
int be_mesh_raster_f32(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const float* weight, const float* feat, int C,
                       const float* normal, const uint8_t* normal_valid, const float* cam_dst, const float* pose, float near, int cull,
                       int Ho, int Wo, float* depth_out, int32_t* face_out, float* weight_out, float* feat_out, float* normal_out,
                       uint8_t* normal_valid_out, float* bary_out, void* workspace, size_t workspace_bytes, void* stream);

/* The connected components of a mesh (vertices [V,3], faces [T,3] int32), their sizes, a decision per component, and the compaction
 * of a mesh to the vertices and faces that stay.  be_hip/components.py is the statement and the kernels equal it bit for bit: every
 * output is a function of the mesh alone.  Two vertices are connected when a chain of faces joins them (one shared vertex is
 * enough).  A face with an index outside [0, V) is ignored: it links nothing, counts nowhere, has face_component -1 and is never
 * kept.  0 <= V, T < 2^31 everywhere; nothing synchronises with the host; a repeated run gives the same bits.
 *
 * be_mesh_components_i32: label [V] = the least vertex index of the vertex's component, component [V] = the component's dense id
 * 0..K-1 in increasing order of label, face_component [T] = component[faces[3 t]], *total (int64, on the device) = K.  A lock-free
 * union-find: parent[v] = v; one thread per face unites (i0, i1) and (i1, i2), a union being atomicMin(&parent[hi], lo) on the two
 * roots, retried with the value it lost to, which is strictly smaller - no thread waits for another -; one thread per vertex walks
 * to its root; be_exclusive_scan_u8_i32 over the root flags numbers the components.  workspace: 8-byte aligned,
 * be_mesh_components_workspace_bytes(V) bytes (0: bad V).
 *
 * be_mesh_components_stats: triangles, nvertices [Kcap] int32 and area_q [Kcap] int64 per dense id, Kcap >= K (the elements from K
 * on are left 0).  The area of a face in float32, one rounding per operation, no fused multiply-add: u = b - a, v = c - a,
 * n = u x v (each component x y - z w), A = 0.5f * sqrtf((nx nx + ny ny) + nz nz), 0 when not finite, at most 2^(62 - BE_COMPONENTS_AREA_BITS) = 2^22;
 * q = (int64)(A * 2^BE_COMPONENTS_AREA_BITS); area_q = the integer sum of q.  Integer atomics, the lanes of a wave that share a
 * component combined first.
 *
 * be_mesh_components_decide: keep [Kcap] uint8, written for k < min(*total, Kcap): triangles >= min_triangles and area_q >=
 * (int64)((double) min_area * 2^BE_COMPONENTS_AREA_BITS) (clamped to 2^63 - 1); largest != 0: of those only the one with the most
 * triangles, the lowest id on a tie (a 64-bit atomicMax of (triangles << 32) | (0xffffffff - k)).  K is read on the device, so a
 * caller that sized the arrays by V needs no read-back.  vertex_keep [V] (NULL: not wanted) = keep[component[v]].  workspace:
 * 8-byte aligned, BE_COMPONENTS_DECIDE_WORKSPACE_BYTES.
 *
 * be_mesh_select_count: voff [V] / foff [T] int32 = the exclusive prefix sums of vertex_keep != 0 and of "the face's three indices
 * are in range and kept", totals [2] int64 on the device = (V', T').  workspace: 8-byte aligned, be_mesh_select_workspace_bytes(V,
 * T).  The caller reads totals (the one synchronisation a result of variable length costs), allocates and calls
 * be_mesh_select_emit with the same mesh, vertex_keep, voff, foff and V2 = V', T2 = T': the kept vertices in their order with every
 * per-vertex array given (weight [V], feat [C,V] -> [C,V2], normal [V,3], normal_valid [V] uint8, edge [V] int64, component [V]
 * int32; an input and its output are both NULL or both given), the kept faces in their order with their indices renumbered,
 * vertex_index [V2] and face_index [T2] int32 = the old positions.  Every output element is written exactly once. */
#define BE_COMPONENTS_AREA_BITS 40
#define BE_COMPONENTS_DECIDE_WORKSPACE_BYTES 8
size_t be_mesh_components_workspace_bytes(int64_t V);
int be_mesh_components_i32(const int32_t* faces, int64_t V, int64_t T, int32_t* label, int32_t* component, int32_t* face_component,
                           int64_t* total, void* workspace, size_t workspace_bytes, void* stream);
int be_mesh_components_stats(const float* vertices, const int32_t* faces, int64_t V, int64_t T, const int32_t* component, int64_t Kcap,
                             int32_t* triangles, int32_t* nvertices, int64_t* area_q, void* stream);
int be_mesh_components_decide(const int32_t* triangles, const int64_t* area_q, const int64_t* total, int64_t Kcap, int64_t min_triangles,
                              float min_area, int largest, uint8_t* keep, const int32_t* component, int64_t V, uint8_t* vertex_keep,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t be_mesh_select_workspace_bytes(int64_t V, int64_t T);
int be_mesh_select_count(const int32_t* faces, int64_t V, int64_t T, const uint8_t* vertex_keep, int32_t* voff, int32_t* foff,
                         int64_t* totals, void* workspace, size_t workspace_bytes, void* stream);
int be_mesh_select_emit(const float* vertices, const int32_t* faces, int64_t V, int64_t T, const float* weight, const float* feat, int C,
                        const float* normal, const uint8_t* normal_valid, const int64_t* edge, const int32_t* component,
                        const uint8_t* vertex_keep, const int32_t* voff, const int32_t* foff, int64_t V2, int64_t T2, float* vertices_out,
                        int32_t* faces_out, float* weight_out, float* feat_out, float* normal_out, uint8_t* normal_valid_out,
                        int64_t* edge_out, int32_t* component_out, int32_t* vertex_index, int32_t* face_index, void* stream);

/* Mesh simplification by vertex clustering on a cell grid.  be_hip/simplify.py is the statement and the kernels equal it bit for bit:
 * every output is a function of the mesh and the grid alone.  cell [3] and origin [3] are host floats (metres per axis; a corner of
 * cell (0, 0, 0)); cell must be a finite number > 0 whose reciprocal inv = (float)(1.0 / (double) cell) is finite, origin finite.
 * Per vertex and axis in float32, one rounding per operation: t = (x - o) * inv, i = floorf(t), r = t - i, q = (int64)(r *
 * 2^BE_SIMPLIFY_FRAC_BITS).  A vertex is unusable when |i| < 2^BE_SIMPLIFY_INDEX_BITS fails on an axis (NaN, inf) or its quantised
 * weight wq (be_fuse_views_f32's; 65536 with weight NULL) is 0.  0 <= V, T <= 2^29; nothing synchronises with the host; a repeated
 * run gives the same bits.  No thread waits for another: the two hash tables are open addressing over a power of two >= twice the
 * keys, a probe loop ends after that many slots at the latest and then sets the overflow word, and nothing spins.
 *
 * be_mesh_cluster_f32: label [V] = the least index among the usable vertices of the vertex's cell (-1: unusable), cluster [V] = the
 * cell's dense id 0..V'-1 in increasing order of label (-1), members [V] int32 = the vertices per dense id (0 from V' on), totals [2]
 * int64 on the device = (V', overflow != 0: the table was exhausted and the outputs are not to be used).  A slot of the table takes
 * a vertex index by a 32-bit atomicCAS when empty and atomicMin when its occupant has the same cell; be_exclusive_scan_u8_i32 over
 * the root flags numbers the clusters.  workspace: 8-byte aligned, be_mesh_cluster_workspace_bytes(V) bytes (0: bad V).
 *
 * be_mesh_simplify_count with cluster as be_mesh_cluster_f32 gave it: sums = be_mesh_simplify_sum_rows(C, normal != NULL) rows of V
 * int64 each, per dense id (64-bit integer atomics): sum wq, sum wq q (3 rows), sum wq fq_c (C rows; fq of be_fuse_views_f32) and,
 * with normals, sum wq and sum wq fq(normal) (3 rows) over the members whose normal_valid is set (NULL: all).  fflag [T] uint8 = the
 * face stays: its indices are in range, its corners lie in three different clusters, and, with (a, b, c) its clusters rotated so
 * that a is the least, it is the LEAST face index among the faces with the same (a, min(b, c), max(b, c)) and the same winding
 * (b < c) - and, with flaps == 0, no face has that triple in the other winding.  foff [T] int32 = the exclusive prefix sums of
 * fflag, totals [2] int64 on the device = (T', overflow).  workspace: 8-byte aligned, be_mesh_simplify_workspace_bytes(T).
 *
 * The caller reads both totals (the one synchronisation a result of variable length costs), allocates and calls
 * be_mesh_simplify_emit with V2 = V', T2 = T' (normals != 0: the sums hold the normal rows): per cluster in float64, one rounding per
 * operation, vertices_out = (float)(o + (i + (double) sum wq q / (double) sum wq * 2^-24) * c), weight_out (NULL: not wanted) =
 * (float)((double) sum wq / members * 2^-16), feat_out [C,V2] = (float)((double) sum wq fq / (double) sum wq * 2^-16), normal_out =
 * that mean over the valid members, normalised in float32 (l = sqrtf((x x + y y) + z z), m / l) with normal_valid_out = a valid
 * member and 0 < l < inf, else +0 and 0; the kept faces in their order with their corners renumbered, face_index [T2] = their old
 * positions.  Every output element is written exactly once. */
#define BE_SIMPLIFY_INDEX_BITS 20
#define BE_SIMPLIFY_FRAC_BITS 24
size_t be_mesh_cluster_workspace_bytes(int64_t V);
int be_mesh_cluster_f32(const float* vertices, const float* weight, int64_t V, const float* cell, const float* origin, int32_t* label,
                        int32_t* cluster, int32_t* members, int64_t* totals, void* workspace, size_t workspace_bytes, void* stream);
int be_mesh_simplify_sum_rows(int C, int normals);
size_t be_mesh_simplify_workspace_bytes(int64_t T);
int be_mesh_simplify_count(const float* vertices, const int32_t* faces, int64_t V, int64_t T, const float* weight, const float* feat, int C,
                           const float* normal, const uint8_t* normal_valid, const float* cell, const float* origin, const int32_t* cluster,
                           int flaps, int64_t* sums, uint8_t* fflag, int32_t* foff, int64_t* totals, void* workspace, size_t workspace_bytes,
                           void* stream);
int be_mesh_simplify_emit(const float* vertices, const int32_t* faces, int64_t V, int64_t T, const float* cell, const float* origin,
                          const int32_t* label, const int32_t* cluster, const int32_t* members, const int64_t* sums, int C, int normals,
                          const uint8_t* fflag, const int32_t* foff, int64_t V2, int64_t T2, float* vertices_out, int32_t* faces_out,
                          float* weight_out, float* feat_out, float* normal_out, uint8_t* normal_valid_out, int32_t* face_index, void* stream);

/* Mesh smoothing (Taubin's lambda | mu) on integer sums.  be_hip/smooth.py is the statement and the kernels equal it bit for bit: every
 * output is a function of the mesh alone.  A vertex is usable when its coordinates are finite and |x| < 2^BE_SMOOTH_COORD_MAX_LOG2; a
 * face when its indices are in [0, V), pairwise distinct, and name usable vertices (any other face is ignored).  0 <= V, T <= 2^29;
 * nothing synchronises with the host and nothing is read back; a repeated run gives the same bits.  One workspace size serves the
 * three entries: 8-byte aligned, be_mesh_smooth_workspace_bytes(V, T) bytes (0: bad V or T).
 *
 * be_mesh_adjacency_f32: valence [V] int32 = the usable faces at the vertex; boundary [V] uint8 = 1 when the vertex touches an
 * undirected edge that exactly one usable face holds (a face given twice counts twice), else 0.  The edges are counted in an
 * open-addressing table of 64-bit keys (min << 32 | max) over a power of two >= 2 * 3 T slots, claimed by atomicCAS; it holds at most
 * 3 T keys, so a probe always ends and the table cannot overflow.  No thread waits for another.
 *
 * be_mesh_smooth_f32: that setup, rows of 2 valence neighbour indices per vertex (a scan, an atomic cursor per vertex; the order in
 * a row is arbitrary), Q0 = (int64) rint((double) x * 2^BE_SMOOTH_FRAC_BITS), then per iteration a step with lam and - unless mu == 0
 * - a step with mu, one launch each: S = the int64 sum of Q over the row, d = (double) S / (double) n - (double) Q in float64 with
 * one rounding per operation, Q' = Q + (int64) rint(f * d) for a vertex with n = 2 valence > 0 that is not boundary (or any such
 * vertex with free_boundary = 1), else Q; no atomics, no LDS, no barrier.  vertices_out = the input's bits where Q == Q0 on all three
 * axes, else (float)((double) Q * 2^-30); displacement [V] = sqrtf((dx dx + dy dy) + dz dz) in float32, 0 for an unusable vertex.
 * iters in [0, BE_SMOOTH_MAX_ITERS], lam in (0, 1], mu in [-2, 0].
 *
 * be_mesh_normals_f32: per usable face cross(b - a, c - a) in float32 (be_mesh_components_stats' operation order), components that
 * are not finite 0, clamped to +-2^12, nq = (int64)(n * 2^BE_SMOOTH_NORMAL_BITS) added to the three corners (64-bit integer
 * atomics); normal [V,3] = that sum as (float)((double) sum * 2^-40), normalised in float32 (l = sqrtf((x x + y y) + z z), m / l),
 * normal_valid [V] uint8 = 0 < l < inf, else +0 and 0. */
#define BE_SMOOTH_FRAC_BITS 30
#define BE_SMOOTH_COORD_MAX_LOG2 16
#define BE_SMOOTH_NORMAL_BITS 40
#define BE_SMOOTH_MAX_ITERS 10000
size_t be_mesh_smooth_workspace_bytes(int64_t V, int64_t T);
int be_mesh_adjacency_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t T, int32_t* valence, uint8_t* boundary, void* workspace,
                          size_t workspace_bytes, void* stream);
int be_mesh_smooth_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t T, int iters, double lam, double mu, int free_boundary,
                       float* vertices_out, float* displacement, int32_t* valence, uint8_t* boundary, void* workspace, size_t workspace_bytes,
                       void* stream);
int be_mesh_normals_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t T, float* normal, uint8_t* normal_valid, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Depth registration: the two kernels of a point-to-plane ICP on depth maps; the loop around them is be_hip/registration.py.
 * Lattice, camera and pose arguments are be_reproject_f32's; all per-sample arithmetic is fp32, one rounding per operation.
 *
 * be_depth_normals_f32: normal [3,H*W] of depth [H,W] on the lattice (scale, top, left) of camera cam.  A pixel is good when its
 * depth is a finite number > 0; P is its unprojection (be_unproject_f32 under the identity pose).  Along x the neighbour at x + r
 * (r = step) counts when it is inside the image, good and |Z(x + r) - Z(x)| <= max_jump * r (one fp32 product); likewise x - r.
 * du = P(x + r) - P(x - r) when both count, P(x + r) - P(x) or P(x) - P(x - r) when one does; dv likewise along y.
 * n = du x dv (each component a b - c d), l = sqrtf((nx nx + ny ny) + nz nz), n = n / l, negated when (nx Px + ny Py) + nz Pz > 0:
 * the normal faces the camera.  (+0, +0, +0) where the pixel is not good, a direction has no neighbour that counts, or l is not a
 * finite number > 0.  Every output element is written exactly once.  1 <= step <= BE_NORMALS_MAX_STEP; max_jump >= 0, finite.
 *
 * be_icp_linearize_f32: source depth_s [Hs,Ws] (weight_s of the same shape or NULL: 1) in cam_src on its lattice, target depth_d
 * [Hd,Wd], normal_d [3,Hd*Wd] (weight_d or NULL) on the pixels of cam_dst, pose: source frame -> target frame.  Source sample i
 * with projection P = (Xd, Yd, Zd), (fu, fv) takes part iff it passes be_reproject_f32's test on the Hd x Wd frame and, with
 * j = (int) fv * Wd + (int) fu:  Zq = depth_d[j] is a finite number > 0;  n = normal_d[:, j] has a non-zero component;
 * D = P - Q, Q = (((fu - cxd) / fxd) Zq, ((fv - cyd) / fyd) Zq, Zq), satisfies (Dx Dx + Dy Dy) + Dz Dz <= max_dist max_dist;
 * w = weight_s[i] weight_d[j] satisfies w > 0 and w < inf (NaN fails every test).  Then r = (nx Dx + ny Dy) + nz Dz; with
 * huber > 0 and |r| > huber, w = w (huber / |r|); the row is J = (P x n, n) - the derivative of r under P' = P + omega x P + v.
 * The 8 floats J[0..5], r, w are converted to double and 30 terms, each multiplied left to right in double, are added up:
 * sums[0..20] = w J[a] J[b] (a <= b, row-major upper triangle), sums[21..26] = w J[a] r, sums[27] = w r r, sums[28] = w,
 * sums[29] = the number of samples that took part; sums[30] = sums[31] = 0.  The order of summation is a function of Hs * Ws alone
 * (fixed grid of at most 64 workgroups, each thread in increasing sample order, a fixed tree over lanes, waves and workgroups; no
 * floating-point atomics): repeated calls, other streams and other devices give the same bits.  sums: 32 doubles on the device;
 * rows_out: [8,Hs*Ws] float32 (J, r, w per sample; 0 where the sample took no part) or NULL; scratch: be_icp_scratch_bytes(Hs, Ws)
 * bytes of device memory, 8-byte aligned (-1 for sizes out of range).  Nothing synchronises with the host.
 * near, max_dist, huber >= 0 and finite. */
#define BE_NORMALS_MAX_STEP 8
int be_depth_normals_f32(const float* depth, int H, int W, int scale, int top, int left, const float* cam, int step, float max_jump,
                         float* normal, void* stream);
int64_t be_icp_scratch_bytes(int Hs, int Ws);
int be_icp_linearize_f32(const float* depth_s, const float* weight_s, int Hs, int Ws, int scale, int top, int left,
                         const float* cam_src, const float* depth_d, const float* normal_d, const float* weight_d, int Hd, int Wd,
                         const float* cam_dst, const float* pose, float near, float max_dist, float huber, void* scratch, double* sums,
                         float* rows_out, void* stream);

/* Dense depth from sparse samples by nearest-sample flood fill.  depth [H,W] float32 on the device; weight [H,W] float32 or NULL
 * (weight 1 everywhere).  Pixel p is a seed iff weight[p] > 0, depth[p] > 0 and depth[p] < inf (NaN fails all three).  Every pixel
 * is given a seed by jump flooding: an int32 seed map holds each pixel's current seed as the linear index y * W + x (-1: none); one
 * pass with step s gives each pixel, of the nine positions p + (dy, dx) s (dy, dx in {-1, 0, 1}) inside the image that hold a seed,
 * the candidate c with the smallest key (d2(p, c), c), d2 the integer squared distance - ties to the lower index; passes are double
 * buffered.  The steps are 1, 2^(L-1), .., 4, 2, 1 with L = ceil(log2(max(H, W))) ("1+JFA"; a 1 x 1 image: the single step 1).  The
 * assignment is the nearest seed on almost every pixel and a near-nearest one on the rest (jump flooding is approximate).
 * fuse = 1 runs the final run of steps <= 8 as one launch over LDS tiles with a 15-pixel halo, fuse = 0 one launch per pass: the
 * same integers either way.  smooth_r = r in 0..8: a seed keeps its depth bit for bit; r = 0: a hole takes its seed's depth;
 * r > 0: a hole with seed s takes num / den over the seeds q of the window [sy-r, sy+r] x [sx-r, sx+r] clipped to the image, in
 * row-major order, fp32 with one rounding per operation: d = z_q - z_s; k = w_q / (1 + (d d) inv), inv = 1 / (sigma_z sigma_z);
 * num += k z_q; den += k.  Outputs [H,W]: depth_out (the input at seeds, the filled depth at holes), index int32 (the seed's linear
 * index; the pixel's own at a seed), dist2 int32 (the squared distance to it; 0 at a seed); with no seed in the image 0, -1, -1.
 * Every output element is written exactly once; nothing synchronises with the host.  scratch: device memory for 2 H W int32 (the
 * two seed maps), and H W float32 more when smooth_r > 0 (the per-seed means).  1 <= H, W <= 16384; sigma_z > 0; fuse 0 or 1. */
int be_fill_nearest_f32(const float* depth, const float* weight, int H, int W, int smooth_r, float sigma_z, int fuse,
                        int32_t* scratch, float* depth_out, int32_t* index, int32_t* dist2, void* stream);

/* Dense depth from sparse samples by edge-aware diffusion: the holes take the harmonic interpolant of the seeds.  depth, weight as
 * be_fill_nearest_f32 (the same seeds); edge [H,W] float32 or NULL.  A seed's boundary value b is what be_fill_nearest_f32 copies
 * from it: its depth at smooth_r = 0, its robust local mean at smooth_r > 0.  With e = min(max(edge, 0), 1) (NaN: 0; NULL: 0) the
 * conductance between 4-neighbours p, q is c_pq = max(leak, 1 - max(e_p, e_q)); the image border has no neighbour and no term.
 * Every hole satisfies u_p sum_q c_pq = sum_q c_pq u_q, a neighbouring seed contributing b.  Outputs [H,W]: depth_out (the input
 * at seeds, bit for bit; u at holes), index and dist2 exactly as be_fill_nearest_f32 writes them, and residual [1] float32: the
 * maximum over the holes of |sum_q c_pq u_q / sum_q c_pq - u_p| after the last sweep.  No seed in the image: 0, -1, -1, 0; every
 * pixel a seed: a copy of the input.
 * The fixed point is reached by a fixed schedule: be_fill_nearest_f32's result is the start; a pyramid of 2 x 2 poolings (down to a
 * longer side <= 4) is relaxed from the coarsest level up, each level the start value of the holes of the next; a level is relaxed
 * by red-black over-relaxed sweeps (omega = 2 / (1 + sin(pi / longer side))) on LDS regions of up to 128 x 128, a level of several
 * 96 x 96 tiles in launches of 16 sweeps between which the 16-pixel halos are refreshed.  iters = 0: 4 x the longer side sweeps on
 * every level (rounded up to a multiple of 16); iters in 1..4096: that many on every level.  fuse = 0 runs one sweep per launch
 * (the baseline the tiled launch is timed against; the tiled levels then refresh their halos every sweep, so the values differ
 * within the convergence error).  The schedule is a function of (H, W, iters, fuse) alone: nothing depends on the data, nothing
 * synchronises with the host, no float is accumulated atomically, and repeated calls give the same bits.
 * scratch: be_fill_diffuse_scratch_bytes(H, W) bytes of device memory (-1 for a size out of range); its first 3 H W words are
 * be_fill_nearest_f32's scratch, whose third image (the per-seed means) is read here.  1 <= H, W <= 16384; sigma_z > 0;
 * 0 < leak <= 1. */
int64_t be_fill_diffuse_scratch_bytes(int H, int W);
int be_fill_diffuse_f32(const float* depth, const float* weight, const float* edge, int H, int W, int smooth_r, float sigma_z,
                        float leak, int iters, int fuse, int32_t* scratch, float* depth_out, int32_t* index, int32_t* dist2,
                        float* residual, void* stream);

/* nn.Unfold(21, stride) in the order blurry_edges_test.py:120-121 consumes it:
 * img [B,C,H,W] -> out [B, Hp*Wp, C, 21, 21], patch (i,j) = rows stride*i.., cols stride*j.., index i*Wp+j. */
int be_unfold_patches_f32(const float* img, float* out, int B, int C, int H, int W, int stride, void* stream);

/* Feature normalisation between the two stages (blurry_edges_test.py:123-132):
 * params10 [2,P,10] (raw CNN output, image-major) + colors [2,P,9] -> pm [P,38]. */
int be_local_features_f32(const float* params10, const float* colors, float* pm, int64_t P, void* stream);
/* De-normalisation of the GlobalStage output (blurry_edges_test.py:134-138): y [P,12] -> est [P,12]. */
int be_global_denorm_f32(const float* y, float* est, int64_t P, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * The base-class methods of PostProcessBase one by one (for callers that subclass the reference's
 * PostProcessLocalBase / PostProcessGlobalBase and chain them themselves), flat layout:
 * ------------------------------------------------------------------------------------------------- */
/* params2dists (utils/postprocessing_loss.py:43-86): params8 [N,8] -> dists [N,2,21,21]. */
int be_params2dists_f32(const be_render_opts* opts_host, const float* params8, float* dists, int64_t n, void* stream);
/* dists2indicators (:91-95): dists [N,2,21,21], etas [N,2] -> wedges [N,3,21,21]. */
int be_dists2indicators_f32(const float* dists, const float* etas, float* wedges, int64_t n, void* stream);
/* inverse_3by3 (:104-112): n row-major 3x3 matrices (cofactor inverse, fp64 inside). */
int be_inverse3x3_f32(const float* a, float* out, int64_t n, void* stream);
/* get_image_derivative (:114-117): per-plane Sobel magnitude, valid padding: [planes,H,W] -> [planes,H-2,W-2]. */
int be_image_derivative_f32(const float* img, float* out, int64_t planes, int H, int W, void* stream);
/* nn.Fold of a strided patch tensor (local2global_*, :151-173), owner computes.  Element (b,c,r,col,i,j) of the
 * source sits at b*s_b + c*s_c + r*s_r + col*s_col + i*s_pi + j*s_pj (floats).  mode 0: overlap sum, 1: sum /
 * overlap count, 2: number of covering patches whose entry is > 0 (src_int, if not NULL, is read instead of src). */
int be_fold_patches_f32(const float* src, const int32_t* src_int, float* out, int B, int C, int hp, int wp, int H, int W,
                        int stride, int64_t s_b, int64_t s_c, int64_t s_r, int64_t s_col, int64_t s_pi, int64_t s_pj,
                        int mode, void* stream);

/* Adjoints of the methods above and of DepthEtas, for `loss.backward()` through a caller's own LocalLoss / GlobalLoss subclass
 * (local_training.py:32-52,106; global_training.py:62-157,212).  g* = cotangent (dL/d.) with the shape of the tensor it
 * belongs to; derivatives are evaluated in fp64 from the fp32 operands; per-patch sums have a fixed order. */
/* params2dists: gdists [N,2,21,21] -> gparams8 [N,8] (d/d x0,y0,x1,y1,theta1,phi1,theta2,phi2; remainder has slope 1). */
int be_params2dists_bwd_f32(const be_render_opts* opts_host, const float* params8, const float* gdists, float* gparams8, int64_t n,
                            void* stream);
/* dists2indicators: gwedges [N,3,21,21] -> gdists [N,2,21,21], getas [N,2]. */
int be_dists2indicators_bwd_f32(const float* dists, const float* etas, const float* gwedges, float* gdists, float* getas, int64_t n,
                                void* stream);
/* inverse_3by3: inv = the forward's output, gout [n,3,3] -> ga = -inv^T gout inv^T. */
int be_inverse3x3_bwd_f32(const float* inv, const float* gout, float* ga, int64_t n, void* stream);
/* get_image_derivative: img [planes,H,W], gout [planes,H-2,W-2] -> gimg [planes,H,W]. */
int be_image_derivative_bwd_f32(const float* img, const float* gout, float* gimg, int64_t planes, int H, int W, void* stream);
/* params2etas: gp = geta * d eta / d p. */
int be_params2etas_bwd_f32(const float* p, const float* geta, float* gp, int64_t n, void* stream);
/* normalized_gaussian (utils/postprocessing_loss.py:97-98): y = exp(-x^2 / delta_sq), and its adjoint. */
int be_normalized_gaussian_f32(const float* x, float* y, float delta_sq, int64_t n, void* stream);
int be_normalized_gaussian_bwd_f32(const float* x, const float* gy, float* gx, float delta_sq, int64_t n, void* stream);
/* DepthEtas.etas2depth / depth2sigma (utils/depth_etas.py:23-37): the branch taken is the forward's. */
int be_etas2depth_bwd_f32(const be_depth_consts* consts_host, const float* eta1, const float* eta2, const float* gdepth,
                          float* geta1, float* geta2, int64_t n, void* stream);
int be_depth2sigma_bwd_f32(const be_depth_consts* consts_host, const float* depth, float rho_prime, const float* geta, float* gdepth,
                           int64_t n, void* stream);
/* be_fold_patches_f32, modes 0 (sum) and 1 (mean): gout [B,C,H,W] -> gsrc in the source's strided layout. */
int be_fold_patches_bwd_f32(const float* gout, float* gsrc, int B, int C, int hp, int wp, int H, int W, int stride, int64_t s_b,
                            int64_t s_c, int64_t s_r, int64_t s_col, int64_t s_pi, int64_t s_pj, int mode, void* stream);
/* est[:, col0:col1] <- remainder(est[:, col0:col1], 2 pi) IN PLACE, est [n,ld] (LocalLoss.get_patches, local_training.py:33). */
int be_wrap_angles_inplace_f32(float* est, int64_t n, int ld, int col0, int col1, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LocalLoss forward + backward (training)
 *   replaces LocalLoss.get_patches + LocalLoss.forward (local_training.py:32-52) and the autograd graph under
 *   them.  est [B,10] raw CNN output (angles are wrapped inside, :33), img_fit / gt [B,21,21,3] channels-last
 *   (the dataset layout; local_training.py:105 passes the clean image as both), bdist [B,21,21],
 *   deri [B,19,19,3].  partial [B,3] = per-patch sums of the three terms:
 *     loss = sum(partial[:,0])/(B*441) + beta_bndry*sum(partial[:,1])/(B*441) + beta_smooth*sum(partial[:,2])/(B*361)
 *   grad_est [B,10] = d loss / d est (NULL to skip); patches [B,3,21,21], boundary [B,21,21] optional.
 * ------------------------------------------------------------------------------------------------- */
int be_local_loss_f32(const be_render_opts* opts_host, const float* est, const float* img_fit, const float* gt,
                      const float* bdist, const float* deri, float beta_bndry, float beta_smooth, float* partial,
                      float* grad_est, float* patches, float* boundary, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * GlobalLoss forward + backward (global-stage training)
 *   replaces GlobalLoss.get_patches + get_loss (global_training.py:69-139) and the autograd graph under them.
 *   est [B,P,12] raw GlobalStage output; img_fit / img_gt [B,2,H,W,3] channels-last (dataset layout);
 *   G [B,2,3,H,W], Gderi [B,2,3,H-2,W-2], Gbndry [B,H,W]: the CURRENT folded image, its Sobel magnitude and the
 *   folded boundary map (the reference detaches them, :94,:100,:106; produce them with be_render_full_f32 +
 *   be_fold_records_f32 + be_image_derivative_f32); bdist [B,H,W]; deri [B,2,H-2,W-2,3]; bdepth [B,H,W];
 *   gamma6 (host) = gamma_{color, color_cons, bndry_cons, smthns, smthns_cons, bndry_loc}.
 *   partial [B*P,8] = per-patch sums of the six mean terms, the depth numerator and the depth-mask count;
 *   grad [B*P,12] = gradient of  sum_k gamma_k * mean_k  w.r.t. est;  grad_depth [B*P,4] = gradient of the depth
 *   NUMERATOR w.r.t. est[:,8:12] (the caller adds gamma_depth / total_mask_count * grad_depth).
 * ------------------------------------------------------------------------------------------------- */
int be_global_loss_f32(const be_render_opts* opts_host, const be_depth_consts* consts_host, const float* est,
                       const float* img_fit, const float* img_gt, const float* G, const float* Gderi,
                       const float* Gbndry, const float* bdist, const float* deri, const float* bdepth,
                       const float* gamma6_host, float* partial, float* grad, float* grad_depth, int B, int hp, int wp,
                       int H, int W, int stride, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LocalStage CNN  (models/local_stage.py:30-73), inference (BatchNorm folded into the convs)
 * ------------------------------------------------------------------------------------------------- */

/* Kernel-layout weights.  Sizes in floats: be_local_stage_packed_floats(). One contiguous device buffer. */
size_t be_local_stage_packed_floats(void);

/* The reference state-dict (100 entries) as raw device pointers, in state_dict() order,
 * skipping the int64 num_batches_tracked entries: for each of the 13 conv+BN pairs
 *   {conv.weight [Cout,Cin,k,k], conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var}
 * then fc.1.{weight [1024,2304],bias}, fc.2.{weight,bias,running_mean,running_var}, fc.4.{weight [10,1024],bias}
 * = 13*6 + 2 + 4 + 2 = 86 pointers. */
#define BE_LOCAL_STAGE_NTENSORS 86
int be_local_stage_pack_f32(const float* const* tensors_host /* [86] device ptrs */, float bn_eps,
                            float* packed, void* stream);

/* Per-call options of the forward (NULL = the defaults).  They travel with the call - no process-wide state, so two models
 * with different settings, or two host threads, do not interfere.
 *   winograd  1 (default): the 3x3 convolutions on the 6x6 maps (layers 1-3) run in Winograd form (be_wino_tile_rows()); 0: direct
 *             implicit GEMM (the form the split-bf16 experiment and A/B runs use).  Both read the same packed buffer.
 *   chunk     the batch is walked in sub-batches of this many patches (0 = default 8192) so that the workspace stays bounded
 *             whatever N is; the same value must be given to be_local_stage_workspace_bytes(). */
typedef struct be_local_stage_opts {
    int winograd;
    int chunk;
} be_local_stage_opts;

/* Workspace (activations) for a batch of n patches walked in sub-batches of `chunk` (0 = default), in bytes. */
size_t be_local_stage_workspace_bytes(int64_t n, int chunk);

/* LocalStage.forward in eval mode: x [N,3,21,21] (NCHW as the reference feeds it) -> out [N,10]. */
int be_local_stage_forward_f32(const float* packed, const float* x, float* out, int64_t n,
                               void* workspace, size_t workspace_bytes, const be_local_stage_opts* opts, void* stream);

/* The same forward with the 21x21 windows gathered from a view (e.g. straight from the image pair [2,3,H,W]) in
 * place of nn.Unfold + permute (blurry_edges_test.py:120-121); patch numbering as be_render_colors_view_f32. */
int be_local_stage_forward_view_f32(const float* packed, const be_patch_view* view_host, int64_t patches_per_image,
                                    float* out, int64_t n, void* workspace, size_t workspace_bytes,
                                    const be_local_stage_opts* opts, void* stream);

/* HOST-ONLY inspection hooks of the LocalStage eval path (no GPU, no launch).
 * be_local_stage_layout_debug: the table of regions of the packed buffer, in the order they lie in it; together they tile
 * [0, be_local_stage_packed_floats()).  Region k: layer_form_reads[3k..] = {layer (state_dict() order: 0 conv1, 1-12 the blocks'
 * conv1 / conv2 / downsample, 13 fc.1, 14 fc.4; -1: none), form, index of the region whose matrix its pack call reads or -1};
 * w_b_off_n[4k..] = {matrix offset, matrix floats, bias offset, bias floats}.  Forms: 0 fp32 matrix + bias, 1 conv2 fused with its
 * downsample's columns, 2 Winograd U with its planes + bias (the downsample's bias added), 3 the 1x1 downsample as an fp32
 * convolution of its own, 4 split-bf16 row-GEMM planes, 5 layer0's pixel-major planes, 6 the downsample as conv2's second K segment,
 * 7 the 384-float zero bias.  Returns the number of regions (<= 32), or BE_EINVAL when cap is smaller.
 * be_local_stage_route_debug: the kernels a sub-batch of nb patches takes under opts->winograd and the process's BE_* knobs.
 * out[8]: staging (0 [21,21,4], 1 rows padded to 28 pixels), conv1 (0 k_conv_igemm, 1 pixel-major LDS-DMA, 2 fp32 conv1 + pool,
 * 3 split-bf16 conv1 + pool), conv1's launch pools, layer0 in split-bf16, the Winograd blocks chained, the 6x6 blocks (0 direct
 * fused convolutions, 1 Winograd with the downsample folded into conv2's GEMMs, 2 Winograd + a split-bf16 downsample launch,
 * 3 Winograd + an fp32 downsample launch), the second pool's and the inter-block maps are stored, fc.1 on the split-bf16 row GEMM.
 * Returns 8. */
int be_local_stage_layout_debug(int* layer_form_reads, int64_t* w_b_off_n, int cap);
int be_local_stage_route_debug(int winograd, int nb, int* out);

/* Layer-level entry points (used by the layer-by-layer parity tests and by the training path).
 * Activations are NHWC.  act: 0 none, 1 Smish (models/local_stage.py:4-6), 2 ReLU (GlobalStage FFN). */
typedef struct be_conv_desc {
    int n, h, w;          /* batch, spatial size (stride 1, "same" padding)      */
    int cin, cout;        /* cin % 32 == 0 (conv1: cin = 4, NHWC4 input)         */
    int ksize;            /* 1, 3, or 7 (7: the conv1 row-gather mode: cin = 4 = the staging's channels, of which the fourth is
                           * zero padding - weights are packed from cin <= 3)  */
    int act;
} be_conv_desc;
size_t be_conv_packed_floats(int cout, int cin, int ksize);
/* Fold conv bias + eval-mode BatchNorm into packed weights/bias.  bn_* may be NULL (plain conv/linear).
 * layout_chw_hw: 0, or H*W (9) when the input features were flattened from (C,H,W) (fc.1, :45-46). */
int be_conv_pack_f32(const float* weight_oihw, const float* bias, const float* bn_gamma, const float* bn_beta,
                     const float* bn_mean, const float* bn_var, float bn_eps, int cout, int cin, int ksize,
                     int layout_chw_hw, float* packed_w, float* packed_bias, void* stream);
/* A table of pack jobs in ONE launch: job i = be_conv_pack_f32 (dgrad = 0; BatchNorm pointers may be NULL) or
 * be_conv_pack_dgrad_f32 (dgrad = 1: bias / BatchNorm pointers ignored) with the same argument meaning and the same
 * preconditions (the caller checks them: the table lives in DEVICE memory and is not inspected on the host).  A training step
 * re-packs every layer for the forward and the data-gradient convolution (local_training.py:103-106 under autograd). */
typedef struct be_pack_job {
    const float *weight, *bias, *bn_gamma, *bn_beta, *bn_mean, *bn_var;
    float* packed_w;
    float* packed_bias;
    float bn_eps;
    int cout, cin, ksize, layout_chw_hw, dgrad;
} be_pack_job;
int be_conv_pack_jobs_f32(const be_pack_job* jobs_device, int njobs, void* stream);
/* y[n,h,w,cout] = act(conv(x) + bias (+ residual)); residual may be NULL; ldy = row stride of y in floats.
 * The residual is read with y's row stride: element (m, c) at residual[m * ldy + c], on every route (implicit GEMM, pixel-major,
 * row GEMM).  With ldy > cout a contiguous [n,h,w,cout] residual would be read at the wrong stride and past its end: lay it out
 * like y.  Nothing outside y's first cout columns is written. */
int be_conv_nhwc_f32(const be_conv_desc* desc_host, const float* x, const float* packed_w,
                     const float* packed_bias, const float* residual, float* y, int ldy, void* stream);
/* The same convolution with scratch lent by the caller: launches with few output tiles (batch-64 training: M = 2304
 * rows) split their K loop over up to 8 slices (partial sums in scratch, summed in a fixed order with the bias /
 * residual / activation applied by a second small kernel); large launches behave exactly as be_conv_nhwc_f32.
 * scratch: 8 * M * cout_pad32 * 4 bytes is always enough (fewer slices are used when it is smaller).
 * The residual has y's row stride here too (residual[m * ldy + c]): the kernel that sums the slices reads it that way. */
int be_conv_nhwc_splitk_f32(const be_conv_desc* d, const float* x, const float* packed_w, const float* packed_bias,
                            const float* residual, float* y, int ldy, void* scratch, size_t scratch_bytes, void* stream);
/* HOST-ONLY inspection hook of the fp32 convolution's planner (no GPU, no launch): the plan that be_conv_nhwc_f32 and its fused2
 * / batched / splitk forms (mode 0) or the training units' convolutions (mode 1; 2: where 96-wide outputs may run as two 64-wide
 * tiles, the backward) make for desc under the process's BE_* knobs, with a fused second input of cin2 channels (0: none), a
 * residual (has_res != 0), nbatch batched problems (1: not batched) and scratch_bytes of lent scratch (0: none).  out[16]:
 * route (0 row GEMM, 1 pixel-major LDS-DMA, 2 implicit GEMM), tile (0 small 64x64, 1 small 128x32, 2 small 64x64 uniform,
 * 3 128x128, 4 128x96, 5 128x64, 6 128x32, 7 row-gather), K-chunk in floats, BE_KERNEL_* id, pixmaj, m_tiles, n_tiles,
 * grid x / y / z (x = 0: the row GEMM sizes its own grid), K slices S, ldp (row stride of the slices; 0 when S = 1), then what
 * a training pair is handed to run the convolution in its merged launch: small tile or -1 (none: mode 0, no scratch, or not a
 * small tile), S, ldp, grid x.  *flops_executed: the MFMA work of the launch as its profile record states it.
 * Returns BE_OK, or BE_EINVAL with the message the entry points give for the same arguments. */
int be_conv_plan_debug(const be_conv_desc* desc_host, int cin2, int has_res, int ldy, int nbatch, size_t scratch_bytes, int mode,
                       int* out, double* flops_executed);
/* ResidualBlock tail in ONE launch (models/local_stage.py:22-27): y = act(conv_kxk(x) + conv_1x1(x2) + bias) where the
 * second branch is the block's downsample; its 1x1 conv is appended to the K loop of the first (no residual tensor
 * in HBM).  Weights: both branches (each with its own folded BatchNorm) packed side by side, biases summed. */
size_t be_conv_fused2_packed_floats(int cout, int cin, int ksize, int cin2);
int be_conv_pack_fused2_f32(const float* weight_oihw, const float* bias, const float* bn_gamma, const float* bn_beta,
                            const float* bn_mean, const float* bn_var, const float* weight2_oi, const float* bias2,
                            const float* bn2_gamma, const float* bn2_beta, const float* bn2_mean, const float* bn2_var,
                            float bn_eps, int cout, int cin, int ksize, int cin2, float* packed_w, float* packed_bias,
                            void* stream);
int be_conv_nhwc_fused2_f32(const be_conv_desc* desc_host, const float* x, const float* x2, int cin2,
                            const float* packed_w, const float* packed_bias, float* y, int ldy, void* stream);
/* nbatch independent problems of the same shape in one launch (grid.z): batch b reads x + b*x_stride, packed_w +
 * b*w_stride and writes y + b*y_stride (strides in floats, multiples of 4).  packed_bias may be NULL (no bias) - here
 * and in be_conv_nhwc_f32.  Used for the per-position GEMMs of the Winograd convolutions below. */
int be_conv_nhwc_batched_f32(const be_conv_desc* d, const float* x, const float* packed_w, const float* packed_bias, float* y,
                             int ldy, int nbatch, int64_t x_stride, int64_t w_stride, int64_t y_stride, void* stream);

/* Winograd form of the 3x3 'same' convolutions on 6x6 maps (LocalStage layers 1-3): fewer multiplies than the direct form, the
 * transforms in fp32, the transform-domain products in split-bf16 (each fp32 operand split exactly into three bf16 pieces, six bf16
 * MFMAs per product, fp32 accumulation; per-GEMM error at or below the fp32 products'; the same bits at every batch size).
 * Environment BE_WINO_F32=1 (read once per process) restores exact fp32 products and accumulation.  Tile shape (compile-time, be_wino_tile_rows()): 6 = F(6,3) along the rows x F(3,3) along
 * the columns - two 8x5 tiles per map, 40 transform positions, 80 multiplies per map and channel pair instead of 324 (the default
 * since round 4); 3 = F(3,3) x F(3,3) - four 5x5 tiles, 25 positions, 100 multiplies (rounds 1-3).  be_wino_pack_f32 folds an
 * optional eval BatchNorm like be_conv_pack_f32 and writes U [positions][cout_pad32][cin] + bias [cout_pad32]; behind U in the same buffer
 * the hi / mid / lo bf16 pieces of U that the split-bf16 GEMMs read (positions x cout padded to 128 x cin x 3 bf16: packed size =
 * U + 1.5 x positions x cout_pad128 x cin floats, be_wino_packed_floats);
 * be_wino_conv3x3_6x6_f32 runs input transform, `positions` batched GEMMs and output transform (+ bias, residual, activation).
 * workspace: be_wino_workspace_floats(n, cin, cout) floats.  cin %% 32 == 0, cout %% 4 == 0. */
int be_wino_tile_rows(void);      /* 6 or 3: output rows per Winograd tile; positions = 5 (rows + 2), tiles per map = 12 / rows */
size_t be_wino_packed_floats(int cout, int cin);
int be_wino_pack_f32(const float* w_oihw, const float* bias, const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                     const float* bn_var, float bn_eps, int cout, int cin, float* packed_w, float* packed_bias, void* stream);
size_t be_wino_workspace_floats(int64_t n, int cin, int cout);
int be_wino_conv3x3_6x6_f32(const float* x, const float* packed_w, const float* packed_bias, const float* residual, float* y,
                            int64_t n, int cin, int cout, int act, float* workspace, size_t workspace_floats, void* stream);

/* Two chained 3x3 convolutions (conv1 -> act1 -> conv2 -> + residual -> act2: a residual block of LocalStage) with the
 * intermediate 6x6 map kept in registers between conv1's output transform and conv2's input transform. */
size_t be_wino_pair_workspace_floats(int64_t n, int cin, int cmid, int cout);
int be_wino_conv3x3_pair_6x6_f32(const float* x, const float* packed_w1, const float* packed_bias1, int act1,
                                 const float* packed_w2, const float* packed_bias2, const float* residual, int act2, float* y,
                                 int64_t n, int cin, int cmid, int cout, float* workspace, size_t workspace_floats, void* stream);
/* The same block as a link of a chain that shares ONE workspace.  x_in_v != 0: the start of the workspace already holds x's input
 * transform in this block's layout (left by the link in front), which is not computed again.  next_cmid > 0: besides y, the input
 * transform of y for a following block whose first convolution has next_cmid outputs is left at the start of the workspace; refused
 * when those positions * tiles * n * cout floats would reach past 100 n max(cin, cmid), where this block's own buffers start.
 * be_maxpool_wino_in_11x11_f32 heads a chain: the 3/2/1 max-pool of [n,11,11,c] -> pooled [n,6,6,c] (be_maxpool_nhwc_f32's bits) and
 * the input transform of the pooled map at the start of the workspace (positions * tiles * n * c floats; c %% 32 == 0).
 * Results are those of the unchained calls bit for bit. */
int be_wino_conv3x3_pair_chain_6x6_f32(const float* x, const float* packed_w1, const float* packed_bias1, int act1,
                                       const float* packed_w2, const float* packed_bias2, const float* residual, int act2, float* y,
                                       int64_t n, int cin, int cmid, int cout, float* workspace, size_t workspace_floats, void* stream,
                                       int x_in_v, int next_cmid);
int be_maxpool_wino_in_11x11_f32(const float* x, float* pooled, int64_t n, int c, int next_cmid, float* workspace,
                                 size_t workspace_floats, void* stream);

/* A residual block's 1x1 downsample inside conv2's transform-domain GEMMs (round 14).  A 1x1 kernel is a 3x3 with only the centre
 * tap; its kernel transform is non-zero at be_wino_ds_positions() of the positions (18 of the 40 with the 8x5 tiles: 5 zr + zc with
 * zr neither first nor last, zc in 1..3), and there conv2's GEMMs run on over the transform of the block's INPUT, into the same
 * accumulator: M[z] = V_h[z] U2[z]^T + V_x[z] U_ds[z]^T, K order V_h ascending, then V_x ascending.  No residual tensor is written or
 * read; the downsample's rounding is that of a Winograd layer instead of a row GEMM's.
 * be_wino_ds_pack_f32: w [cout,cin] (+ bias, + eval BatchNorm, folded as be_wino_pack_f32 does) -> packed_ds = U_ds
 * [positions'][cout_pad32][cin] fp32 (be_wino_pack_f32's arithmetic on the centre-tap kernel, live position 5 zr + zc at number
 * 3 (zr - 1) + zc - 1) followed by its hi / mid / lo bf16 planes in the GEMM's block layout (be_wino_ds_packed_floats; cin %% 16 == 0);
 * the folded bias [cout_pad32] goes to packed_bias unless that is NULL (the caller adds it to conv2's).
 * be_wino_conv3x3_pair_ds_6x6_f32: be_wino_conv3x3_pair_chain_6x6_f32 with packed_ds in place of the residual.  The workspace has
 * three regions (x's transform, M, conv1's transform: be_wino_pair_ds_workspace_floats); x may be NULL with x_in_v, and y with
 * next_cmid > 0 (the map is then not stored).  Requires the two transforms in one layout (always so when cmid == cout); refused under
 * BE_WINO_F32=1.  Bits depend on neither the batch nor BE_WINO_ZGROUPS.
 * be_wino_gemms_ext_f32: the GEMMs alone.  V [positions][tiles][cin] (tile_major 0) or [tiles][positions][cin] (1), tiles =
 * (12 / be_wino_tile_rows()) n; M and Vx (cin_ext channels, NULL: no second segment) likewise; packed_w of be_wino_pack_f32. */
int be_wino_ds_positions(void);
size_t be_wino_ds_packed_floats(int cout, int cin);
int be_wino_ds_pack_f32(const float* w_oi, const float* bias, const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                        const float* bn_var, float bn_eps, int cout, int cin, float* packed_ds, float* packed_bias, void* stream);
size_t be_wino_pair_ds_workspace_floats(int64_t n, int cin, int cmid, int cout);
int be_wino_conv3x3_pair_ds_6x6_f32(const float* x, const float* packed_w1, const float* packed_bias1, int act1,
                                    const float* packed_w2, const float* packed_bias2, const float* packed_ds, int act2, float* y,
                                    int64_t n, int cin, int cmid, int cout, float* workspace, size_t workspace_floats, void* stream,
                                    int x_in_v, int next_cmid);
int be_wino_gemms_ext_f32(const float* V, const float* packed_w, float* M, int64_t n, int cin, int cout, const float* Vx,
                          const float* packed_ds, int cin_ext, int tile_major, void* stream);

/* Row GEMM in the same split-bf16 arithmetic (bf16x6): y[m][ldy] = act(x[m][k] w^T + bias (+ residual)), act 0 none / 1 Smish / 2 ReLU,
 * residual with y's row stride; bias and residual may be NULL.  LocalStage's 1x1 downsamples of layers 1-3 and fc.1 run on it wherever
 * the Winograd path runs; environment BE_ROWS_F32=1 (read once per process) sends those four back to the fp32 kernels (BE_WINO_F32=1 does
 * too).  One kernel body for every m >= 1: a row's bits do not depend on the batch it is computed in.  be_gemm_rows_bf6_pack_f32 reads
 * a packed fp32 matrix [cout_pad32][cin] (be_conv_pack_f32 of a 1x1 convolution or linear) and writes its hi / mid / lo bf16 planes:
 * be_gemm_rows_bf6_packed_floats = 1.5 x cout_pad128 x cin floats (0 unless cin %% 16 == 0).  x, packed_w and planes 16-byte aligned. */
size_t be_gemm_rows_bf6_packed_floats(int cout, int cin);
int be_gemm_rows_bf6_pack_f32(const float* packed_w, int cout, int cin, float* planes, void* stream);
int be_gemm_rows_bf6_f32(const float* x, int64_t m, int k, const float* planes, int n, const float* bias, const float* residual,
                         int act, float* y, int ldy, void* stream);

/* 3x3 convolution (pad 1) + bias + activation on NHWC maps, optionally with a 1x1 convolution of x2 appended to the K loop (the
 * ResidualBlock tail of be_conv_nhwc_fused2_f32; x2 NULL and cin2 0: the plain convolution), in the same split-bf16 arithmetic (bf16x6)
 * on a pixel-major kernel.  LocalStage's layer0 runs on it wherever the Winograd path runs; environment BE_L0_F32=1 (read once per
 * process) sends layer0 back to the fp32 kernels (BE_WINO_F32=1 does too).  One kernel body for every n >= 1: an image's bits do not
 * depend on the batch it is computed in.  Shapes: cout_pad32 == 96, cin %% 32 == 0, cin2 %% 16 == 0, h and w >= 3, 256 images spanning
 * < 2^32 bytes; others return BE_EINVAL before any launch.  be_conv3x3_pm_bf6_pack_f32 reads the packed fp32 matrix [96][9 cin + cin2]
 * of be_conv_pack_f32 / be_conv_pack_fused2_f32 and writes its hi / mid / lo bf16 planes in be_gemm_rows_bf6_pack_f32's block layout:
 * be_conv3x3_pm_bf6_packed_floats = 1.5 x 128 x (9 cin + cin2) floats (0 for unsupported shapes).  The bias is the packed fp32 bias.
 * x, x2, packed_w and planes 16-byte aligned. */
size_t be_conv3x3_pm_bf6_packed_floats(int cout, int cin, int cin2);
int be_conv3x3_pm_bf6_pack_f32(const float* packed_w, int cout, int cin, int cin2, float* planes, void* stream);
int be_conv3x3_pm_bf6_f32(const be_conv_desc* desc_host, const float* x, const float* x2, int cin2, const float* planes,
                          const float* packed_bias, float* y, int ldy, void* stream);

/* nn.MaxPool2d(k, stride, pad) on NHWC (models/local_stage.py:42-43). */
int be_maxpool_nhwc_f32(const float* x, float* y, int n, int h, int w, int c, int k, int stride, int pad,
                        void* stream);
/* The same pooling reading an input whose rows are ldx floats apart (a channel slice of a wider NHWC tensor). */
int be_maxpool_nhwc_ld_f32(const float* x, int ldx, float* y, int n, int h, int w, int c, int k, int stride, int pad,
                           void* stream);
/* [N,3,21,21] NCHW -> [N,21,21,4] NHWC with a zero 4th channel (input staging of conv1). */
int be_nchw3_to_nhwc4_f32(const float* x, float* y, int64_t n, int hw, void* stream);
/* The padded form of that staging for large batches: [N,h,wrow,4], image column c at padded column c + 3, zeros in the
 * other columns (wrow >= w + 7; LocalStage uses 28), so that the 8-pixel kernel rows of conv1 stay inside a row and the
 * pixel-major LDS-DMA kernel needs no zero-fill (be_conv_pm.hip).  models/local_stage.py:34-37. */
int be_nchw3_to_nhwc4p_f32(const float* x, float* y, int64_t n, int h, int w, int wrow, void* stream);
int be_view_to_nhwc4p_f32(const be_patch_view* view_host, int64_t patches_per_image, int64_t first, float* y, int64_t n,
                          int wrow, void* stream);
/* conv1 (7x7, pad 3, cin 4 = rgb + zero, cout 64) + folded BatchNorm + activation on that padded staging; weights as packed
 * by be_conv_pack_f32(ksize 7).  Bit-identical to be_conv_nhwc_f32 on the unpadded staging. */
int be_conv7x7_nhwc4p_f32(const be_conv_desc* d, const float* x, int wrow, const float* packed_w, const float* packed_bias,
                          float* y, int ldy, void* stream);
/* conv1 + folded BatchNorm + Smish + MaxPool2d(3, 2, 1) of LocalStage's head (models/local_stage.py:34-37,42,64-65) in ONE launch,
 * image-major: x4p [n,21,28,4] (the padded staging of be_nchw3_to_nhwc4p_f32 / be_view_to_nhwc4p_f32, wrow = 28), packed_w / bias =
 * the 7x7 pack of be_conv_pack_f32 (cout 64, K = 224), y [n,11,11,64].  A workgroup keeps whole images in LDS, the weights in
 * registers, and writes only the pooled map.  Bit-identical to be_conv7x7_nhwc4p_f32 (act 1) followed by be_maxpool_nhwc_f32(3,2,1). */
int be_conv7x7_pool_nhwc4p_f32(const float* x4p, int64_t n, const float* packed_w, const float* packed_bias, float* y, void* stream);
/* The same head in split-bf16 arithmetic (bf16x6: the image split to hi / mid / lo bf16 planes once, in LDS; the weights once per wave,
 * in registers; six v_mfma_f32_32x32x16_bf16 per 16-deep K chunk, fp32 accumulation).  Same arguments, same checks, same packed fp32
 * weights and bias: nothing new is packed.  One kernel body for every n >= 1: an image's bits do not depend on the batch it is
 * computed in.  Against a float64 reference it errs at most 2 x what be_conv7x7_pool_nhwc4p_f32 errs.  LocalStage takes it wherever
 * the Winograd path runs, at every sub-batch size; environment BE_C1_F32=1 (read once per process) restores the fp32 routing of
 * conv1 + pool (BE_WINO_F32=1 does too). */
int be_conv7x7_pool_bf6_nhwc4p_f32(const float* x4p, int64_t n, const float* packed_w, const float* packed_bias, float* y, void* stream);
/* Patches [first, first+n) of a view -> [n,21,21,4] (the staging be_local_stage_forward_view_f32 uses). */
int be_view_to_nhwc4_f32(const be_patch_view* view_host, int64_t patches_per_image, int64_t first, float* y,
                         int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * LocalStage training kernels (models/local_stage.py under autograd; local_training.py:103-108)
 *   Activations are NHWC matrices [M = N*H*W][C].  scratch: be_train_scratch_bytes() bytes, 16-byte aligned,
 *   reused by every call (stream-ordered).  All reductions are two-stage in a fixed order (no float atomics).
 * ------------------------------------------------------------------------------------------------- */
size_t be_train_scratch_bytes(void);
/* nn.BatchNorm2d/1d in train mode (+ optional residual add, + optional Smish): batch mean / biased variance per
 * channel, running stats updated with `momentum` and the unbiased variance (run_* may be NULL).
 * out = act((y-mean)*invstd*gamma + beta (+res)); s_in (may be NULL) receives the Smish input for the backward. */
int be_bn_train_fwd_f32(const float* y, const float* gamma, const float* beta, const float* res, float eps,
                        float momentum, float* run_mean, float* run_var, float* mean, float* invstd, float* s_in,
                        float* out, int M, int C, int act, void* scratch, size_t scratch_bytes, void* stream);
/* Backward of the above: ds = dout * smish'(s_in) (s_in NULL: ds = dout), dgamma = sum ds*xhat, dbeta = sum ds,
 * dy = gamma*invstd*(ds - dbeta/M - xhat*dgamma/M).  ds may alias dout; ds is also the gradient of `res`. */
int be_bn_train_bwd_f32(const float* dout, const float* s_in, const float* y, const float* mean, const float* invstd,
                        const float* gamma, float* ds, float* dy, float* dgamma, float* dbeta, int M, int C,
                        void* scratch, size_t scratch_bytes, void* stream);
/* out[c] = sum_r a[r][c] (conv / linear bias gradients). */
int be_col_sum_f32(const float* a, float* out, int M, int C, void* scratch, size_t scratch_bytes, void* stream);
/* Backward of nn.MaxPool2d on NHWC: the gradient goes to the first maximum of each window (PyTorch's rule). */
int be_maxpool_nhwc_bwd_f32(const float* x, const float* dout, float* dx, int n, int h, int w, int c, int k, int stride,
                            int pad, void* stream);
/* Weight gradient of a stride-1 "same" conv / a Linear (ksize 1 on a 1x1 image), fp32 MFMA, written in the
 * reference's parameter layout dw [cout][cin][k][k] (ksize 7: x is the NHWC4 staging, dw is [cout][3][7][7];
 * layout_chw_hw as in be_conv_pack_f32). */
int be_conv_wgrad_f32(const float* x, const float* dy, float* dw, int n, int h, int w, int cin, int cout, int ksize,
                      int layout_chw_hw, void* scratch, size_t scratch_bytes, void* stream);
/* Data gradient = be_conv_nhwc_f32 with the transposed, tap-mirrored weights packed by this function
 * (dx has `cin` channels; run the conv with desc.cin = cout, desc.cout = cin, act 0).  packed_bias: cin_pad32 zeros. */
size_t be_conv_dgrad_packed_floats(int cout, int cin, int ksize);
int be_conv_pack_dgrad_f32(const float* weight_oihw, int cout, int cin, int ksize, int layout_chw_hw, float* packed_w,
                           float* packed_bias, void* stream);
/* Last Linear (K -> J, J small): dx [M,K], dw [J,K], db [J] from x [M,K], w [J,K], dy [M,J]. */
int be_linear_small_bwd_f32(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int M,
                            int K, int J, void* stream);

/* One training UNIT of LocalStage = nn.Conv2d / nn.Linear -> nn.BatchNorm (batch statistics) [-> + residual] [-> Smish]
 * (models/local_stage.py:11-17, 20-28, 44-50 in train mode; the forward half of local_training.py:103) in three launches:
 * the convolution (desc->act is ignored; its K loop may be split), one kernel that sums the split-K slices with the bias
 * into y [M,cout] and forms the per-row-block column sums of y and y^2, and one that finishes the batch statistics in its
 * prologue (fixed order), updates run_mean / run_var (momentum, unbiased variance; may be NULL), stores mean / invstd [cout]
 * and writes out = act((y-mean)*invstd*gamma + beta (+res)); s_in (may be NULL) keeps the Smish input for the backward.
 * packed_w / packed_bias: be_conv_pack_f32 WITHOUT BatchNorm (the conv bias alone).  cout %% 32 == 0, cout <= 1024.
 * scratch: be_train_scratch_bytes() bytes. */
int be_train_unit_fwd_f32(const be_conv_desc* desc_host, const float* x, const float* packed_w, const float* packed_bias,
                          const float* gamma, const float* beta, const float* res, float eps, float momentum, float* run_mean,
                          float* run_var, float* y, float* mean, float* invstd, float* s_in, float* out, int act,
                          void* scratch, size_t scratch_bytes, void* stream);
/* Backward of that unit (the autograd graph under loss.backward(), local_training.py:106) in four launches (the weight-gradient
 * GEMM and the data-gradient convolution share one grid): ds = dout *
 * smish'(s_in) (s_in NULL: ds = dout; ds is also the residual's gradient) with its column sums; dgamma / dbeta and
 * dy = gamma*invstd*(ds - dbeta/M - xhat*dgamma/M) with the column sums of dy; the weight-gradient GEMM over x (desc = the
 * FORWARD shape; ksize 7: x is the NHWC4 staging and dw is [cout][3][7][7]; layout_chw_hw as in be_conv_pack_f32); the
 * data-gradient convolution through dgrad_packed_w / dgrad_packed_bias (be_conv_pack_dgrad_f32; both NULL with dx NULL when
 * no input gradient is wanted); and one kernel that sums the weight-gradient slices into dw (reference layout), the bias
 * gradient into db and the data-gradient slices (+ dx_add [M,cin] if not NULL: the other branch of a residual block) into dx. */
int be_train_unit_bwd_f32(const be_conv_desc* desc_host, const float* x, const float* dout, const float* s_in, const float* y,
                          const float* mean, const float* invstd, const float* gamma, const float* dgrad_packed_w,
                          const float* dgrad_packed_bias, const float* dx_add, int layout_chw_hw, float* ds, float* dy,
                          float* dgamma, float* dbeta, float* dw, float* db, float* dx, void* scratch, size_t scratch_bytes,
                          void* stream);
/* The same two entry points for TWO units that are independent of each other and share their input - the 3x3 convolution
 * (unit a) and the 1x1 downsample (unit b) of a ResidualBlock (models/local_stage.py:20-28): every launch of the single form
 * carries both units' workgroups (the two convolutions in one grid, the BatchNorm kernels with one grid slice per unit, one
 * closing kernel), each unit in its own part of the scratch regions.  Results are those of the single calls up to the regrouping
 * of fp32 partial sums on the shapes the balanced launch takes (below: where a tile's K loop is cut depends on how many problems
 * share the launch), and bit for bit with BE_NO_TRAIN_SK=1 in the environment.
 * Forward: both units produce the same [n,h,w,cout].  Backward: the units also share x and cin; a->dx receives the SUM of
 * both input gradients (what ResidualBlock's autograd node accumulates), b->dx [M,cin] is working space (contents
 * unspecified afterwards), dx_add must be NULL in both.  Shapes the merged launches do not take run one unit after the
 * other inside the call. */
typedef struct be_train_unit_fwd {
    be_conv_desc desc;
    const float *x, *packed_w, *packed_bias, *gamma, *beta, *res;
    float *run_mean, *run_var, *y, *mean, *invstd, *s_in, *out;
    int act;
} be_train_unit_fwd;
typedef struct be_train_unit_bwd {
    be_conv_desc desc;
    const float *x, *dout, *s_in, *y, *mean, *invstd, *gamma, *dgrad_packed_w, *dgrad_packed_bias, *dx_add;
    int layout_chw_hw;
    float *ds, *dy, *dgamma, *dbeta, *dw, *db, *dx;
} be_train_unit_bwd;
int be_train_unit_pair_fwd_f32(const be_train_unit_fwd* a, const be_train_unit_fwd* b, float eps, float momentum,
                               void* scratch, size_t scratch_bytes, void* stream);
int be_train_unit_pair_bwd_f32(const be_train_unit_bwd* a, const be_train_unit_bwd* b, void* scratch, size_t scratch_bytes,
                               void* stream);
/* Round 6: the matrix work of the four entry points above - forward convolutions, weight-gradient GEMMs, data-gradient
 * convolutions - runs as ONE persistent, balanced launch per call (csrc/be_train_sk.h: every problem lays its tiles end to end on
 * an axis of K chunks, workgroup g takes the chunks [g Q, (g + 1) Q)) for the units it takes, forward and backward alike: ksize
 * 1 | 3, cin and cout multiples of 32 and >= 64 (the forward: any cin that is a multiple of 32), n a multiple of 64, maps of at
 * most 11 x 11 (ksize 3: at least 3 x 3), h = w = 1 included (fc.1), backward: an input gradient wanted (every unit of
 * models/local_stage.py:38-50 behind conv1 at batch 64 k, local_training.py:103-106).  Other shapes, and everything with
 * BE_NO_TRAIN_SK=1 in the environment, take rounds 3-5's equal-slice launches.  The number of workgroups is the device's CU count
 * x 3 (BE_SK_SLOTS), and it decides where the K loops are cut: results depend on the CU count in the grouping of their fp32
 * partial sums, and are reproducible bit for bit on one device.
 * This call is the HOST-ONLY inspection hook of that launch's planner (no GPU, no launch): it runs the planner the entry points
 * run for the unit a (b NULL) or the pair a, b (the same [n,h,w,cout]; backward: the same cin too) - forward != 0: the forward
 * convolutions, else the backward - on `slots` workgroup slots (rounded down to a multiple of 8, >= 8) with conv_bytes /
 * wgrad_bytes of scratch for the convolution / weight-gradient slices, then walks the plan as the kernel does.  Per segment six
 * ints are written to seg (at most cap segments): problem, tile, first chunk, last chunk + 1, slice, slices of that tile; per
 * problem four to problems (room for 4 x 4): first workgroup, workgroups, quota, chunks.  Problems are numbered in the launch's
 * order: the units' weight gradients, then their convolutions (one backward unit: 0 and 1; forward: convolutions only).
 * Returns the segment count, BE_EINVAL for a unit the launch does not take, BE_EWORKSPACE where the planner declines ("not
 * mine": a region holds fewer than two slices of a tile). */
int be_train_sk_plan_debug(const be_conv_desc* a, const be_conv_desc* b, int forward, int slots, size_t conv_bytes,
                           size_t wgrad_bytes, int* seg, int cap, int* problems);

/* Parameter gradients of y = x W^T + b over many rows (the linears of GlobalStage in training, global_training.py:207-213 under
 * autograd): dw [cout,cin] = dy^T x and db [cout] = column sums of dy, in two launches (weight-gradient tiles + column-sum
 * workgroups in one grid, then one reduction kernel; fixed order).  cin, cout multiples of 128, M >= 256 rows. */
int be_linear_param_grads_f32(const float* x, const float* dy, float* dw, float* db, int M, int cin, int cout, void* scratch,
                              size_t scratch_bytes, void* stream);
/* Last Linear forward (K -> J, J small; models/local_stage.py:50): y [M,J] = x [M,K] w [J,K]^T + b, raw parameter layout. */
int be_linear_small_fwd_f32(const float* x, const float* w, const float* b, float* y, int M, int K, int J, void* stream);
/* nn.MaxPool2d forward on NHWC that also records the winning window element (dy*k + dx of the FIRST maximum, one byte per
 * output value; idx 4-byte aligned, c %% 4 == 0), and the backward that routes dout through those bytes. */
int be_maxpool_nhwc_fwd_idx_f32(const float* x, float* y, unsigned char* idx, int n, int h, int w, int c, int k, int stride,
                                int pad, void* stream);
int be_maxpool_nhwc_bwd_idx_f32(const unsigned char* idx, const float* dout, float* dx, int n, int h, int w, int c, int k,
                                int stride, int pad, void* stream);

/* Tail of a training step (local_training.py:107-108): torch.nn.utils.clip_grad_norm_(max_norm, 2) + torch.optim.AdamW.step()
 * for parameters whose gradients are slices of ONE flat buffer (what the LocalStage backward writes), in two launches: squared-
 * norm partials (fp64; this launch also counts the step), the update.  table (device): one entry per workgroup, at most be_adam_chunk() elements
 * each: parameter / exp_avg / exp_avg_sq pointers, offset of the slice in grad_flat, count.  grad_scale multiplies the gradient
 * first (1/world after a summing all-reduce).  max_norm <= 0: no clipping.  step_device: float scalar = steps taken so far
 * (incremented here); grad_norm_out (may be NULL): the norm before clipping.  write_back: store the scaled + clipped gradient
 * back (clip_grad_norm_ modifies .grad in place).  partial: npartial_cap >= ceil(n_flat / be_adam_chunk()) doubles. */
typedef struct be_adam_entry {
    float *p, *m, *v;
    int64_t goff;
    int n;
} be_adam_entry;
int be_adam_chunk(void);
int be_clip_adamw_f32(const be_adam_entry* table_device, int nentries, float* grad_flat, int64_t n_flat, double* partial,
                      int npartial_cap, float max_norm, float grad_scale, double lr, double beta1, double beta2, double eps,
                      double weight_decay, float* step_device, float* grad_norm_out, int write_back, void* stream);
/* Final reduction of be_local_loss_f32's per-patch partials [B,3] into the scalar of LocalLoss.forward (local_training.py:47-52):
 * loss = S0/(441 B) + beta_bndry S1/(441 B) + beta_smooth S2/(361 B), sums in fp64 in patch order. */
int be_local_loss_finish_f32(const float* partial, int B, float beta_bndry, float beta_smooth, float* loss_out, void* stream);

/* eval_depth (utils/metrics.py:3-20) on the device: pred, gt [B,H,W]; a pixel counts when mask_src > 0 (the scripts pass
 * the estimated depth map itself, blurry_edges_test.py:148); crop pixels dropped on every side; out5 (device, float64) =
 * delta1, delta2, delta3, RMSE in cm, AbsRel in cm, summed jointly over the batch as the reference does. */
int be_eval_depth_f32(const float* pred, const float* gt, const float* mask_src, int B, int H, int W, int crop, float tau_n,
                      float z_min, float z_max, double* out5, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Depth-completion U-Net glue ('--densify pp', models/depth_completion_unet.py:79-113; blurry_edges_test.py:141-142).
 * Its convolutions are be_conv_nhwc_f32 launches (3x3 + folded BatchNorm + ReLU; ConvTranspose2d(k=2,s=2) as a 1x1
 * convolution with 4*cout outputs ordered (dy,dx,co)); these two do the layout work around them.
 * ------------------------------------------------------------------------------------------------- */
/* x [N,C,HW] NCHW -> y [N,HW,cpad] NHWC, channels C..cpad-1 zero. */
int be_nchw_to_nhwc_pad_f32(const float* x, float* y, int64_t n, int c, int64_t hw, int cpad, void* stream);
/* Pixel shuffle of the transposed convolution into the decoder's concatenated input: t [N,h,w,4*cout] ->
 * y[n, 2i+dy+top, 2j+dx+left, ch_off+co] of an [N,oh,ow,ldy] tensor (top/left = F.pad offsets diff//2, :63-65;
 * positions outside are dropped; the caller zero-fills the padding border once). */
int be_upconv2x2_scatter_f32(const float* t, float* y, int64_t n, int h, int w, int cout, int oh, int ow, int top, int left,
                             int ldy, int ch_off, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * GlobalStage encoder pieces, inference (nn.TransformerEncoderLayer of models/global_stage.py:28-32; the linears
 * run on be_conv_nhwc_f32 as 1x1 convs)
 * ------------------------------------------------------------------------------------------------- */
/* Multi-head self-attention with head dim 16: qkv [B*L, 3*H*16] (rows = tokens, columns q|k|v as
 * nn.MultiheadAttention's in_proj produces them) -> out [B*L, H*16] = softmax(q k^T / 4) v per head.
 * workspace: be_attention_workspace_floats(B,L,H) floats.  L % 128 == 0; l_valid in (L - 128, L]: the number of real
 * tokens when the caller padded the sequence up to L (keys >= l_valid get probability exactly 0; output rows >= l_valid
 * are computed and meaningless).  nn.TransformerEncoder takes any L <= max_len^2 (models/global_stage.py:18-20). */
size_t be_attention_workspace_floats(int B, int L, int H);
int be_attention_f32(const float* qkv, float* out, float* workspace, int B, int L, int l_valid, int H, void* stream);
/* y = LayerNorm(x + res) over the last dimension D in {64,128,192,256}; res may be NULL; y may alias x. */
int be_add_layernorm_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y,
                         int64_t rows, int D, float eps, void* stream);
/* x[b] += pe for b < batches (PositionalEncoding.forward, models/global_stage.py:18-20); per_batch = L*D floats. */
int be_add_pe_f32(float* x, const float* pe, int64_t batches, int64_t per_batch, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * GlobalStage encoder, training (model.train() of global_training.py:207-213: dropout 0.1 at the four sites of
 * nn.TransformerEncoderLayer, autograd through every layer).  Dropout is counter-based: element i of site `site` is
 * kept iff hash(i, seed, site) >= p * 2^32, so the backward kernels re-derive the masks and nothing is stored.
 * ------------------------------------------------------------------------------------------------- */
/* Attention forward for training: out as be_attention_f32 with dropout on the probabilities (site = batch*H + head,
 * element = query*L + key), lse [B*H, L] = log2-sum-exp of each score row (saved for the backward).  The workspace keeps, for
 * the backward call of the same layer, the split q / k / v and one keep bit per probability (B*H*L*L/8 bytes, from float
 * offset be_attention_train_keep_offset_floats on: [B*H][L/32 query tiles][L/32 key blocks][64 lanes] halfwords). */
size_t be_attention_train_workspace_floats(int B, int L, int H);
int be_attention_train_fwd_f32(const float* qkv, float* out, float* lse, float* workspace, int B, int L, int l_valid, int H,
                               float dropout_p, uint32_t seed, void* stream);
/* Attention backward: dout [B*L, H*16] -> dqkv [B*L, 3*H*16]; probabilities are recomputed from qkv and lse
 * (no [L,L] float tensor is ever stored); deterministic (no atomics).  Same workspace size as the forward; `scratch`
 * (be_attention_bwd_scratch_floats floats, contents irrelevant before and after the call: one buffer can serve every layer)
 * receives the partial dQ sums of the key groups.
 * operands_ready != 0: `workspace` is the buffer the forward call of this layer used and nothing wrote to it since
 * (its split q/k/v and keep bits are reused); 0: they are produced again from qkv and the seed.  l_valid as in be_attention_f32: rows >= l_valid of
 * dout must be zero (they are when the caller slices the padded output), and dqkv comes out zero there. */
size_t be_attention_bwd_scratch_floats(int B, int L, int H);
int be_attention_bwd_f32(const float* qkv, const float* out, const float* lse, const float* dout, float* dqkv,
                         float* workspace, float* scratch, int operands_ready, int B, int L, int l_valid, int H, float dropout_p,
                         uint32_t seed, void* stream);
/* The keep mask the two functions above apply, [B*H, L, L] in {0,1} (test hook; small L only). */
int be_attention_dropout_mask_f32(float* mask, int B, int L, int H, float dropout_p, uint32_t seed, void* stream);
/* The same decisions in the packed layout the forward leaves in its workspace (B*H*L*L/16 halfwords), from the formula:
 * what be_attention_bwd_f32 regenerates when operands_ready == 0, and what the tests compare the forward's stores with. */
size_t be_attention_train_keep_offset_floats(int B, int L, int H);
int be_attention_keep_bits_u16(uint16_t* keep, int B, int L, int H, float dropout_p, uint32_t seed, void* stream);
/* y = dropout(x) = x * keep / (1-p); with gate != NULL additionally zero where gate <= 0, which makes it the
 * backward of dropout(relu(.)) given the ReLU output.  y may alias x.  n < 2^32. */
int be_dropout_f32(const float* x, const float* gate, float* y, int64_t n, float dropout_p, uint32_t seed, uint32_t site,
                   void* stream);
/* v = res + dropout(x) (stored), y = LayerNorm(v); D = 128; res may be NULL. */
int be_add_layernorm_train_f32(const float* x, const float* res, const float* gamma, const float* beta, float* v, float* y,
                               int64_t rows, int D, float eps, float dropout_p, uint32_t seed, uint32_t site, void* stream);
/* LayerNorm backward from the stored v: dv (gradient of v, hence of the residual input; NULL to skip),
 * dx = dropout'(dv) (gradient of the dropped branch; NULL to skip), partial [be_layernorm_bwd_partial_floats]:
 * per-block sums of (dy*xhat | dy) as rows of 2*D floats - be_col_sum_f32 over them gives dgamma | dbeta. */
size_t be_layernorm_bwd_partial_floats(int64_t rows, int D);
int be_layernorm_bwd_f32(const float* dy, const float* v, const float* gamma, float* dv, float* dx, float* partial,
                         int64_t rows, int D, float eps, float dropout_p, uint32_t seed, uint32_t site, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Synthetic-shape training data (train_val_data_generator.py:31-275).  float64 throughout, the
 * reference's array layouts.  shape [N,maxo,10] int32 = (kind 0 circle | 1 rectangle | 2 triangle, vertex count,
 * x0,y0..x3,y3; circle: x0,y0 centre, x1 radius), prop [N,maxo,4] = (depth, c0,c1,c2), objects far -> near,
 * nobj [N], bg [N,3], sig [N,maxo,2] PSF radius in pixels per aperture (utils/data_generator.py:16-17).
 * N < 65536, maxo <= 32.
 * ------------------------------------------------------------------------------------------------- */
/* Rasterisation (cv2.circle / cv2.drawContours of train_val_data_generator.py:58-76, thickness -1 and 1): two bit planes per
 * object, FILL and RING, masks [N][maxo][2][H][ceil(W/32)] uint32 (be_datagen_raster_words of them; bit x & 31 of word x >> 5).
 * The planes follow the algorithms those calls run in OpenCV 4.x modules/imgproc/src/drawing.cpp: Circle() (midpoint walk),
 * Line() = clipLine() + the 8-connected LineIterator from the left end point, CollectPolyEdges() + FillEdgeCollection() (16.16
 * fixed-point edges, active for y0 <= y < y1, runs from ceil(x_left) to floor(x_right)).  Objects >= nobj[i] get empty planes. */
size_t be_datagen_raster_words(int n, int H, int W, int maxo);
int be_datagen_raster_u32(const int* shape, const int* nobj, int n, int H, int W, int maxo, uint32_t* masks, void* stream);
/* aif [N,H,W,3] (colour / 255, as images_aif is stored, :137), bloc [N,H,W] (0/255), idep, bdep [N,H,W]  (:36-41,77-85,100-103);
 * masks: the planes be_datagen_raster_u32 wrote. */
int be_datagen_scene_f64(const uint32_t* masks, const double* prop, const int* nobj, const double* bg, int n, int H, int W,
                         int maxo, double z_far, double* aif, double* bloc, double* idep, double* bdep, void* stream);
/* imgs [N,2,H,W,3]: background, then every object (its FILL plane) blurred with its PSF per aperture and alpha-composited (:87-94). */
size_t be_datagen_blur_scratch_bytes(int n, int H, int W);
int be_datagen_blur_composite_f64(const uint32_t* masks, const double* prop, const int* nobj, const double* bg, const double* sig,
                                  int n, int H, int W, int maxo, int max_nobj, double* imgs, void* scratch,
                                  size_t scratch_bytes, void* stream);
/* imgs <- round(imgs); bdist [N,H,W] city-block distance to the nearest bloc > 0 pixel (ones when there is none);
 * deri [N,2,H,W,3] Sobel magnitude / 255 with reflected borders (:105-123).  scratch >= N*H*W*4 bytes. */
int be_datagen_finish_f64(double* imgs, const double* bloc, double* bdist, double* deri, int n, int H, int W, void* scratch,
                          size_t scratch_bytes, void* stream);
/* gt = imgs/255*alpha, ny = round(clip(Poisson(gt) + sigma*N(0,1), 0, alpha)) (:165-182); alpha [n], per_sample =
 * elements per alpha; counter-based streams keyed by (seed, element). */
int be_datagen_noise_f64(const double* imgs, const double* alpha, double sigma, uint32_t seed, int64_t n, int64_t per_sample,
                         double* gt, double* ny, void* stream);
/* cand [N,H,W] uint8: 1 where a boundary pixel lies within `reach` (Chebyshev) and the pixel is >= margin from every
 * image border (:214-218). */
int be_datagen_candidates_f64(const double* bloc, unsigned char* cand, int n, int H, int W, int reach, int margin, void* stream);
/* R x R crops centred on flat pixel indices pick[i] (into [N,H,W]; must respect the margin R/2) of aperture aper[i]:
 * in6 = aif [N,H,W,3], gt, ny, deri [N,2,H,W,3], idep, bdep [N,H,W]; out9 = aif, gt, ny, deri [P,R,R,3], idep, bdep,
 * bloc, bdist (in-patch city-block distance) [P,R,R], alpha [P]  (:226-252). */
int be_datagen_crop_f64(const double* const* in6, const double* bloc, const double* alpha, const int64_t* pick, const int* aper,
                        int64_t n_patch, int n, int H, int W, int R, double* const* out9, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Textured test set (test_data_generator.py:87-121, render_layer + render_image): the layered defocus render, float64, both
 * apertures.  L = n_interval + 1 depth layers per layer set (set 0 background, set 1 foreground object + mask); keys [N,2,L] =
 * np.linspace(max, min, L) of each set's depth plane (:116-117; the foreground's over its mask); layer weights are the hat functions
 * of :95-102 evaluated in the reference's operation order; each layer is a scipy.ndimage.convolve(mode='reflect') with its PSF
 * (taps in row-major order, |w| <= DBL_EPSILON skipped, no contraction).  bkgd, frgd [N,H,W,3] (BGR, 0..255), mask [N,H,W] (0/1),
 * depth_bg, depth_fg [N,H,W].  psf: per (image, set, aperture, layer) one (2*kmax+1)^2 slot holding the layer's (2k+1)^2 kernel
 * (utils/data_generator.py:19-23) centred in it, k = psf_k [N,2,2,L] (clamped to kmax on the device); psf_len (doubles) must be at
 * least be_datagen_test_psf_doubles(N, n_interval, kmax).  Outputs img_clean [N,2,H,W,3] = bg * (1 - m) + fg, mask_blur [N,2,H,W]
 * = m (clipped to [0, 1]).  all_layers = 1 adds every layer's term (the reference's full sum; checking only).  N <= 32767, kmax <= 64;
 * N = 0 launches nothing. */
size_t be_datagen_test_psf_doubles(int n, int n_interval, int kmax);
int be_datagen_test_render_f64(const double* bkgd, const double* frgd, const double* mask, const double* depth_bg,
                               const double* depth_fg, const double* keys, const double* psf, const int* psf_k, size_t psf_len,
                               int kmax, int n, int H, int W, int n_interval, int all_layers, double* img_clean, double* mask_blur,
                               void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py's roofline leg): opt-in hipEvent pair around every matrix-kernel launch and around the
 * HBM-bound kernels of the LocalStage / pass-A step, recorded on
 * the launch stream.  be_profile_enable(0) turns it off and frees the events.  Not thread-safe.
 * ------------------------------------------------------------------------------------------------- */
#define BE_KERNEL_CONV_128x128      0   /* k_conv_igemm<2,2,2,2,TAPS>: layers 1-3 + fc.1 (the dominant kernel) */
#define BE_KERNEL_CONV_128x96       1   /* layer0                                                              */
#define BE_KERNEL_CONV_128x64       2
#define BE_KERNEL_CONV_128x32       3   /* fc.4                                                                */
#define BE_KERNEL_CONV_ROW8_128x64  4   /* conv1 (7x7 row-gather)                                              */
#define BE_KERNEL_CONV_SMALL        5   /* 64x64 / 128x32 tiles for small M (training batches)                 */
#define BE_KERNEL_WINO_GEMM         6   /* k_wino_gemm_ps<0, 0> (split bf16; fp32: k_wino_gemm_ws / k_wino_gemm): the transform-domain GEMMs (one per position) of a Winograd layer, with a block's 1x1 downsample as a second K segment where it is folded in (k_wino_gemm_ps<0, 0, 1>); FLOPs as fp32 products */
#define BE_KERNEL_GEMM_ROWS         7   /* row GEMMs: k_wino_gemm_ps<EPI> on pre-split weights (split bf16: fc.1, and LocalStage's 1x1 downsamples under BE_WINO_DS_GEMM=1; FLOPs as fp32 products); fp32: k_wino_gemm<1> / k_wino_gemm_ws<.., 1> (1x1 convolutions / linears, large batches) */
/* HBM-bound kernels: `bytes` = the algorithmic bytes the launch has to move, `flops` = 0 */
#define BE_KERNEL_WINO_TRANSFORM    8   /* k_wino_in / k_wino_out / k_wino_out_in / k_wino_out_pool2 */
#define BE_KERNEL_MAXPOOL           9   /* k_maxpool_nhwc */
#define BE_KERNEL_RENDER_COLORS    10   /* k_render_colors (pass A: wedges + ridge colour solve) */
#define BE_KERNEL_STAGING          11   /* NCHW / image view -> NHWC4 staging of conv1's input */
#define BE_KERNEL_TRAIN_BWD_GEMMS  12   /* k_unit_gemms / k_unit_gemms_sk: training units' weight-gradient GEMMs + data-gradient convolutions (one or two units), a block's two forward convolutions: one launch */
#define BE_KERNEL_CONV1_POOL       13   /* k_conv1_pool: conv1 7x7 + Smish + the first max-pool, image-major (bytes: staging in, pooled 11x11x64 map out) */
int be_profile_enable(int max_launches);
int be_profile_reset(void);
/* Waits for the recorded events; fills up to cap records (launch order); returns the number filled (>= 0)
 * or a negative error.  flops/bytes = ALGORITHMIC work of the launch (the convolution's 2*MAC with the unpadded K,
 * zero-padding taps included as the reference counts them; in+weights+out bytes); flops_executed (may be NULL) =
 * the MFMA work actually issued (tile padding included, taps outside the image skipped). */
int be_profile_read(int* kernel_id_host, double* flops_host, double* bytes_host, double* flops_executed_host,
                    float* ms_host, int cap);

#ifdef __cplusplus
}
#endif
#endif /* BLURRY_EDGES_HIP_H */
