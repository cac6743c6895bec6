// Textured test set on the GPU: the layered defocus render of test_data_generator.py:87-121 (render_layer + render_image),
// float64, for a batch of images and both apertures.
//
// The reference blurs every one of the n_interval+1 depth layers with a full-image scipy.ndimage.convolve(mode='reflect') per
// aperture and per layer set (background; foreground object + its mask), then sums the layers under hat weights.  At one pixel
// only the one to three layers whose hat covers its depth carry a nonzero weight, so k_layered_render evaluates the weights of
// a small window of layers around the arithmetic estimate (the reference's comparisons and formulas, its operation order) and
// convolves only where the weight is nonzero.  Adding the reference's zero terms would not change a bit: the accumulators start
// at +0 and every product is >= +0 or -0.  all_layers = 1 instead adds every layer's term, the reference's full-sum form (a
// checking mode, ~50x the arithmetic).
//
// Bit-exactness with scipy's NI_Correlate on a symmetric kernel: taps in row-major order of input offsets (dy = -k..k, then
// dx = -k..k) accumulated from 0.0, taps with |w| <= DBL_EPSILON skipped, multiply and add rounded separately (contraction off
// below), the half-sample symmetric 'reflect' index map with period 2n (a kernel wider than the image is still right).
//
// One thread per (pixel, aperture, image); 16x16 pixel tiles.  The input planes are read through the caches (the image and the
// few PSFs a tile touches stay resident); no LDS staging: the measured time is in DESIGN.md section 6b.
#include "be_common.h"
#include <cfloat>

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 16;
constexpr int KMAX_LIMIT = 64;        // PSF radius cap the entry accepts (the default camera needs 17)
constexpr int WINDOW = 2;             // layers evaluated each side of the estimate: covers |t - j| < 1 + ulps

// scipy.ndimage 'reflect' (half-sample symmetric): ... 1 0 | 0 1 .. n-1 | n-1 n-2 ..., period 2n
__device__ __forceinline__ int reflect_index(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n <= 1) return 0;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// render_layer's weight of layer j at depth dm (test_data_generator.py:95-102), the reference's operations in its order:
// mask_last = (dm <= depth - diff) & (dm > depth), mask_next = (dm <= depth) & (dm > depth + diff); the boolean masks multiply
// as 0.0 / 1.0.
__device__ __forceinline__ double hat_weight(double dm, double depth, double diff, int j, int last) {
    const double ml = (dm <= depth - diff && dm > depth) ? 1.0 : 0.0;
    const double mn = (dm <= depth && dm > depth + diff) ? 1.0 : 0.0;
    if (j == 0) return (dm > depth ? 1.0 : 0.0) + (dm - depth - diff) / (-diff) * mn;
    if (j == last) return (depth - diff - dm) / (-diff) * ml + (dm <= depth ? 1.0 : 0.0);
    return (depth - diff - dm) / (-diff) * ml + (dm - depth - diff) / (-diff) * mn;
}

// the layers [lo, hi] whose weight can be nonzero at depth dm: keys run from keys[0] (max) down to keys[last] (min)
__device__ __forceinline__ void layer_window(double dm, const double* keys, int last, int& lo, int& hi) {
    const double span = keys[0] - keys[last];
    double t = span > 0.0 ? (keys[0] - dm) / span * (double)last : 0.0;
    t = fmin(fmax(t, -2.0), (double)last + 2.0);
    const int f = (int)floor(t);
    lo = max(f - WINDOW, 0);
    hi = min(f + WINDOW + 1, last);
}

struct RenderArgs {
    const double* bkgd; const double* frgd; const double* mask;       // [n,H,W,3] [n,H,W,3] [n,H,W]
    const double* depth_bg; const double* depth_fg;                   // [n,H,W]
    const double* keys;                                               // [n,2,L]   set 0 background, 1 foreground
    const double* psf; const int* psf_k;                              // [n,2,2,L,S,S]  [n,2,2,L]   (set, aperture, layer)
    double* img_clean; double* mask_blur;                             // [n,2,H,W,3]  [n,2,H,W]
    int H, W, L, K, all_layers;
};

// sum over the kernel's taps of img[reflect(y+dy), reflect(x+dx), c] * w(dy, dx) for C channels (+ the mask plane when M)
template <int C, bool M>
__device__ __forceinline__ void convolve_at(const double* __restrict__ img, const double* __restrict__ msk, int H, int W, int y,
                                            int x, const double* __restrict__ ker, int S, int K, int k, double* acc) {
    for (int c = 0; c < C + (M ? 1 : 0); ++c) acc[c] = 0.0;
    for (int dy = -k; dy <= k; ++dy) {
        const int yy = reflect_index(y + dy, H);
        const double* row = img + (size_t)yy * W * C;
        const double* mrow = M ? msk + (size_t)yy * W : nullptr;
        const double* krow = ker + (size_t)(dy + K) * S + K;
        for (int dx = -k; dx <= k; ++dx) {
            const double w = krow[dx];
            if (fabs(w) <= DBL_EPSILON) continue;
            const int xx = reflect_index(x + dx, W);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = acc[c] + row[(size_t)xx * C + c] * w;
            if (M) acc[C] = acc[C] + mrow[xx] * w;
        }
    }
}

__global__ void __launch_bounds__(TILE * TILE) k_layered_render(RenderArgs a) {
    const int x = blockIdx.x * TILE + threadIdx.x, y = blockIdx.y * TILE + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const int img = blockIdx.z >> 1, ap = blockIdx.z & 1;
    const int H = a.H, W = a.W, L = a.L, K = a.K, S = 2 * a.K + 1, last = a.L - 1;
    const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
    double out[2][4];                               // [set][channels | mask]: background c0..c2, foreground c0..c2 + mask
    for (int s = 0; s < 2; ++s) {
        const double* keys = a.keys + ((size_t)img * 2 + s) * L;
        const double diff = keys[1] - keys[0];
        const double dm = (s == 0 ? a.depth_bg : a.depth_fg)[img * plane + p];
        const double* src = (s == 0 ? a.bkgd : a.frgd) + img * plane * 3;
        const double* msk = a.mask + img * plane;
        const size_t tab = ((size_t)img * 2 + s) * 2 + ap;            // (image, set, aperture) row of the PSF tables
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        int lo = 0, hi = last;
        if (!a.all_layers) layer_window(dm, keys, last, lo, hi);
        for (int j = lo; j <= hi; ++j) {
            const double w = hat_weight(dm, keys[j], diff, j, last);
            if (w == 0.0 && !a.all_layers) continue;
            const double* ker = a.psf + (tab * L + j) * S * S;
            const int k = min(max(a.psf_k[tab * L + j], 0), K);
            double c[4];
            if (s == 0) {
                convolve_at<3, false>(src, nullptr, H, W, y, x, ker, S, K, k, c);
            } else {
                convolve_at<3, true>(src, msk, H, W, y, x, ker, S, K, k, c);
                acc[3] = acc[3] + c[3] * w;
            }
            for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + c[ch] * w;
        }
        for (int ch = 0; ch < 4; ++ch) out[s][ch] = acc[ch];
    }
    // render_image (:119): mask clipped to [0, 1], img_clean = bg * (1 - m) + fg
    const double m = fmin(fmax(out[1][3], 0.0), 1.0);
    const size_t o = ((size_t)img * 2 + ap) * plane + p;
    a.mask_blur[o] = m;
    for (int ch = 0; ch < 3; ++ch) a.img_clean[o * 3 + ch] = out[0][ch] * (1.0 - m) + out[1][ch];
}

}  // namespace

extern "C" size_t be_datagen_test_psf_doubles(int n, int n_interval, int kmax) {
    if (n < 0 || n_interval < 1 || kmax < 0) return 0;
    const size_t S = 2 * (size_t)kmax + 1;
    return (size_t)n * 4 * (size_t)(n_interval + 1) * S * S;
}

extern "C" int be_datagen_test_render_f64(const double* bkgd, const double* frgd, const double* mask, const double* depth_bg,
                                          const double* depth_fg, const double* keys, const double* psf, const int* psf_k,
                                          size_t psf_len, int kmax, int n, int H, int W, int n_interval, int all_layers,
                                          double* img_clean, double* mask_blur, void* stream) {
    BE_REQUIRE(n >= 0 && n <= 32767, "be_datagen_test_render_f64: n = %d outside [0, 32767]", n);
    BE_REQUIRE(n_interval >= 1, "be_datagen_test_render_f64: n_interval = %d < 1", n_interval);
    BE_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 28), "be_datagen_test_render_f64: bad image size %d x %d", H, W);
    BE_REQUIRE(kmax >= 0 && kmax <= KMAX_LIMIT, "be_datagen_test_render_f64: kmax = %d outside [0, %d]", kmax, KMAX_LIMIT);
    BE_REQUIRE(bkgd && frgd && mask && depth_bg && depth_fg && keys && psf && psf_k && img_clean && mask_blur,
               "be_datagen_test_render_f64: null pointer");
    BE_REQUIRE(all_layers == 0 || all_layers == 1, "be_datagen_test_render_f64: all_layers must be 0 or 1");
    const size_t need = be_datagen_test_psf_doubles(n, n_interval, kmax);
    BE_REQUIRE(psf_len >= need, "be_datagen_test_render_f64: PSF table of %zu doubles overruns (needs %zu)", psf_len, need);
    if (n == 0) return BE_OK;
    RenderArgs a{bkgd, frgd, mask, depth_bg, depth_fg, keys, psf, psf_k, img_clean, mask_blur, H, W, n_interval + 1, kmax, all_layers};
    const dim3 grid((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, 2 * n);
    hipLaunchKernelGGL(k_layered_render, grid, dim3(TILE, TILE), 0, be::as_stream(stream), a);
    return be::check_launch("be_datagen_test_render_f64");
}
