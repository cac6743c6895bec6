// Shared host-side helpers of libblurry_edges_hip (error reporting, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include "../../include/blurry_edges_hip.h"

namespace be {

char* last_error_buf();   // thread-local, 512 bytes

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(BE_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return BE_OK;
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// per-device caches (function attributes, CU counts) are indexed by the current device id: one process may drive several GPUs
constexpr int kMaxDevices = 64;
inline int current_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) d = 0;
    return d;
}

// First-call caches shared by host threads (ADVICE / VERDICT r2: the plain `static bool attr_set[]` arrays were written without
// synchronisation).  One atomic per device: two threads racing on their first call both set the (idempotent) function attribute
// and both publish the flag with release semantics; later calls are one acquire load.
struct DeviceFlags { std::atomic<int> v[kMaxDevices]; };
inline int ensure_dynamic_lds(const void* kernel, size_t lds_bytes, DeviceFlags& flags) {
    const int dev = current_device();          // the attribute is per device
    if (flags.v[dev].load(std::memory_order_acquire)) return BE_OK;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return fail(BE_ELAUNCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    flags.v[dev].store(1, std::memory_order_release);
    return BE_OK;
}
// CU count of the current device (256 on MI355X), cached per device
inline int device_cu_count() {
    static DeviceFlags cus{};
    const int dev = current_device();
    int c = cus.v[dev].load(std::memory_order_acquire);
    if (c > 0) return c;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    cus.v[dev].store(c, std::memory_order_release);
    return c;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// an A/B knob of the environment: set and not 0.  Callers keep the answer in a `static const`: a knob is read once per process
inline bool knob_on(const char* name) {
    const char* v = getenv(name);
    return v != nullptr && atoi(v) != 0;
}

// Opt-in per-launch timing (be_profile_* in the C ABI): when enabled, every conv launch is bracketed by two
// pre-created hipEvents recorded on the launch stream (asynchronous; read back later).
struct ProfileScope {
    ProfileScope(hipStream_t s, int kernel_id, double flops, double bytes, double flops_executed);
    ~ProfileScope();
    hipStream_t s_; int slot_;
};

// be_wino.hip: row GEMM on the LDS-DMA kernel (1x1 convolutions / linears of large batches); preconditions at the definition
int gemm_rows(const float* x, int64_t M, int K, const float* packed_w, int N, const float* bias, const float* res, int act,
              float* y, int ldy, void* stream);

// be_wino.hip: y[M][ldy] = x[M][K] w[Npad][K]^T, RAW accumulators (no bias, no activation) on the weight-stationary GEMM kernel;
// returns 1 when the shape is not one it takes (K in {96, 256, 384}, M % 128 == 0, >= 128 row tiles, N % 128 == 0)
int gemm_rows_ws(const float* x, int64_t M, int K, const float* packed_w, int N, float* y, int ldy, void* stream);
// be_wino.hip: the split-bf16 (bf16x6) row GEMM on the pre-split planes of w (be_gemm_rows_bf6_pack_f32), any M >= 1: the body of
// be_gemm_rows_bf6_f32.  rows_bf6_enabled(): false under BE_ROWS_F32=1 or BE_WINO_F32=1 (read once per process)
int gemm_rows_bf6(const float* x, int64_t M, int K, const float* planes, int N, const float* bias, const float* res, int act,
                  float* y, int ldy, void* stream);
bool rows_bf6_enabled();
// be_api.hip: a[i] += b[i], i < n (pack-time helper)
int vec_add_inplace(float* a, const float* b, int n, void* stream);

// be_conv_pm.hip: pixel-major LDS-DMA convolution for large batches (3x3 (+ fused 1x1 on x2), or the 7x7 conv1 on the padded
// staging with `wrow` pixels per row); returns 1 when the shape is not one it is built for.  conv_pm_takes: that question on its
// own (shape, 32-bit spans and the BE_NO_CONV_PM knob; no pointer, no device): be_conv.hip's planner routes by it
bool conv_pm_takes(const be_conv_desc* d, int wrow, bool fused, int cin2, int ldy);
int conv_pm(const be_conv_desc* d, const float* x, int wrow, const float* x2, int cin2, const float* pw, const float* pb,
            float* y, int ldy, int ktot, void* stream);

// be_conv_pm_bf6.hip: the pixel-major 3x3 convolution (+ fused 1x1 on x2) for cout_pad32 = 96 in split-bf16 arithmetic on the planes
// of be_conv3x3_pm_bf6_pack_f32, any n >= 1: the body of be_conv3x3_pm_bf6_f32 (LocalStage's layer0 on the Winograd path).
// l0_bf6_enabled(): false under BE_L0_F32=1 or BE_WINO_F32=1 (read once per process)
int conv3x3_pm_bf6(const be_conv_desc* d, const float* x, const float* x2, int cin2, const float* planes, const float* bias,
                   float* y, int ldy, void* stream);
bool l0_bf6_enabled();
// be_conv1_pool_bf6.hip: c1_bf6_enabled(): false under BE_C1_F32=1 or BE_WINO_F32=1 (read once per process): LocalStage's conv1 +
// max-pool then keeps the fp32 routing (be_conv7x7_pool_nhwc4p_f32 for large sub-batches, conv1 and the pool kernel for small ones)
bool c1_bf6_enabled();

// be_wino.hip: be_wino_conv3x3_pair_6x6_f32; pool2 = 1 writes the 2x2 max-pool of the block's output, [n,3,3,cout].
// Chained blocks (be_wino_conv3x3_pair_chain_6x6_f32): x_in_v = 1: x's input transform already lies at the start of the workspace;
// next_cmid > 0: y's input transform for a following block (conv1 with next_cmid outputs) is left there (not with pool2)
int wino_pair(const float* x, const float* packed_w1, const float* packed_bias1, int act1, const float* packed_w2,
              const float* packed_bias2, const float* residual, int act2, float* y, int64_t n, int cin, int cmid, int cout,
              float* workspace, size_t workspace_floats, void* stream, int pool2, int x_in_v = 0, int next_cmid = 0,
              const float* packed_ds = nullptr);
// packed_ds (be_wino_ds_pack_f32): the block's 1x1 downsample runs as a second K segment of conv2's GEMMs, no residual
// tensor, three workspace regions (be_wino_pair_ds_workspace_floats); y may then be null with next_cmid > 0 (not stored).
// wino_ds_fold_enabled(): LocalStage takes that form - false under BE_WINO_DS_GEMM=1, BE_WINO_F32=1, BE_ROWS_F32=1
// (read once per process).  pool_wino_in: be_maxpool_wino_in_11x11_f32; pooled may be null (the pooled map is then not stored)
bool wino_ds_fold_enabled();
int pool_wino_in(const float* x, float* pooled, int64_t n, int c, int next_cmid, float* workspace, size_t workspace_floats, void* stream);
// be_conv.hip: convolution / linear of a training unit: planned (conv_plan, the planner of every be_conv_nhwc*_f32 entry point) and
// launched.  With scratch the plan may split the K loop of a small-M tile: then the S raw slices are LEFT in scratch as [S][M][ldp]
// (S > 1 reported, nothing written to y, bias / res not applied) for the caller's kernel to sum; S == 1: y = conv + bias (+ res).
// conv_train_prepare (be_igemm_body.h) makes the same plan and hands it back instead of launching it.
int conv_train(const be_conv_desc* d, const float* x, const float* pw, const float* pb, const float* res, float* y, int ldy,
               void* scratch, size_t scratch_bytes, int* S_out, int* ldp_out, void* stream);

#define BE_REQUIRE(cond, ...) do { if (!(cond)) return be::fail(BE_EINVAL, __VA_ARGS__); } while (0)

}  // namespace be
