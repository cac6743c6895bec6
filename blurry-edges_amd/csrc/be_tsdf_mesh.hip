// A triangle mesh out of a TSDF volume's means (be_tsdf_mesh_count_f32, be_tsdf_mesh_emit_f32) and the device-side
// exclusive scan it needs (be_exclusive_scan_u8_i32).  Marching tetrahedra on the Kuhn split of every cell into 6 tetrahedra about
// the body diagonal 000-111: be_hip/mesh.py states the method, the numbering, the order of the outputs and every float operation in
// numpy, derives the case table (be_tsdf_mesh_table.h is generated from it) and the tests hold the kernels to it bit for bit.
//
// A mesh vertex lies on a lattice edge (owner voxel v, type e = 0..6), a triangle belongs to a cell and a tetrahedron: every output
// has one owner thread and its slot is an exclusive prefix sum of per-voxel counts, so there are no atomics and no hash table, and
// the result is the same on every run.  The scan is three launches (per-workgroup sums, a scan of those sums in 64 bits by one
// workgroup, per-workgroup apply); no workgroup ever waits for another.  The host reads the two totals between count and emit to
// allocate the outputs: the one synchronisation a result of variable length costs.
//
// All float arithmetic is float32 with one rounding per written operation (no contraction).
#include <cstdint>
#include "be_common.h"
#include "be_tsdf_vol.h"
#include "be_tsdf_mesh_table.h"

#pragma clang fp contract(off)

namespace {

using be::Vol;

constexpr int kScanThreads = 256;
constexpr int kScanItems = 4;                                           // bytes per thread: one 32-bit load where the input allows it
constexpr int kScanSpan = kScanThreads * kScanItems;                    // BE_SCAN_SPAN elements per workgroup
static_assert(kScanSpan == BE_SCAN_SPAN && kScanThreads == BE_SCAN_SUMS_PER_PASS, "the header states the scan's spans");

// ------------------------------------------------------------------------------------------------------------------- the scan
// inclusive scan over the 256 threads of a workgroup: shuffles inside each wave64, the 4 wave totals through LDS
__device__ __forceinline__ int64_t block_inclusive_scan(int64_t v, int64_t* __restrict__ wave_sums, int64_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    __syncthreads();                                                    // wave_sums may still be read from the previous use
    if (lane == 63) wave_sums[wave] = v;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int w = 0; w < kScanThreads / 64; ++w) {
        const int64_t s = wave_sums[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return v + before;
}

// a thread's kScanItems counts, those past n zero; POPC: the counts are the population counts of the bytes (edge masks)
template <bool POPC>
__device__ __forceinline__ void load_counts(const uint8_t* __restrict__ in, int64_t n, int64_t i0, bool aligned, int c[kScanItems]) {
    uint32_t word = 0;
    if (aligned && i0 + kScanItems <= n) {
        word = *reinterpret_cast<const uint32_t*>(in + i0);
    } else {
        for (int k = 0; k < kScanItems; ++k)
            if (i0 + k < n) word |= (uint32_t)in[i0 + k] << (8 * k);
    }
    for (int k = 0; k < kScanItems; ++k) {
        const uint32_t b = (word >> (8 * k)) & 0xffu;
        c[k] = POPC ? __popc(b) : (int)b;
    }
}

template <bool POPC>
__global__ __launch_bounds__(kScanThreads) void k_scan_reduce(const uint8_t* __restrict__ in, int64_t n, int aligned, int64_t* __restrict__ sums) {
    __shared__ int64_t wave_sums[kScanThreads / 64];
    const int64_t i0 = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    int c[kScanItems];
    load_counts<POPC>(in, n, i0, aligned != 0, c);
    int s = 0;
    for (int k = 0; k < kScanItems; ++k) s += c[k];
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) t += wave_sums[w];
        sums[blockIdx.x] = t;
    }
}

// one workgroup: the workgroup sums -> their exclusive prefix, in place, 256 at a time with a carry; the total of everything
__global__ __launch_bounds__(kScanThreads) void k_scan_sums(int64_t* __restrict__ sums, int64_t nb, int64_t* __restrict__ total) {
    __shared__ int64_t wave_sums[kScanThreads / 64];
    int64_t carry = 0;
    for (int64_t base = 0; base < nb; base += kScanThreads) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < nb ? sums[i] : 0;
        int64_t all;
        const int64_t incl = block_inclusive_scan(v, wave_sums, &all);
        if (i < nb) sums[i] = carry + (incl - v);
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <bool POPC>
__global__ __launch_bounds__(kScanThreads) void k_scan_apply(const uint8_t* __restrict__ in, int64_t n, int aligned, const int64_t* __restrict__ sums,
                                                             int32_t* __restrict__ out) {
    __shared__ int64_t wave_sums[kScanThreads / 64];
    const int64_t i0 = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    int c[kScanItems];
    load_counts<POPC>(in, n, i0, aligned != 0, c);
    int s = 0;
    for (int k = 0; k < kScanItems; ++k) s += c[k];
    int64_t all;
    const int64_t incl = block_inclusive_scan((int64_t)s, wave_sums, &all);
    int64_t run = sums[blockIdx.x] + (incl - s);
    for (int k = 0; k < kScanItems; ++k) {
        if (i0 + k < n) out[i0 + k] = (int32_t)(uint32_t)(uint64_t)run;  // the low 32 bits: a total >= 2^31 is refused by the caller
        run += c[k];
    }
}

size_t scan_workspace_bytes(int64_t n) { return (size_t)((n + kScanSpan - 1) / kScanSpan + 1) * sizeof(int64_t); }

template <bool POPC>
int scan(const char* who, const uint8_t* in, int64_t n, int32_t* out, int64_t* total, void* workspace, hipStream_t s) {
    int64_t* sums = static_cast<int64_t*>(workspace);
    const int64_t nb = (n + kScanSpan - 1) / kScanSpan;
    const int aligned = (reinterpret_cast<uintptr_t>(in) & 3u) == 0;
    if (nb > 0) hipLaunchKernelGGL(k_scan_reduce<POPC>, dim3((unsigned)nb), dim3(kScanThreads), 0, s, in, n, aligned, sums);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kScanThreads), 0, s, sums, nb, total);
    if (nb > 0) hipLaunchKernelGGL(k_scan_apply<POPC>, dim3((unsigned)nb), dim3(kScanThreads), 0, s, in, n, aligned, sums, out);
    return be::check_launch(who);
}

// ------------------------------------------------------------------------------------------------------------------- the mesh
struct Idx { int ix, iy, iz; };

__device__ __forceinline__ Idx split(const Vol& vol, int64_t i) {
    Idx p;
    p.ix = (int)(i % vol.nx);
    const int64_t r = i / vol.nx;
    p.iy = (int)(r % vol.ny);
    p.iz = (int)(r / vol.ny);
    return p;
}

__device__ __forceinline__ int64_t corner_offset(const Vol& vol, int k) {
    return ((int64_t)((k >> 2) & 1) * vol.ny + ((k >> 1) & 1)) * vol.nx + (k & 1);
}

// the cube code of the cell whose origin corner is voxel i (all 8 corners inside the volume): bit k set when corner k has D > 0
__device__ __forceinline__ int cube_code(const float* __restrict__ D, const Vol& vol, int64_t i) {
    const int64_t dy = vol.nx, dz = (int64_t)vol.nx * vol.ny;
    const float* p = D + i;
    return (p[0] > 0.0f ? 1 : 0) | (p[1] > 0.0f ? 2 : 0) | (p[dy] > 0.0f ? 4 : 0) | (p[dy + 1] > 0.0f ? 8 : 0) | (p[dz] > 0.0f ? 16 : 0) |
           (p[dz + 1] > 0.0f ? 32 : 0) | (p[dz + dy] > 0.0f ? 64 : 0) | (p[dz + dy + 1] > 0.0f ? 128 : 0);
}

// One thread per voxel taken as a cell's origin corner: the cell's triangle count, 0 where the voxel is no cell's origin (the last
// layer of an axis) or a corner is not observed.  The 8 weights are tested before D is read, as the ray cast does.
__global__ __launch_bounds__(256) void k_mesh_cells(Vol vol, const float* __restrict__ D, const float* __restrict__ W, float min_weight,
                                                    uint8_t* __restrict__ nt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= vol.n) return;
    const Idx p = split(vol, i);
    int count = 0;
    if (p.ix <= vol.nx - 2 && p.iy <= vol.ny - 2 && p.iz <= vol.nz - 2) {
        const int64_t dy = vol.nx, dz = (int64_t)vol.nx * vol.ny;
        const float* w = W + i;
        const bool valid = w[0] > min_weight && w[1] > min_weight && w[dy] > min_weight && w[dy + 1] > min_weight && w[dz] > min_weight &&
                           w[dz + 1] > min_weight && w[dz + dy] > min_weight && w[dz + dy + 1] > min_weight;
        if (valid) count = kMeshCubeCount[cube_code(D, vol, i)];
    }
    nt[i] = (uint8_t)count;
}

// One thread per voxel: bit e of its mask is set when its edge of type e is active - the endpoints differ in positivity and one
// of the cells that contain both emits a triangle (nt > 0: the cell is valid and crossed, and all its lattice edges are tet edges).
// The cells that contain edge e of voxel v have their origin at v - (0 or 1) along every axis the edge does not advance on.
__global__ __launch_bounds__(256) void k_mesh_edges(Vol vol, const float* __restrict__ D, const uint8_t* __restrict__ nt, uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= vol.n) return;
    const Idx p = split(vol, i);
    // cells[k]: the cell with its origin at v - (bits of k) emits something, k = 4 bz + 2 by + bx
    int cells = 0;
    for (int k = 0; k < 7; ++k) {
        const int bx = k & 1, by = (k >> 1) & 1, bz = (k >> 2) & 1;
        if (p.ix - bx >= 0 && p.iy - by >= 0 && p.iz - bz >= 0 && nt[i - corner_offset(vol, k)] != 0) cells |= 1 << k;
    }
    int m = 0;
    if (cells != 0) {
        const bool pos = D[i] > 0.0f;
        for (int e = 0; e < 7; ++e) {
            const int o = e < 3 ? 1 << e : (e == 3 ? 3 : e == 4 ? 5 : e == 5 ? 6 : 7);      // the offset's bits, 4 dz + 2 dy + dx
            // the containing cells step back only along the axes where o has no bit
            int inside = 0;
            for (int k = 0; k < 7; ++k)
                if ((k & o) == 0) inside |= (cells >> k) & 1;
            // a cell that emits and contains the edge has all its corners inside the volume: D at the far endpoint exists
            if (inside && (D[i + corner_offset(vol, o)] > 0.0f) != pos) m |= 1 << e;
        }
    }
    mask[i] = (uint8_t)m;
}

// the gradient of D at voxel q along one axis over the metric spacing s: central where both neighbours exist and are observed, else
// one-sided towards the one that is (one is, for an endpoint of an active edge); +0 where neither
__device__ __forceinline__ float axis_gradient(const float* __restrict__ D, const float* __restrict__ W, float min_weight, int64_t q, int i,
                                               int n, int64_t stride, float s) {
    const bool hi = i + 1 < n && W[q + stride] > min_weight;
    const bool lo = i - 1 >= 0 && W[q - stride] > min_weight;
    if (hi && lo) return (D[q + stride] - D[q - stride]) * 0.5f / s;
    if (hi) return (D[q + stride] - D[q]) / s;
    if (lo) return (D[q] - D[q - stride]) / s;
    return 0.0f;
}

// One thread per voxel that owns a vertex: its active edges in the order of e, at voff + rank
__global__ __launch_bounds__(256) void k_mesh_vertices(Vol vol, const float* __restrict__ D, const float* __restrict__ W, const float* __restrict__ Fm,
                                                       int C, float min_weight, const uint8_t* __restrict__ mask, const int32_t* __restrict__ voff,
                                                       int64_t V, float* __restrict__ vertices, float* __restrict__ weight, float* __restrict__ feat,
                                                       float* __restrict__ normal, uint8_t* __restrict__ normal_valid, int64_t* __restrict__ edge) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= vol.n) return;
    const int m = mask[i];
    if (m == 0) return;
    const Idx p = split(vol, i);
    const int64_t dy = vol.nx, dz = (int64_t)vol.nx * vol.ny;
    const float Da = D[i], Wa = W[i];
    const float xa = vol.x0 + (float)p.ix * vol.sx;
    const float ya = vol.y0 + (float)p.iy * vol.sy;
    const float za = vol.z0 + (float)p.iz * vol.sz;
    float gax = 0.0f, gay = 0.0f, gaz = 0.0f;
    if (normal) {
        gax = axis_gradient(D, W, min_weight, i, p.ix, vol.nx, 1, vol.sx);
        gay = axis_gradient(D, W, min_weight, i, p.iy, vol.ny, dy, vol.sy);
        gaz = axis_gradient(D, W, min_weight, i, p.iz, vol.nz, dz, vol.sz);
    }
    int64_t slot = voff[i];
    for (int e = 0; e < 7; ++e) {
        if (!((m >> e) & 1)) continue;
        const int64_t v = slot++;
        if (v < 0 || v >= V) continue;                                   // never, while V is the total the count phase reported
        const int o = e < 3 ? 1 << e : (e == 3 ? 3 : e == 4 ? 5 : e == 5 ? 6 : 7);
        const int ox = o & 1, oy = (o >> 1) & 1, oz = (o >> 2) & 1;
        const int64_t j = i + corner_offset(vol, o);
        const float Db = D[j];
        const float t = Da / (Da - Db);
        const float xb = vol.x0 + (float)(p.ix + ox) * vol.sx;
        const float yb = vol.y0 + (float)(p.iy + oy) * vol.sy;
        const float zb = vol.z0 + (float)(p.iz + oz) * vol.sz;
        vertices[3 * v + 0] = xa + t * (xb - xa);
        vertices[3 * v + 1] = ya + t * (yb - ya);
        vertices[3 * v + 2] = za + t * (zb - za);
        weight[v] = Wa + t * (W[j] - Wa);
        for (int c = 0; c < C; ++c) {
            const float* Fc = Fm + (int64_t)c * vol.n;
            const float fa = Fc[i];
            feat[(int64_t)c * V + v] = fa + t * (Fc[j] - fa);
        }
        edge[v] = 7 * i + e;
        if (normal) {
            const float gbx = axis_gradient(D, W, min_weight, j, p.ix + ox, vol.nx, 1, vol.sx);
            const float gby = axis_gradient(D, W, min_weight, j, p.iy + oy, vol.ny, dy, vol.sy);
            const float gbz = axis_gradient(D, W, min_weight, j, p.iz + oz, vol.nz, dz, vol.sz);
            const float gx = gax + t * (gbx - gax);
            const float gy = gay + t * (gby - gay);
            const float gz = gaz + t * (gbz - gaz);
            const float l = sqrtf((gx * gx + gy * gy) + gz * gz);
            const bool ok = l > 0.0f && l < __builtin_inff();
            normal[3 * v + 0] = ok ? gx / l : 0.0f;
            normal[3 * v + 1] = ok ? gy / l : 0.0f;
            normal[3 * v + 2] = ok ? gz / l : 0.0f;
            normal_valid[v] = ok ? 1 : 0;
        }
    }
}

// One thread per cell that emits: its triangles in the order of (t, the table), at toff + rank; a triangle's vertex is the rank of
// its edge among the active edges of the edge's owner, past that owner's voff
__global__ __launch_bounds__(256) void k_mesh_faces(Vol vol, const float* __restrict__ D, const uint8_t* __restrict__ nt, const uint8_t* __restrict__ mask,
                                                    const int32_t* __restrict__ voff, const int32_t* __restrict__ toff, int64_t T,
                                                    int32_t* __restrict__ faces) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= vol.n) return;
    if (nt[i] == 0) return;
    const int cube = cube_code(D, vol, i);
    int64_t slot = toff[i];
    for (int t = 0; t < 6; ++t) {
        int code = 0;
        for (int c = 0; c < 4; ++c) code |= ((cube >> kMeshTetCorner[t][c]) & 1) << c;
        const int count = kMeshTriCount[t][code];
        for (int s = 0; s < count; ++s) {
            const int64_t f = slot++;
            if (f < 0 || f >= T) continue;                               // never, while T is the total the count phase reported
            for (int j = 0; j < 3; ++j) {
                const int ve = kMeshTriVert[t][code][s][j];
                const int64_t owner = i + corner_offset(vol, ve >> 3);
                const int e = ve & 7;
                faces[3 * f + j] = voff[owner] + __popc((uint32_t)mask[owner] & ((1u << e) - 1u));
            }
        }
    }
}

size_t mesh_workspace_bytes(int64_t n) { return scan_workspace_bytes(n); }

}  // namespace

extern "C" size_t be_exclusive_scan_workspace_bytes(int64_t n) { return n < 0 ? 0 : scan_workspace_bytes(n); }

extern "C" int be_exclusive_scan_u8_i32(const uint8_t* counts, int64_t n, int32_t* offsets, int64_t* total, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    BE_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "be_exclusive_scan_u8_i32: n must be in [0, 2^31), got %lld", (long long)n);
    BE_REQUIRE(total && workspace && (n == 0 || (counts && offsets)), "be_exclusive_scan_u8_i32: null pointer");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= scan_workspace_bytes(n),
               "be_exclusive_scan_u8_i32: workspace must be 8-byte aligned and hold be_exclusive_scan_workspace_bytes(n) = %zu bytes, got %zu",
               scan_workspace_bytes(n), workspace_bytes);
    return scan<false>("be_exclusive_scan_u8_i32", counts, n, offsets, total, workspace, be::as_stream(stream));
}

extern "C" size_t be_tsdf_mesh_workspace_bytes(int64_t n) { return n < 0 ? 0 : mesh_workspace_bytes(n); }

extern "C" int be_tsdf_mesh_count_f32(const float* D, const float* W, const int* dims, float min_weight, uint8_t* nt, uint8_t* mask,
                                      int32_t* voff, int32_t* toff, int64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
    BE_REQUIRE(D && W && nt && mask && voff && toff && totals && workspace, "be_tsdf_mesh_count_f32: null pointer");
    const float zero[3] = {0.0f, 0.0f, 0.0f}, one[3] = {1.0f, 1.0f, 1.0f};
    Vol vol;
    if (const int rc = be::make_vol("be_tsdf_mesh_count_f32", dims, zero, one, 1.0f, &vol)) return rc;
    BE_REQUIRE(min_weight >= 0.0f && min_weight < __builtin_inff(), "be_tsdf_mesh_count_f32: min_weight must be a finite number >= 0");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= mesh_workspace_bytes(vol.n),
               "be_tsdf_mesh_count_f32: workspace must be 8-byte aligned and hold be_tsdf_mesh_workspace_bytes(n) = %zu bytes, got %zu",
               mesh_workspace_bytes(vol.n), workspace_bytes);
    hipStream_t s = be::as_stream(stream);
    const dim3 grid((unsigned)((vol.n + 255) / 256));
    hipLaunchKernelGGL(k_mesh_cells, grid, dim3(256), 0, s, vol, D, W, min_weight, nt);
    hipLaunchKernelGGL(k_mesh_edges, grid, dim3(256), 0, s, vol, D, nt, mask);
    if (const int rc = scan<true>("be_tsdf_mesh_count_f32", mask, vol.n, voff, totals, workspace, s)) return rc;
    return scan<false>("be_tsdf_mesh_count_f32", nt, vol.n, toff, totals + 1, workspace, s);
}

extern "C" int be_tsdf_mesh_emit_f32(const float* D, const float* W, const float* Fm, int C, const int* dims, const float* origin,
                                     const float* voxel, float min_weight, const uint8_t* nt, const uint8_t* mask, const int32_t* voff,
                                     const int32_t* toff, int64_t V, int64_t T, float* vertices, int32_t* faces, float* weight, float* feat,
                                     float* normal, uint8_t* normal_valid, int64_t* edge, void* stream) {
    BE_REQUIRE(D && W && nt && mask && voff && toff, "be_tsdf_mesh_emit_f32: null pointer");
    BE_REQUIRE(C >= 0 && C <= BE_FUSE_MAX_CHANNELS && (C == 0 || Fm), "be_tsdf_mesh_emit_f32: C must be in [0, %d], and Fm given when C > 0",
               BE_FUSE_MAX_CHANNELS);
    Vol vol;
    if (const int rc = be::make_vol("be_tsdf_mesh_emit_f32", dims, origin, voxel, 1.0f, &vol)) return rc;
    BE_REQUIRE(min_weight >= 0.0f && min_weight < __builtin_inff(), "be_tsdf_mesh_emit_f32: min_weight must be a finite number >= 0");
    BE_REQUIRE(V >= 0 && T >= 0 && V < ((int64_t)1 << 31) && T < ((int64_t)1 << 31),
               "be_tsdf_mesh_emit_f32: V = %lld vertices and T = %lld triangles; both must be in [0, 2^31)", (long long)V, (long long)T);
    BE_REQUIRE(V == 0 || (vertices && weight && edge && (C == 0 || feat)), "be_tsdf_mesh_emit_f32: null vertex output with V > 0");
    BE_REQUIRE((normal == nullptr) == (normal_valid == nullptr), "be_tsdf_mesh_emit_f32: normal and normal_valid are given together or not at all");
    BE_REQUIRE(T == 0 || faces, "be_tsdf_mesh_emit_f32: null faces with T > 0");
    hipStream_t s = be::as_stream(stream);
    const dim3 grid((unsigned)((vol.n + 255) / 256));
    if (V > 0)
        hipLaunchKernelGGL(k_mesh_vertices, grid, dim3(256), 0, s, vol, D, W, C > 0 ? Fm : nullptr, C, min_weight, mask, voff, V, vertices, weight,
                           feat, normal, normal_valid, edge);
    if (T > 0) hipLaunchKernelGGL(k_mesh_faces, grid, dim3(256), 0, s, vol, D, nt, mask, voff, toff, T, faces);
    return be::check_launch("be_tsdf_mesh_emit_f32");
}
