// Taubin smoothing of an indexed mesh on integer sums (be_mesh_adjacency_f32, be_mesh_smooth_f32, be_mesh_normals_f32).
// be_hip/smooth.py states every output in numpy and the tests hold the kernels to it bit for bit: positions are fixed-point integers,
// a vertex's neighbour sum is an int64 sum, so the outputs are a function of the mesh alone, whatever order the threads run in.
//
// Setup, once per call: flag the usable vertices and faces; count every usable face at its corners (integer atomics) and insert its
// three undirected edges into an open-addressing table of 64-bit keys (min << 32 | max; atomicCAS on an empty slot, an integer count
// per slot); scan the valences; fill the rows (two neighbour indices per face and corner) through an atomic cursor per vertex - the
// order inside a row is arbitrary and only integer sums read it -; mark both ends of every key of count 1 as boundary.  The table
// holds a power of two >= 2 * 3T slots and at most 3T distinct keys, slots never empty again, and a probe walks up to the whole
// table: it always meets its key or an empty slot, so the table cannot overflow and the call needs NO read-back.  No thread waits
// for another.
//
// The hot loop is one launch per step: a thread per vertex gathers its row's Q triples; a row longer than kLongRow slots is summed
// by the whole wave (strided reads, an integer butterfly).  No atomics, no LDS, no barrier; a ping-pong pair of Q buffers.
//
// float32 and float64 arithmetic with one rounding per written operation (no contraction).
#include <cstdint>
#include "be_common.h"

#pragma clang fp contract(off)

namespace {

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int64_t kMaxCount = (int64_t)1 << 29;                        // vertices, triangles
constexpr float kCoordLimit = (float)(1 << BE_SMOOTH_COORD_MAX_LOG2);
constexpr double kFracScale = (double)(1 << BE_SMOOTH_FRAC_BITS);
constexpr int kLongRow = 64;                                            // slots: a longer row is the wave's, not the thread's
constexpr int kScanBlock = 1024;                                        // items per workgroup of the scan: 256 threads x 4

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// thread v: usable iff the three coordinates are finite and |x| < 2^16 (NaN fails); its valence starts at 0
__global__ __launch_bounds__(256) void k_smooth_usable(const float* __restrict__ vertices, int64_t V, uint8_t* __restrict__ usable,
                                                       int32_t* __restrict__ valence) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const bool ok = fabsf(vertices[3 * v]) < kCoordLimit && fabsf(vertices[3 * v + 1]) < kCoordLimit && fabsf(vertices[3 * v + 2]) < kCoordLimit;
    usable[v] = ok ? 1 : 0;
    valence[v] = 0;
}

// the corners of face f, or false: an index out of range, a repeated index, an unusable vertex
__device__ __forceinline__ bool face_corners(const int32_t* __restrict__ faces, int64_t f, int64_t V, const uint8_t* __restrict__ usable, int32_t c[3]) {
    c[0] = faces[3 * f];
    c[1] = faces[3 * f + 1];
    c[2] = faces[3 * f + 2];
    if (!(c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] < V && c[1] < V && c[2] < V)) return false;
    if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return false;
    return usable[c[0]] && usable[c[1]] && usable[c[2]];
}

// thread f: the face's flag, one more face at each corner and - with a table - one more face on each of its three edges
__global__ __launch_bounds__(256) void k_smooth_faces(const int32_t* __restrict__ faces, int64_t V, int64_t T, const uint8_t* __restrict__ usable,
                                                      uint8_t* __restrict__ fuse, int32_t* __restrict__ valence,
                                                      unsigned long long* __restrict__ keys, uint32_t* __restrict__ counts, uint64_t mask) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    int32_t c[3];
    const bool ok = face_corners(faces, f, V, usable, c);
    fuse[f] = ok ? 1 : 0;
    if (!ok) return;
    for (int k = 0; k < 3; ++k) atomicAdd(valence + c[k], 1);
    for (int k = 0; k < 3; ++k) {
        const uint32_t a = (uint32_t)c[k], b = (uint32_t)c[(k + 1) % 3];
        const unsigned long long key = ((unsigned long long)(a < b ? a : b) << 32) | (a < b ? b : a);
        uint64_t s = mix64(key) & mask;
        for (uint64_t n = 0; n <= mask; ++n) {                           // at most the table's capacity; ends earlier (the head of this file)
            const unsigned long long old = atomicCAS(keys + s, kEmptyKey, key);
            if (old == kEmptyKey || old == key) {
                atomicAdd(counts + s, 1u);
                break;
            }
            s = (s + 1) & mask;
        }
    }
}

// thread s: both ends of a key that exactly one face holds are boundary
__global__ __launch_bounds__(256) void k_smooth_boundary(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ counts, uint64_t cap,
                                                         int64_t V, uint8_t* __restrict__ boundary) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= cap) return;
    const unsigned long long key = keys[s];
    if (key == kEmptyKey || counts[s] != 1u) return;
    const int64_t a = (int64_t)(key >> 32), b = (int64_t)(key & 0xffffffffull);
    if (a < V && b < V) {                                                // always: the keys are corners of usable faces
        boundary[a] = 1;
        boundary[b] = 1;
    }
}

// ---- an exclusive scan of int32 counts into uint32 offsets (the total stays below 2^32: at most 3 * 2^29), three launches: the sum
// of each workgroup's 1024 items, a scan of those sums by one workgroup, the offsets.  No workgroup waits for another.
__device__ __forceinline__ uint32_t block_exclusive(uint32_t x, uint32_t* lds, uint32_t* total) {
    const int t = threadIdx.x;
    lds[t] = x;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t y = t >= d ? lds[t - d] : 0u;
        __syncthreads();
        lds[t] += y;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    *total = lds[255];
    __syncthreads();
    return incl - x;
}

__global__ __launch_bounds__(256) void k_smooth_scan_sums(const int32_t* __restrict__ counts, int64_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t lds[256];
    const int64_t base = (int64_t)blockIdx.x * kScanBlock + 4 * threadIdx.x;
    uint32_t x = 0;
    for (int k = 0; k < 4; ++k)
        if (base + k < n) x += (uint32_t)counts[base + k];
    uint32_t total;
    block_exclusive(x, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums [nb] -> their exclusive prefix sums, in place, 256 at a time with a carry
__global__ __launch_bounds__(256) void k_smooth_scan_top(uint32_t* __restrict__ sums, int64_t nb) {
    __shared__ uint32_t lds[256];
    uint32_t carry = 0;
    for (int64_t base = 0; base < nb; base += 256) {
        const int64_t i = base + threadIdx.x;
        const uint32_t x = i < nb ? sums[i] : 0u;
        uint32_t total;
        const uint32_t e = block_exclusive(x, lds, &total);
        if (i < nb) sums[i] = carry + e;
        carry += total;
    }
}

// offsets, and the cursors of the fill start at 0
__global__ __launch_bounds__(256) void k_smooth_scan_apply(const int32_t* __restrict__ counts, int64_t n, const uint32_t* __restrict__ sums,
                                                           uint32_t* __restrict__ offsets, int32_t* __restrict__ cursor) {
    __shared__ uint32_t lds[256];
    const int64_t base = (int64_t)blockIdx.x * kScanBlock + 4 * threadIdx.x;
    uint32_t c[4], x = 0;
    for (int k = 0; k < 4; ++k) {
        c[k] = base + k < n ? (uint32_t)counts[base + k] : 0u;
        x += c[k];
    }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + block_exclusive(x, lds, &total);
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) {
            offsets[base + k] = run;
            cursor[base + k] = 0;
        }
        run += c[k];
    }
}

// thread f: a usable face (a, b, c) gives a: (b, c), b: (c, a), c: (a, b), each to the next free pair of its corner's row
__global__ __launch_bounds__(256) void k_smooth_fill(const int32_t* __restrict__ faces, int64_t T, const uint8_t* __restrict__ fuse,
                                                     const uint32_t* __restrict__ offsets, const int32_t* __restrict__ valence,
                                                     int32_t* __restrict__ cursor, int32_t* __restrict__ rows) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T || !fuse[f]) return;
    const int32_t c[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    for (int k = 0; k < 3; ++k) {
        const int32_t v = c[k];
        const int32_t p = atomicAdd(cursor + v, 1);
        if (p < 0 || p >= valence[v]) continue;                          // never: the cursor counts what the valence counted
        const uint64_t at = 2 * ((uint64_t)offsets[v] + (uint64_t)p);
        rows[at] = c[(k + 1) % 3];
        rows[at + 1] = c[(k + 2) % 3];
    }
}

// thread v: Q0 = (int64) rint((double) x * 2^30), 0 for an unusable vertex
__global__ __launch_bounds__(256) void k_smooth_quantise(const float* __restrict__ vertices, int64_t V, const uint8_t* __restrict__ usable,
                                                         int64_t* __restrict__ Q) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const bool ok = usable[v] != 0;
    for (int a = 0; a < 3; ++a) Q[3 * v + a] = ok ? (int64_t)rint((double)vertices[3 * v + a] * kFracScale) : 0;
}

__device__ __forceinline__ int64_t wave_sum(int64_t x) {
    for (int d = 32; d > 0; d >>= 1) x = (int64_t)((uint64_t)x + (uint64_t)__shfl_xor((long long)x, d, 64));
    return x;
}

// One step with factor f.  Thread v sums its row when it has at most kLongRow slots; the longer rows of a wave's 64 vertices are
// then summed one after the other by all its lanes.  Sums wrap as unsigned; every lane of a wave stays in the loop to its end.
__global__ __launch_bounds__(256) void k_smooth_step(const int64_t* __restrict__ Qin, int64_t* __restrict__ Qout, int64_t V,
                                                     const uint32_t* __restrict__ offsets, const int32_t* __restrict__ valence,
                                                     const uint8_t* __restrict__ boundary, const int32_t* __restrict__ rows, double f, int free_boundary) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = v < V;
    const int64_t n = in ? 2 * (int64_t)valence[v] : 0;
    const uint64_t start = in ? 2 * (uint64_t)offsets[v] : 0;
    uint64_t S[3] = {0, 0, 0};
    if (n <= kLongRow) {
        for (int64_t i = 0; i < n; ++i) {
            const int64_t u = rows[start + i];
            for (int a = 0; a < 3; ++a) S[a] += (uint64_t)Qin[3 * u + a];
        }
    }
    unsigned long long todo = __ballot(n > kLongRow);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        const int64_t rn = __shfl((long long)n, src, 64);
        const uint64_t rs = (uint64_t)__shfl((long long)start, src, 64);
        uint64_t P[3] = {0, 0, 0};
        for (int64_t i = lane; i < rn; i += 64) {
            const int64_t u = rows[rs + i];
            for (int a = 0; a < 3; ++a) P[a] += (uint64_t)Qin[3 * u + a];
        }
        for (int a = 0; a < 3; ++a) {
            const int64_t t = wave_sum((int64_t)P[a]);
            if (lane == src) S[a] = (uint64_t)t;
        }
    }
    if (!in) return;
    const bool movable = n > 0 && (free_boundary || !boundary[v]);
    for (int a = 0; a < 3; ++a) {
        const int64_t q = Qin[3 * v + a];
        int64_t r = q;
        if (movable) {
            const double mean = (double)(int64_t)S[a] / (double)n;
            const double d = mean - (double)q;
            r = (int64_t)((uint64_t)q + (uint64_t)(int64_t)rint(f * d));
        }
        Qout[3 * v + a] = r;
    }
}

// thread v: the position - the input's bits where Q == Q0 on all three axes - and the displacement
__global__ __launch_bounds__(256) void k_smooth_finalise(const float* __restrict__ vertices, int64_t V, const uint8_t* __restrict__ usable,
                                                         const int64_t* __restrict__ Q, float* __restrict__ vertices_out,
                                                         float* __restrict__ displacement) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const bool ok = usable[v] != 0;
    float x[3], y[3];
    bool same = true;
    for (int a = 0; a < 3; ++a) {
        x[a] = vertices[3 * v + a];
        const int64_t q0 = ok ? (int64_t)rint((double)x[a] * kFracScale) : 0;
        const int64_t q = Q[3 * v + a];
        same = same && q == q0;
        y[a] = (float)((double)q * (1.0 / kFracScale));
    }
    const uint32_t* bits = reinterpret_cast<const uint32_t*>(vertices);
    uint32_t* out_bits = reinterpret_cast<uint32_t*>(vertices_out);
    float d[3];
    for (int a = 0; a < 3; ++a) {
        if (same) out_bits[3 * v + a] = bits[3 * v + a];
        else vertices_out[3 * v + a] = y[a];
        d[a] = same ? 0.0f : y[a] - x[a];
    }
    displacement[v] = ok ? sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) : 0.0f;
}

// thread f: the face's normal in components.face_area_q's operation order, quantised, added to its three corners
__global__ __launch_bounds__(256) void k_smooth_normal_sums(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                            const uint8_t* __restrict__ usable, unsigned long long* __restrict__ sums) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    int32_t c[3];
    if (!face_corners(faces, f, V, usable, c)) return;
    float p[3][3];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) p[k][a] = vertices[3 * (int64_t)c[k] + a];
    const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const float wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
    const float n[3] = {uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx};
    for (int a = 0; a < 3; ++a) {
        float x = n[a];
        if (!(fabsf(x) < __builtin_inff())) x = 0.0f;                    // NaN and inf
        x = fminf(fmaxf(x, -4096.0f), 4096.0f);
        const int64_t nq = (int64_t)(x * 0x1p40f);
        if (nq == 0) continue;
        for (int k = 0; k < 3; ++k) atomicAdd(sums + 3 * (int64_t)c[k] + a, (unsigned long long)nq);
    }
}

// thread v: the normalised sum
__global__ __launch_bounds__(256) void k_smooth_normal_emit(const unsigned long long* __restrict__ sums, int64_t V, float* __restrict__ normal,
                                                            uint8_t* __restrict__ normal_valid) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    float m[3];
    for (int a = 0; a < 3; ++a) m[a] = (float)((double)(int64_t)sums[3 * v + a] * 0x1p-40);
    const float l = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    const bool valid = l > 0.0f && l < __builtin_inff();
    for (int a = 0; a < 3; ++a) normal[3 * v + a] = valid ? m[a] / l : 0.0f;
    normal_valid[v] = valid ? 1 : 0;
}

size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }
dim3 grid_for(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }
bool counts_ok(int64_t V, int64_t T) { return V >= 0 && T >= 0 && V <= kMaxCount && T <= kMaxCount; }
int64_t scan_blocks(int64_t V) { return (V + kScanBlock - 1) / kScanBlock; }

// the edge table of T triangles: the power of two >= 2 * 3 T, at least 2
uint64_t capacity(int64_t T) {
    uint64_t c = 2;
    while (c < 6 * (uint64_t)T) c <<= 1;
    return c;
}

struct Workspace {
    int64_t *QA, *QB;                                                   // [V,3] each; QA doubles as the normal sums
    unsigned long long* keys;                                            // [cap]
    uint32_t* counts;                                                    // [cap]
    int32_t* rows;                                                       // [6 T]
    uint32_t* offsets;                                                   // [V]
    int32_t* cursor;                                                     // [V]
    uint32_t* sums;                                                      // [scan_blocks(V)]
    uint8_t *usable, *fuse;                                              // [V], [T]
    size_t bytes;
};

Workspace carve(void* workspace, int64_t V, int64_t T) {
    const size_t nv = (size_t)V, nt = (size_t)T;
    const uint64_t cap = capacity(T);
    char* p = static_cast<char*>(workspace);
    char* const p0 = p;
    Workspace w;
    w.QA = reinterpret_cast<int64_t*>(p);
    p += nv * 24;
    w.QB = reinterpret_cast<int64_t*>(p);
    p += nv * 24;
    w.keys = reinterpret_cast<unsigned long long*>(p);
    p += cap * 8;
    w.counts = reinterpret_cast<uint32_t*>(p);
    p += pad8(cap * 4);
    w.rows = reinterpret_cast<int32_t*>(p);
    p += pad8(nt * 24);
    w.offsets = reinterpret_cast<uint32_t*>(p);
    p += pad8(nv * 4);
    w.cursor = reinterpret_cast<int32_t*>(p);
    p += pad8(nv * 4);
    w.sums = reinterpret_cast<uint32_t*>(p);
    p += pad8((size_t)scan_blocks(V) * 4);
    w.usable = reinterpret_cast<uint8_t*>(p);
    p += pad8(nv);
    w.fuse = reinterpret_cast<uint8_t*>(p);
    p += pad8(nt);
    w.bytes = (size_t)(p - p0);
    return w;
}

// flags, valences, the edge table and boundary [V] (0 / 1) on stream s
int adjacency(const char* who, const float* vertices, const int32_t* faces, int64_t V, int64_t T, const Workspace& w, int32_t* valence, uint8_t* boundary,
              hipStream_t s) {
    if (V == 0) return BE_OK;
    const uint64_t cap = capacity(T);
    hipError_t e = hipMemsetAsync(boundary, 0, (size_t)V, s);
    if (e == hipSuccess && T > 0) e = hipMemsetAsync(w.keys, 0xff, cap * 8, s);
    if (e == hipSuccess && T > 0) e = hipMemsetAsync(w.counts, 0, cap * 4, s);
    if (e != hipSuccess) return be::fail(BE_ELAUNCH, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    hipLaunchKernelGGL(k_smooth_usable, grid_for(V), dim3(256), 0, s, vertices, V, w.usable, valence);
    if (T > 0) {
        hipLaunchKernelGGL(k_smooth_faces, grid_for(T), dim3(256), 0, s, faces, V, T, w.usable, w.fuse, valence, w.keys, w.counts, cap - 1);
        hipLaunchKernelGGL(k_smooth_boundary, grid_for(cap), dim3(256), 0, s, w.keys, w.counts, cap, V, boundary);
    }
    return be::check_launch(who);
}

bool workspace_ok(const void* workspace, size_t bytes, int64_t V, int64_t T) {
    return workspace && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && bytes >= be_mesh_smooth_workspace_bytes(V, T);
}

}  // namespace

extern "C" size_t be_mesh_smooth_workspace_bytes(int64_t V, int64_t T) {
    if (!counts_ok(V, T)) return 0;
    return carve(nullptr, V, T).bytes;
}

extern "C" int be_mesh_adjacency_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t T, int32_t* valence, uint8_t* boundary,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    BE_REQUIRE(counts_ok(V, T), "be_mesh_adjacency_f32: V = %lld vertices and T = %lld triangles; both must be in [0, 2^29]", (long long)V, (long long)T);
    BE_REQUIRE((V == 0 || (vertices && valence && boundary)) && (T == 0 || faces), "be_mesh_adjacency_f32: null pointer");
    BE_REQUIRE(workspace_ok(workspace, workspace_bytes, V, T),
               "be_mesh_adjacency_f32: workspace must be 8-byte aligned and hold be_mesh_smooth_workspace_bytes(V, T) = %zu bytes, got %zu",
               be_mesh_smooth_workspace_bytes(V, T), workspace_bytes);
    return adjacency("be_mesh_adjacency_f32", vertices, faces, V, T, carve(workspace, V, T), valence, boundary, be::as_stream(stream));
}

extern "C" int be_mesh_smooth_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t T, int iters, double lam, double mu, int free_boundary,
                                  float* vertices_out, float* displacement, int32_t* valence, uint8_t* boundary, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    BE_REQUIRE(counts_ok(V, T), "be_mesh_smooth_f32: V = %lld vertices and T = %lld triangles; both must be in [0, 2^29]", (long long)V, (long long)T);
    BE_REQUIRE(iters >= 0 && iters <= BE_SMOOTH_MAX_ITERS, "be_mesh_smooth_f32: iters = %d; must be in [0, %d]", iters, BE_SMOOTH_MAX_ITERS);
    BE_REQUIRE(lam > 0.0 && lam <= 1.0, "be_mesh_smooth_f32: lam = %g; must be a finite number in (0, 1]", lam);
    BE_REQUIRE(mu >= -2.0 && mu <= 0.0, "be_mesh_smooth_f32: mu = %g; must be a finite number in [-2, 0]", mu);
    BE_REQUIRE(free_boundary == 0 || free_boundary == 1, "be_mesh_smooth_f32: free_boundary must be 0 (boundary vertices held) or 1");
    BE_REQUIRE((V == 0 || (vertices && vertices_out && displacement && valence && boundary)) && (T == 0 || faces), "be_mesh_smooth_f32: null pointer");
    BE_REQUIRE(workspace_ok(workspace, workspace_bytes, V, T),
               "be_mesh_smooth_f32: workspace must be 8-byte aligned and hold be_mesh_smooth_workspace_bytes(V, T) = %zu bytes, got %zu",
               be_mesh_smooth_workspace_bytes(V, T), workspace_bytes);
    if (V == 0) return BE_OK;
    const Workspace w = carve(workspace, V, T);
    hipStream_t s = be::as_stream(stream);
    if (const int rc = adjacency("be_mesh_smooth_f32(adjacency)", vertices, faces, V, T, w, valence, boundary, s)) return rc;
    const unsigned nb = (unsigned)scan_blocks(V);
    hipLaunchKernelGGL(k_smooth_scan_sums, dim3(nb), dim3(256), 0, s, valence, V, w.sums);
    hipLaunchKernelGGL(k_smooth_scan_top, dim3(1), dim3(256), 0, s, w.sums, (int64_t)nb);
    hipLaunchKernelGGL(k_smooth_scan_apply, dim3(nb), dim3(256), 0, s, valence, V, w.sums, w.offsets, w.cursor);
    if (T > 0) hipLaunchKernelGGL(k_smooth_fill, grid_for(T), dim3(256), 0, s, faces, T, w.fuse, w.offsets, valence, w.cursor, w.rows);
    hipLaunchKernelGGL(k_smooth_quantise, grid_for(V), dim3(256), 0, s, vertices, V, w.usable, w.QA);
    if (const int rc = be::check_launch("be_mesh_smooth_f32(setup)")) return rc;
    int64_t *in = w.QA, *out = w.QB;
    for (int it = 0; it < iters; ++it) {
        for (int half = 0; half < 2; ++half) {
            if (half == 1 && mu == 0.0) break;
            hipLaunchKernelGGL(k_smooth_step, grid_for(V), dim3(256), 0, s, in, out, V, w.offsets, valence, boundary, w.rows, half ? mu : lam,
                               free_boundary);
            int64_t* t = in;
            in = out;
            out = t;
        }
    }
    hipLaunchKernelGGL(k_smooth_finalise, grid_for(V), dim3(256), 0, s, vertices, V, w.usable, in, vertices_out, displacement);
    return be::check_launch("be_mesh_smooth_f32");
}

extern "C" int be_mesh_normals_f32(const float* vertices, const int32_t* faces, int64_t V, int64_t T, float* normal, uint8_t* normal_valid,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    BE_REQUIRE(counts_ok(V, T), "be_mesh_normals_f32: V = %lld vertices and T = %lld triangles; both must be in [0, 2^29]", (long long)V, (long long)T);
    BE_REQUIRE((V == 0 || (vertices && normal && normal_valid)) && (T == 0 || faces), "be_mesh_normals_f32: null pointer");
    BE_REQUIRE(workspace_ok(workspace, workspace_bytes, V, T),
               "be_mesh_normals_f32: workspace must be 8-byte aligned and hold be_mesh_smooth_workspace_bytes(V, T) = %zu bytes, got %zu",
               be_mesh_smooth_workspace_bytes(V, T), workspace_bytes);
    if (V == 0) return BE_OK;
    const Workspace w = carve(workspace, V, T);
    hipStream_t s = be::as_stream(stream);
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(w.QA);
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)V * 24, s);
    if (e != hipSuccess) return be::fail(BE_ELAUNCH, "be_mesh_normals_f32: hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_smooth_usable, grid_for(V), dim3(256), 0, s, vertices, V, w.usable, w.cursor);
    if (T > 0) hipLaunchKernelGGL(k_smooth_normal_sums, grid_for(T), dim3(256), 0, s, vertices, faces, V, T, w.usable, sums);
    hipLaunchKernelGGL(k_smooth_normal_emit, grid_for(V), dim3(256), 0, s, sums, V, normal, normal_valid);
    return be::check_launch("be_mesh_normals_f32");
}
