// The connected components of an indexed triangle mesh, their sizes, a decision per component and the compaction of a mesh to what
// stays (be_mesh_components_*, be_mesh_select_*).  be_hip/components.py states every output in numpy and the tests hold
// the kernels to it bit for bit: a label is the LEAST vertex index of its component and the sums are integers, so the outputs are a
// function of the mesh alone, whatever order the threads run in.
//
// The labelling is a lock-free union-find over parent [V]: links only ever point from a larger index to a smaller one, set by
// atomicMin, so the forest has no cycles and the root of a tree is its component's least index.  A union that loses the race for a
// root goes on with the value it lost to, which is strictly smaller: the loop ends on its own, and no thread ever waits for another
// thread or workgroup to act.  Dense ids and the slots of the compaction come from be_exclusive_scan_u8_i32.
//
// The area arithmetic is float32 with one rounding per written operation (no contraction).
#include <cstdint>
#include "be_common.h"

#pragma clang fp contract(off)

namespace {

constexpr float kAreaMax = (float)((int64_t)1 << (62 - BE_COMPONENTS_AREA_BITS));   // 2^22 m^2: q stays below 2^62
constexpr float kAreaScale = (float)((int64_t)1 << BE_COMPONENTS_AREA_BITS);

__device__ __forceinline__ int32_t load_parent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x while other threads link: parent is read with agent-scope atomic loads (the XCDs do not share an L2; a stale value
// is an ancestor all the same and costs a step) and halved on the way with atomicMin, which can only replace a parent by a smaller
// ancestor
__device__ __forceinline__ int32_t find_root(int32_t* __restrict__ parent, int32_t x) {
    for (;;) {
        const int32_t p = load_parent(parent + x);
        if (p == x) return x;
        const int32_t g = load_parent(parent + p);
        if (g < p) atomicMin(parent + x, g);
        x = g;
    }
}

__device__ __forceinline__ void unite(int32_t* __restrict__ parent, int32_t a, int32_t b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicMin(parent + hi, lo);
        if (old == hi) return;                                           // hi was a root and now hangs below lo
        a = old;                                                         // another thread linked hi first: old < hi joins lo instead
        b = lo;
    }
}

__device__ __forceinline__ bool face_in_range(const int32_t* __restrict__ faces, int64_t f, int64_t V, int32_t i[3]) {
    i[0] = faces[3 * f];
    i[1] = faces[3 * f + 1];
    i[2] = faces[3 * f + 2];
    return i[0] >= 0 && i[1] >= 0 && i[2] >= 0 && i[0] < V && i[1] < V && i[2] < V;
}

__global__ __launch_bounds__(256) void k_components_init(int32_t* __restrict__ parent, int64_t V) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < V) parent[v] = (int32_t)v;
}

// one thread per face: the unions (i0, i1) and (i1, i2)
__global__ __launch_bounds__(256) void k_components_link(int32_t* __restrict__ parent, const int32_t* __restrict__ faces, int64_t V, int64_t T) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    int32_t i[3];
    if (!face_in_range(faces, f, V, i)) return;
    unite(parent, i[0], i[1]);
    unite(parent, i[1], i[2]);
}

// one thread per vertex, after every link: the root, and whether the vertex is one.  parent is not written here.
__global__ __launch_bounds__(256) void k_components_flatten(const int32_t* __restrict__ parent, int64_t V, int32_t* __restrict__ label,
                                                            uint8_t* __restrict__ is_root) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int32_t x = (int32_t)v;
    for (int32_t p = parent[x]; p != x; p = parent[x]) x = p;
    label[v] = x;
    is_root[v] = x == (int32_t)v ? 1 : 0;
}

// thread i: component of vertex i through its root's dense id, and face_component of face i
__global__ __launch_bounds__(256) void k_components_ids(const int32_t* __restrict__ label, const int32_t* __restrict__ root_id,
                                                        const int32_t* __restrict__ faces, int64_t V, int64_t T, int32_t* __restrict__ component,
                                                        int32_t* __restrict__ face_component) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < V) component[i] = root_id[label[i]];
    if (i < T) {
        int32_t j[3];
        face_component[i] = face_in_range(faces, i, V, j) ? root_id[label[j[0]]] : -1;
    }
}

// the lanes of a wave that share a key add up before one of them issues the atomics: most waves see one component, the surface.
// Called by every lane of the wave (key < 0: nothing to add).
__device__ __forceinline__ void wave_add(int32_t key, int64_t q, int32_t* __restrict__ count, unsigned long long* __restrict__ sum) {
    const int lane = threadIdx.x & 63;
    bool todo = key >= 0;
    for (;;) {
        const unsigned long long active = __ballot(todo);
        if (active == 0) break;
        const int src = __ffsll(active) - 1;
        const int32_t k = __shfl(key, src, 64);
        const bool mine = todo && key == k;
        const unsigned long long members = __ballot(mine);
        int64_t s = mine ? q : 0;
        if (sum)
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == src) {
            atomicAdd(count + k, (int32_t)__popcll(members));
            if (sum) atomicAdd(sum + k, (unsigned long long)s);
        }
        todo = todo && !mine;
    }
}

__device__ __forceinline__ int64_t face_area_q(const float* __restrict__ vertices, const int32_t i[3]) {
    const float* a = vertices + 3 * (int64_t)i[0];
    const float* b = vertices + 3 * (int64_t)i[1];
    const float* c = vertices + 3 * (int64_t)i[2];
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    float A = 0.5f * sqrtf((nx * nx + ny * ny) + nz * nz);
    if (!(A >= 0.0f && A < __builtin_inff())) A = 0.0f;                  // NaN and inf
    A = fminf(A, kAreaMax);
    return (int64_t)(A * kAreaScale);
}

// thread i: face i into triangles and area_q, vertex i into nvertices, each through its component's dense id (< Kcap)
__global__ __launch_bounds__(256) void k_components_stats(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                          const int32_t* __restrict__ component, int64_t Kcap, int32_t* __restrict__ triangles,
                                                          int32_t* __restrict__ nvertices, unsigned long long* __restrict__ area_q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t key = -1;
    int64_t q = 0;
    if (i < T) {
        int32_t j[3];
        if (face_in_range(faces, i, V, j)) {
            key = component[j[0]];
            q = face_area_q(vertices, j);
        }
    }
    if (key >= Kcap) key = -1;                                           // never, while component came from the same mesh
    wave_add(key, q, triangles, area_q);
    key = i < V ? component[i] : -1;
    if (key >= Kcap) key = -1;
    wave_add(key, 0, nvertices, nullptr);
}

// thread k < K: keep, and with `largest` the maximum over the kept of (triangles << 32) | (0xffffffff - k): the most triangles, the
// lowest id on a tie; one atomic per wave
__global__ __launch_bounds__(256) void k_components_decide(const int32_t* __restrict__ triangles, const int64_t* __restrict__ area_q,
                                                           const int64_t* __restrict__ total, int64_t Kcap, int32_t min_triangles, int64_t min_area_q,
                                                           int largest, uint8_t* __restrict__ keep, unsigned long long* __restrict__ best) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t K = *total < Kcap ? *total : Kcap;
    unsigned long long key = 0;
    if (k < K) {
        const bool kept = triangles[k] >= min_triangles && area_q[k] >= min_area_q;
        keep[k] = kept ? 1 : 0;
        if (kept) key = ((unsigned long long)(uint32_t)triangles[k] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)k);
    }
    if (!largest) return;
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key != 0) atomicMax(best, key);
}

__global__ __launch_bounds__(256) void k_components_largest(const int64_t* __restrict__ total, int64_t Kcap, const unsigned long long* __restrict__ best,
                                                            uint8_t* __restrict__ keep) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t K = *total < Kcap ? *total : Kcap;
    if (k >= K) return;
    const unsigned long long b = *best;                                  // 0: nothing was kept
    keep[k] = b != 0 && (int64_t)(0xffffffffu - (uint32_t)b) == k ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_components_vertex_keep(const int32_t* __restrict__ component, int64_t V, const uint8_t* __restrict__ keep,
                                                                int64_t Kcap, uint8_t* __restrict__ vertex_keep) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int32_t k = component[v];
    vertex_keep[v] = k >= 0 && k < Kcap && keep[k] ? 1 : 0;
}

// thread i: the flag of vertex i as 0 / 1, and of face i: its three indices in range and kept
__global__ __launch_bounds__(256) void k_mesh_select_flags(const int32_t* __restrict__ faces, int64_t V, int64_t T, const uint8_t* __restrict__ vertex_keep,
                                                           uint8_t* __restrict__ vflag, uint8_t* __restrict__ fflag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < V) vflag[i] = vertex_keep[i] ? 1 : 0;
    if (i < T) {
        int32_t j[3];
        fflag[i] = face_in_range(faces, i, V, j) && vertex_keep[j[0]] && vertex_keep[j[1]] && vertex_keep[j[2]] ? 1 : 0;
    }
}

struct Gather {
    const float *vertices, *weight, *feat, *normal;
    const uint8_t* normal_valid;
    const int64_t* edge;
    const int32_t* component;
    float *vertices_out, *weight_out, *feat_out, *normal_out;
    uint8_t* normal_valid_out;
    int64_t* edge_out;
    int32_t *component_out, *vertex_index, *face_index, *faces_out;
    int C;
};

// thread i: vertex i to its slot voff[i] with every per-vertex array, face i to its slot foff[i] with its indices renumbered.  Every
// output element is written exactly once.
__global__ __launch_bounds__(256) void k_mesh_select_emit(Gather g, const int32_t* __restrict__ faces, int64_t V, int64_t T,
                                                          const uint8_t* __restrict__ vertex_keep, const int32_t* __restrict__ voff,
                                                          const int32_t* __restrict__ foff, int64_t V2, int64_t T2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < V && vertex_keep[i]) {
        const int64_t o = voff[i];
        if (o >= 0 && o < V2) {                                          // always, while V2 is the total the count phase reported
            for (int k = 0; k < 3; ++k) g.vertices_out[3 * o + k] = g.vertices[3 * i + k];
            g.vertex_index[o] = (int32_t)i;
            if (g.weight_out) g.weight_out[o] = g.weight[i];
            for (int c = 0; c < g.C; ++c) g.feat_out[(int64_t)c * V2 + o] = g.feat[(int64_t)c * V + i];
            if (g.normal_out)
                for (int k = 0; k < 3; ++k) g.normal_out[3 * o + k] = g.normal[3 * i + k];
            if (g.normal_valid_out) g.normal_valid_out[o] = g.normal_valid[i];
            if (g.edge_out) g.edge_out[o] = g.edge[i];
            if (g.component_out) g.component_out[o] = g.component[i];
        }
    }
    if (i < T) {
        int32_t j[3];
        if (face_in_range(faces, i, V, j) && vertex_keep[j[0]] && vertex_keep[j[1]] && vertex_keep[j[2]]) {
            const int64_t o = foff[i];
            if (o >= 0 && o < T2) {
                for (int k = 0; k < 3; ++k) g.faces_out[3 * o + k] = voff[j[k]];
                g.face_index[o] = (int32_t)i;
            }
        }
    }
}

size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }
dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
bool counts_ok(int64_t V, int64_t T) { return V >= 0 && T >= 0 && V < ((int64_t)1 << 31) && T < ((int64_t)1 << 31); }

}  // namespace

extern "C" size_t be_mesh_components_workspace_bytes(int64_t V) {
    if (V < 0 || V >= ((int64_t)1 << 31)) return 0;
    return pad8((size_t)V * sizeof(int32_t)) + pad8((size_t)V) + be_exclusive_scan_workspace_bytes(V);
}

extern "C" int be_mesh_components_i32(const int32_t* faces, int64_t V, int64_t T, int32_t* label, int32_t* component, int32_t* face_component,
                                      int64_t* total, void* workspace, size_t workspace_bytes, void* stream) {
    BE_REQUIRE(counts_ok(V, T), "be_mesh_components_i32: V = %lld vertices and T = %lld triangles; both must be in [0, 2^31)", (long long)V,
               (long long)T);
    BE_REQUIRE(total && workspace && (V == 0 || (label && component)) && (T == 0 || (faces && face_component)), "be_mesh_components_i32: null pointer");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= be_mesh_components_workspace_bytes(V),
               "be_mesh_components_i32: workspace must be 8-byte aligned and hold be_mesh_components_workspace_bytes(V) = %zu bytes, got %zu",
               be_mesh_components_workspace_bytes(V), workspace_bytes);
    char* ws = static_cast<char*>(workspace);
    int32_t* parent = reinterpret_cast<int32_t*>(ws);                    // after the flatten: the roots' dense ids
    uint8_t* is_root = reinterpret_cast<uint8_t*>(ws + pad8((size_t)V * sizeof(int32_t)));
    void* scan_ws = ws + pad8((size_t)V * sizeof(int32_t)) + pad8((size_t)V);
    hipStream_t s = be::as_stream(stream);
    if (V > 0) {
        hipLaunchKernelGGL(k_components_init, grid_for(V), dim3(256), 0, s, parent, V);
        if (T > 0) hipLaunchKernelGGL(k_components_link, grid_for(T), dim3(256), 0, s, parent, faces, V, T);
        hipLaunchKernelGGL(k_components_flatten, grid_for(V), dim3(256), 0, s, parent, V, label, is_root);
        if (const int rc = be::check_launch("be_mesh_components_i32(label)")) return rc;
    }
    if (const int rc = be_exclusive_scan_u8_i32(is_root, V, parent, total, scan_ws, be_exclusive_scan_workspace_bytes(V), stream)) return rc;
    const int64_t n = V > T ? V : T;
    if (n > 0) hipLaunchKernelGGL(k_components_ids, grid_for(n), dim3(256), 0, s, label, parent, faces, V, T, component, face_component);
    return be::check_launch("be_mesh_components_i32(ids)");
}

extern "C" int be_mesh_components_stats(const float* vertices, const int32_t* faces, int64_t V, int64_t T, const int32_t* component, int64_t Kcap,
                                        int32_t* triangles, int32_t* nvertices, int64_t* area_q, void* stream) {
    BE_REQUIRE(counts_ok(V, T), "be_mesh_components_stats: V = %lld vertices and T = %lld triangles; both must be in [0, 2^31)", (long long)V,
               (long long)T);
    BE_REQUIRE(Kcap >= 0 && Kcap <= V, "be_mesh_components_stats: Kcap must be in [0, V], got %lld", (long long)Kcap);
    BE_REQUIRE((V == 0 || (vertices && component)) && (T == 0 || faces) && (Kcap == 0 || (triangles && nvertices && area_q)),
               "be_mesh_components_stats: null pointer");
    hipStream_t s = be::as_stream(stream);
    if (Kcap == 0) return BE_OK;
    hipError_t e = hipMemsetAsync(triangles, 0, (size_t)Kcap * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(nvertices, 0, (size_t)Kcap * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(area_q, 0, (size_t)Kcap * sizeof(int64_t), s);
    if (e != hipSuccess) return be::fail(BE_ELAUNCH, "be_mesh_components_stats: hipMemsetAsync: %s", hipGetErrorString(e));
    const int64_t n = V > T ? V : T;
    hipLaunchKernelGGL(k_components_stats, grid_for(n), dim3(256), 0, s, vertices, faces, V, T, component, Kcap, triangles, nvertices,
                       reinterpret_cast<unsigned long long*>(area_q));
    return be::check_launch("be_mesh_components_stats");
}

extern "C" int be_mesh_components_decide(const int32_t* triangles, const int64_t* area_q, const int64_t* total, int64_t Kcap, int64_t min_triangles,
                                         float min_area, int largest, uint8_t* keep, const int32_t* component, int64_t V, uint8_t* vertex_keep,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    BE_REQUIRE(Kcap >= 0 && Kcap < ((int64_t)1 << 31) && V >= 0 && V < ((int64_t)1 << 31), "be_mesh_components_decide: Kcap and V must be in [0, 2^31)");
    BE_REQUIRE(min_triangles >= 0 && min_triangles < ((int64_t)1 << 31), "be_mesh_components_decide: min_triangles must be in [0, 2^31), got %lld",
               (long long)min_triangles);
    BE_REQUIRE(min_area >= 0.0f && min_area < __builtin_inff(), "be_mesh_components_decide: min_area must be a finite number >= 0");
    BE_REQUIRE(total && workspace && (Kcap == 0 || (triangles && area_q && keep)), "be_mesh_components_decide: null pointer");
    BE_REQUIRE(!vertex_keep || V == 0 || component, "be_mesh_components_decide: vertex_keep needs component");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= BE_COMPONENTS_DECIDE_WORKSPACE_BYTES,
               "be_mesh_components_decide: workspace must be 8-byte aligned and hold %d bytes, got %zu", BE_COMPONENTS_DECIDE_WORKSPACE_BYTES,
               workspace_bytes);
    const double scaled = (double)min_area * (double)((int64_t)1 << BE_COMPONENTS_AREA_BITS);   // exact
    const int64_t min_area_q = scaled >= 9223372036854775808.0 ? INT64_MAX : (int64_t)scaled;
    unsigned long long* best = static_cast<unsigned long long*>(workspace);
    hipStream_t s = be::as_stream(stream);
    if (Kcap > 0) {
        if (largest) {
            const hipError_t e = hipMemsetAsync(best, 0, sizeof(unsigned long long), s);
            if (e != hipSuccess) return be::fail(BE_ELAUNCH, "be_mesh_components_decide: hipMemsetAsync: %s", hipGetErrorString(e));
        }
        hipLaunchKernelGGL(k_components_decide, grid_for(Kcap), dim3(256), 0, s, triangles, area_q, total, Kcap, (int32_t)min_triangles, min_area_q,
                           largest ? 1 : 0, keep, best);
        if (largest) hipLaunchKernelGGL(k_components_largest, grid_for(Kcap), dim3(256), 0, s, total, Kcap, best, keep);
    }
    if (vertex_keep && V > 0) hipLaunchKernelGGL(k_components_vertex_keep, grid_for(V), dim3(256), 0, s, component, V, keep, Kcap, vertex_keep);
    return be::check_launch("be_mesh_components_decide");
}

extern "C" size_t be_mesh_select_workspace_bytes(int64_t V, int64_t T) {
    if (!counts_ok(V, T)) return 0;
    return pad8((size_t)V) + pad8((size_t)T) + be_exclusive_scan_workspace_bytes(V > T ? V : T);
}

extern "C" int be_mesh_select_count(const int32_t* faces, int64_t V, int64_t T, const uint8_t* vertex_keep, int32_t* voff, int32_t* foff,
                                    int64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
    BE_REQUIRE(counts_ok(V, T), "be_mesh_select_count: V = %lld vertices and T = %lld triangles; both must be in [0, 2^31)", (long long)V, (long long)T);
    BE_REQUIRE(totals && workspace && (V == 0 || (vertex_keep && voff)) && (T == 0 || (faces && foff)), "be_mesh_select_count: null pointer");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= be_mesh_select_workspace_bytes(V, T),
               "be_mesh_select_count: workspace must be 8-byte aligned and hold be_mesh_select_workspace_bytes(V, T) = %zu bytes, got %zu",
               be_mesh_select_workspace_bytes(V, T), workspace_bytes);
    char* ws = static_cast<char*>(workspace);
    uint8_t* vflag = reinterpret_cast<uint8_t*>(ws);
    uint8_t* fflag = vflag + pad8((size_t)V);
    void* scan_ws = ws + pad8((size_t)V) + pad8((size_t)T);
    const size_t scan_bytes = be_exclusive_scan_workspace_bytes(V > T ? V : T);
    const int64_t n = V > T ? V : T;
    if (n > 0) {
        hipLaunchKernelGGL(k_mesh_select_flags, grid_for(n), dim3(256), 0, be::as_stream(stream), faces, V, T, vertex_keep, vflag, fflag);
        if (const int rc = be::check_launch("be_mesh_select_count(flags)")) return rc;
    }
    if (const int rc = be_exclusive_scan_u8_i32(vflag, V, voff, totals, scan_ws, scan_bytes, stream)) return rc;
    return be_exclusive_scan_u8_i32(fflag, T, foff, totals + 1, scan_ws, scan_bytes, stream);
}

extern "C" int be_mesh_select_emit(const float* vertices, const int32_t* faces, int64_t V, int64_t T, const float* weight, const float* feat, int C,
                                   const float* normal, const uint8_t* normal_valid, const int64_t* edge, const int32_t* component,
                                   const uint8_t* vertex_keep, const int32_t* voff, const int32_t* foff, int64_t V2, int64_t T2, float* vertices_out,
                                   int32_t* faces_out, float* weight_out, float* feat_out, float* normal_out, uint8_t* normal_valid_out,
                                   int64_t* edge_out, int32_t* component_out, int32_t* vertex_index, int32_t* face_index, void* stream) {
    BE_REQUIRE(counts_ok(V, T), "be_mesh_select_emit: V = %lld vertices and T = %lld triangles; both must be in [0, 2^31)", (long long)V, (long long)T);
    BE_REQUIRE(V2 >= 0 && V2 <= V && T2 >= 0 && T2 <= T, "be_mesh_select_emit: V2 = %lld and T2 = %lld must lie in [0, V] and [0, T]", (long long)V2,
               (long long)T2);
    BE_REQUIRE(C >= 0 && C <= BE_FUSE_MAX_CHANNELS, "be_mesh_select_emit: C must be in [0, %d]", BE_FUSE_MAX_CHANNELS);
    BE_REQUIRE((V == 0 || (vertices && vertex_keep && voff)) && (T == 0 || (faces && foff)), "be_mesh_select_emit: null input");
    BE_REQUIRE((V2 == 0 || (vertices_out && vertex_index)) && (T2 == 0 || (faces_out && face_index)), "be_mesh_select_emit: null output");
    BE_REQUIRE(V2 == 0 || ((weight != nullptr) == (weight_out != nullptr) && (C == 0 || (feat && feat_out)) && (normal != nullptr) == (normal_out != nullptr)
                           && (normal_valid != nullptr) == (normal_valid_out != nullptr) && (edge != nullptr) == (edge_out != nullptr)
                           && (component != nullptr) == (component_out != nullptr)),
               "be_mesh_select_emit: a per-vertex array and its output are given together or not at all");
    if (V2 == 0 && T2 == 0) return BE_OK;
    Gather g;
    g.vertices = vertices; g.weight = weight; g.feat = feat; g.normal = normal; g.normal_valid = normal_valid; g.edge = edge; g.component = component;
    g.vertices_out = vertices_out; g.weight_out = weight_out; g.feat_out = feat_out; g.normal_out = normal_out;
    g.normal_valid_out = normal_valid_out; g.edge_out = edge_out; g.component_out = component_out;
    g.vertex_index = vertex_index; g.face_index = face_index; g.faces_out = faces_out;
    g.C = V2 > 0 ? C : 0;
    const int64_t n = V > T ? V : T;
    hipLaunchKernelGGL(k_mesh_select_emit, grid_for(n), dim3(256), 0, be::as_stream(stream), g, faces, V, T, vertex_keep, voff, foff, V2, T2);
    return be::check_launch("be_mesh_select_emit");
}
