// Mesh simplification by vertex clustering on a cell grid (be_mesh_cluster_f32, be_mesh_simplify_*).
// be_hip/simplify.py states every output in numpy and the tests hold the kernels to it bit for bit: a cluster's label is the LEAST
// index of its members, the sums are integers, of equal faces the LEAST index stays, so the outputs are a function of the mesh and
// the grid alone, whatever order the threads run in.
//
// Both tables are open addressing with linear probing over a power of two >= twice the number of keys.  A slot holds an index (a
// vertex, a face), claimed by a 32-bit atomicCAS on an empty slot; an occupied slot is compared by the key of its occupant, which an
// earlier kernel wrote.  Slots never empty again, so the probe path of a key is stable: where a key lands depends on the race, what
// its slot holds at the end (atomicMin) does not.  No thread waits for another; every probe loop is bounded by the table's capacity
// and raises the overflow word, which the caller reads with the totals, instead of going round again.  No floating-point atomics.
//
// The cell arithmetic is float32 and the means float64, each with one rounding per written operation (no contraction).
#include <cstdint>
#include "be_common.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kEmpty = 0xffffffffu;
constexpr float kIndexLimit = (float)(1 << BE_SIMPLIFY_INDEX_BITS);
constexpr float kFracScale = (float)(1 << BE_SIMPLIFY_FRAC_BITS);
constexpr int64_t kMaxCount = (int64_t)1 << 29;                        // vertices, triangles: a table of 2^30 slots at most

struct Grid {
    float o[3], inv[3];
    double od[3], cd[3];
};

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// wq of fusion.py: floorf(min(w, 16) * 65536 + 0.5) for w > 0, else 0 (NaN fails w > 0); no weights: 65536
__device__ __forceinline__ uint32_t quantise_weight(const float* __restrict__ weight, int64_t i) {
    if (!weight) return 65536u;
    const float w = weight[i];
    if (!(w > 0.0f)) return 0u;
    return (uint32_t)floorf(fminf(w, 16.0f) * 65536.0f + 0.5f);
}

// fq of fusion.py: floorf(clamp(f, -2048, 2048) * 65536 + 0.5), NaN counts as 0
__device__ __forceinline__ int64_t quantise_feat(float f) {
    const float fc = f != f ? 0.0f : fminf(fmaxf(f, -2048.0f), 2048.0f);
    return (int64_t)floorf(fc * 65536.0f + 0.5f);
}

// the cell of vertex v: i and q per axis; false when an index does not satisfy |i| < 2^20 (NaN and inf fail)
__device__ __forceinline__ bool cell_of(const float* __restrict__ vertices, int64_t v, const Grid& g, int32_t i[3], int64_t q[3]) {
    bool inside = true;
    for (int a = 0; a < 3; ++a) {
        const float t = (vertices[3 * v + a] - g.o[a]) * g.inv[a];
        const float fi = floorf(t);
        const float r = t - fi;
        const bool in = fabsf(fi) < kIndexLimit;
        i[a] = in ? (int32_t)fi : 0;
        q[a] = in ? (int64_t)(r * kFracScale) : 0;
        inside = inside && in;
    }
    return inside;
}

// thread v: the 63-bit key of its cell, or -1 for an unusable vertex
__global__ __launch_bounds__(256) void k_simplify_keys(const float* __restrict__ vertices, const float* __restrict__ weight, int64_t V, Grid g,
                                                       int64_t* __restrict__ key) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int32_t i[3];
    int64_t q[3];
    const bool usable = cell_of(vertices, v, g, i, q) && quantise_weight(weight, v) != 0u;
    const int64_t b = 1 << BE_SIMPLIFY_INDEX_BITS;
    key[v] = usable ? ((i[0] + b) << (2 * BE_SIMPLIFY_INDEX_BITS + 2)) | ((i[1] + b) << (BE_SIMPLIFY_INDEX_BITS + 1)) | (i[2] + b) : -1;
}

// thread v: into the cluster table.  A slot ends as the least vertex index of its key.
__global__ __launch_bounds__(256) void k_simplify_cluster_insert(const int64_t* __restrict__ key, int64_t V, uint32_t* __restrict__ table, uint32_t mask,
                                                                 uint32_t* __restrict__ slot_of, int64_t* __restrict__ overflow) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int64_t k = key[v];
    uint32_t found = kEmpty;
    if (k >= 0) {
        uint32_t s = (uint32_t)mix64((uint64_t)k) & mask;
        bool placed = false;
        for (uint64_t n = 0; n <= mask; ++n) {                           // at most the table's capacity
            const uint32_t old = atomicCAS(table + s, kEmpty, (uint32_t)v);
            if (old == kEmpty) { placed = true; break; }
            if ((int64_t)old < V && key[old] == k) {
                atomicMin(table + s, (uint32_t)v);
                placed = true;
                break;
            }
            s = (s + 1) & mask;
        }
        if (placed) found = s;
        else *overflow = 1;
    }
    slot_of[v] = found;
}

// thread v, after every insertion: the label and whether the vertex is its cluster's root
__global__ __launch_bounds__(256) void k_simplify_label(const uint32_t* __restrict__ table, const uint32_t* __restrict__ slot_of, int64_t V,
                                                        int32_t* __restrict__ label, uint8_t* __restrict__ is_root) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const uint32_t s = slot_of[v];
    const uint32_t l = s == kEmpty ? kEmpty : table[s];
    const bool ok = (int64_t)l < V;
    label[v] = ok ? (int32_t)l : -1;
    is_root[v] = ok && (int64_t)l == v ? 1 : 0;
}

// thread v: the dense id through the root's, and one more member there
__global__ __launch_bounds__(256) void k_simplify_ids(const int32_t* __restrict__ label, const int32_t* __restrict__ root_id, int64_t V,
                                                      int32_t* __restrict__ cluster, int32_t* __restrict__ members) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int32_t l = label[v];
    const int32_t c = l >= 0 ? root_id[l] : -1;
    cluster[v] = c;
    if (c >= 0 && c < V) atomicAdd(members + c, 1);
}

struct Sums {                                                            // rows of Vcap int64 each, indexed by dense id
    unsigned long long *sw, *sq, *sf, *swn, *sn;                         // [1], [3], [C], [1], [3] rows; swn, sn NULL without normals
};

// thread v: the integer sums of its cluster
__global__ __launch_bounds__(256) void k_simplify_sums(const float* __restrict__ vertices, const float* __restrict__ weight, const float* __restrict__ feat,
                                                       int C, const float* __restrict__ normal, const uint8_t* __restrict__ normal_valid, int64_t V, Grid g,
                                                       const int32_t* __restrict__ cluster, Sums s) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int32_t c = cluster[v];
    if (c < 0 || c >= V) return;
    int32_t i[3];
    int64_t q[3];
    cell_of(vertices, v, g, i, q);
    const int64_t wq = (int64_t)quantise_weight(weight, v);
    atomicAdd(s.sw + c, (unsigned long long)wq);
    for (int a = 0; a < 3; ++a) atomicAdd(s.sq + a * V + c, (unsigned long long)(wq * q[a]));
    for (int ch = 0; ch < C; ++ch) atomicAdd(s.sf + (int64_t)ch * V + c, (unsigned long long)(wq * quantise_feat(feat[(int64_t)ch * V + v])));
    if (s.swn && (!normal_valid || normal_valid[v])) {
        atomicAdd(s.swn + c, (unsigned long long)wq);
        for (int a = 0; a < 3; ++a) atomicAdd(s.sn + a * V + c, (unsigned long long)(wq * quantise_feat(normal[3 * v + a])));
    }
}

// the triple and winding of face f, or false when it is dropped: an index out of range, an unusable corner, two corners in one cluster
__device__ __forceinline__ bool face_triple(const int32_t* __restrict__ faces, int64_t f, int64_t V, const int32_t* __restrict__ cluster, int32_t tri[3],
                                            int* wind) {
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (!(i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < V && i1 < V && i2 < V)) return false;
    const int32_t a = cluster[i0], b = cluster[i1], c = cluster[i2];
    if (a < 0 || b < 0 || c < 0 || a == b || b == c || a == c) return false;
    int32_t x = a, y = b, z = c;                                         // rotated so that x is the least
    if (b < a && b < c) { x = b; y = c; z = a; }
    else if (c < a && c < b) { x = c; y = a; z = b; }
    *wind = y > z ? 1 : 0;
    tri[0] = x;
    tri[1] = y > z ? z : y;
    tri[2] = y > z ? y : z;
    return true;
}

// thread f: into the face table.  rep [cap] holds any face of the slot's triple, least [2 cap] the least face index of each winding.
__global__ __launch_bounds__(256) void k_simplify_face_insert(const int32_t* __restrict__ faces, int64_t V, int64_t T, const int32_t* __restrict__ cluster,
                                                              uint32_t* __restrict__ rep, uint32_t* __restrict__ least, uint32_t mask,
                                                              uint32_t* __restrict__ code, int64_t* __restrict__ overflow) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    int32_t tri[3], other[3];
    int wind = 0, w2 = 0;
    uint32_t found = kEmpty;
    if (face_triple(faces, f, V, cluster, tri, &wind)) {
        uint32_t s = (uint32_t)mix64(mix64((uint64_t)(uint32_t)tri[0]) ^ (((uint64_t)(uint32_t)tri[1] << 32) | (uint32_t)tri[2])) & mask;
        bool placed = false;
        for (uint64_t n = 0; n <= mask; ++n) {                           // at most the table's capacity
            const uint32_t old = atomicCAS(rep + s, kEmpty, (uint32_t)f);
            if (old == kEmpty || ((int64_t)old < T && face_triple(faces, old, V, cluster, other, &w2) && other[0] == tri[0] && other[1] == tri[1] &&
                                  other[2] == tri[2])) {
                atomicMin(least + 2 * (uint64_t)s + wind, (uint32_t)f);
                placed = true;
                break;
            }
            s = (s + 1) & mask;
        }
        if (placed) found = 2 * s + (uint32_t)wind;
        else *overflow = 1;
    }
    code[f] = found;
}

// thread f, after every insertion: the face stays iff it is its winding's least and, without flaps, the other winding is empty
__global__ __launch_bounds__(256) void k_simplify_face_flags(const uint32_t* __restrict__ least, const uint32_t* __restrict__ code, int64_t T, int flaps,
                                                             uint8_t* __restrict__ fflag) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    const uint32_t c = code[f];
    fflag[f] = c != kEmpty && (int64_t)least[c] == f && (flaps || least[c ^ 1u] == kEmpty) ? 1 : 0;
}

struct Emit {
    float *vertices, *weight, *feat, *normal;
    uint8_t* normal_valid;
    int32_t *faces, *face_index;
};

// thread i: root i writes its cluster's vertex to the slot of its dense id, kept face i goes to its slot foff[i] with its corners
// renumbered.  Every output element is written exactly once.
__global__ __launch_bounds__(256) void k_simplify_emit(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t V, int64_t T, Grid g,
                                                       const int32_t* __restrict__ label, const int32_t* __restrict__ cluster,
                                                       const int32_t* __restrict__ members, Sums s, int C, const uint8_t* __restrict__ fflag,
                                                       const int32_t* __restrict__ foff, int64_t V2, int64_t T2, Emit e) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < V && label[i] == (int32_t)i) {
        const int64_t o = cluster[i];
        if (o >= 0 && o < V2) {                                          // always, while V2 is the total the count phase reported
            int32_t ci[3];
            int64_t q[3];
            cell_of(vertices, i, g, ci, q);
            const double sw = (double)(int64_t)s.sw[o];
            for (int a = 0; a < 3; ++a) {
                double m = (double)(int64_t)s.sq[a * V + o] / sw;
                m = m * 0x1p-24;
                const double pos = ((double)ci[a] + m) * g.cd[a];
                e.vertices[3 * o + a] = (float)(g.od[a] + pos);
            }
            if (e.weight) e.weight[o] = (float)(sw / (double)members[o] * 0x1p-16);
            for (int ch = 0; ch < C; ++ch) e.feat[(int64_t)ch * V2 + o] = (float)((double)(int64_t)s.sf[(int64_t)ch * V + o] / sw * 0x1p-16);
            if (e.normal) {
                const int64_t wn = (int64_t)s.swn[o];
                float m[3];
                for (int a = 0; a < 3; ++a) m[a] = wn > 0 ? (float)((double)(int64_t)s.sn[a * V + o] / (double)wn * 0x1p-16) : 0.0f;
                const float l = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
                const bool valid = wn > 0 && l > 0.0f && l < __builtin_inff();
                for (int a = 0; a < 3; ++a) e.normal[3 * o + a] = valid ? m[a] / l : 0.0f;
                e.normal_valid[o] = valid ? 1 : 0;
            }
        }
    }
    if (i < T && fflag[i]) {
        const int64_t o = foff[i];
        if (o >= 0 && o < T2) {
            for (int k = 0; k < 3; ++k) {
                const int32_t j = faces[3 * i + k];
                e.faces[3 * o + k] = j >= 0 && j < V ? cluster[j] : -1;   // in range: the face was kept
            }
            e.face_index[o] = (int32_t)i;
        }
    }
}

size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }
dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
bool counts_ok(int64_t V, int64_t T) { return V >= 0 && T >= 0 && V <= kMaxCount && T <= kMaxCount; }

// the table for n keys: the power of two >= 2 n, at least 2
uint64_t capacity(int64_t n) {
    uint64_t c = 2;
    while (c < 2 * (uint64_t)n) c <<= 1;
    return c;
}

bool make_grid(const float* cell, const float* origin, Grid* g) {
    for (int a = 0; a < 3; ++a) {
        const float c = cell[a], o = origin[a];
        const float inv = (float)(1.0 / (double)c);
        if (!(c > 0.0f && c < __builtin_inff() && inv < __builtin_inff()) || !(o > -__builtin_inff() && o < __builtin_inff())) return false;
        g->o[a] = o;
        g->inv[a] = inv;
        g->od[a] = (double)o;
        g->cd[a] = (double)c;
    }
    return true;
}

int rows_of(int C, bool normals) { return 4 + C + (normals ? 4 : 0); }

Sums sums_of(int64_t* sums, int64_t V, int C, bool normals) {
    unsigned long long* p = reinterpret_cast<unsigned long long*>(sums);
    Sums s;
    s.sw = p;
    s.sq = p + V;
    s.sf = p + 4 * V;
    s.swn = normals ? p + (4 + (int64_t)C) * V : nullptr;
    s.sn = normals ? p + (5 + (int64_t)C) * V : nullptr;
    return s;
}

}  // namespace

extern "C" size_t be_mesh_cluster_workspace_bytes(int64_t V) {
    if (V < 0 || V > kMaxCount) return 0;
    const size_t n = (size_t)V;
    return pad8(n * 8) + pad8(capacity(V) * 4) + pad8(n * 4) + pad8(n) + pad8(n * 4) + be_exclusive_scan_workspace_bytes(V);
}

extern "C" int be_mesh_cluster_f32(const float* vertices, const float* weight, int64_t V, const float* cell, const float* origin, int32_t* label,
                                   int32_t* cluster, int32_t* members, int64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
    BE_REQUIRE(V >= 0 && V <= kMaxCount, "be_mesh_cluster_f32: V = %lld vertices; must be in [0, 2^29]", (long long)V);
    BE_REQUIRE(cell && origin && totals && workspace && (V == 0 || (vertices && label && cluster && members)), "be_mesh_cluster_f32: null pointer");
    Grid g;
    BE_REQUIRE(make_grid(cell, origin, &g), "be_mesh_cluster_f32: cell must be positive and finite (with a finite reciprocal) and origin finite");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= be_mesh_cluster_workspace_bytes(V),
               "be_mesh_cluster_f32: workspace must be 8-byte aligned and hold be_mesh_cluster_workspace_bytes(V) = %zu bytes, got %zu",
               be_mesh_cluster_workspace_bytes(V), workspace_bytes);
    const size_t n = (size_t)V;
    const uint64_t cap = capacity(V);
    char* ws = static_cast<char*>(workspace);
    int64_t* key = reinterpret_cast<int64_t*>(ws);
    ws += pad8(n * 8);
    uint32_t* table = reinterpret_cast<uint32_t*>(ws);
    ws += pad8(cap * 4);
    uint32_t* slot_of = reinterpret_cast<uint32_t*>(ws);
    ws += pad8(n * 4);
    uint8_t* is_root = reinterpret_cast<uint8_t*>(ws);
    ws += pad8(n);
    int32_t* root_id = reinterpret_cast<int32_t*>(ws);
    ws += pad8(n * 4);
    hipStream_t s = be::as_stream(stream);
    hipError_t e = hipMemsetAsync(totals + 1, 0, sizeof(int64_t), s);    // the overflow word
    if (V > 0) {
        if (e == hipSuccess) e = hipMemsetAsync(table, 0xff, cap * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(members, 0, n * 4, s);
    }
    if (e != hipSuccess) return be::fail(BE_ELAUNCH, "be_mesh_cluster_f32: hipMemsetAsync: %s", hipGetErrorString(e));
    if (V > 0) {
        hipLaunchKernelGGL(k_simplify_keys, grid_for(V), dim3(256), 0, s, vertices, weight, V, g, key);
        hipLaunchKernelGGL(k_simplify_cluster_insert, grid_for(V), dim3(256), 0, s, key, V, table, (uint32_t)(cap - 1), slot_of, totals + 1);
        hipLaunchKernelGGL(k_simplify_label, grid_for(V), dim3(256), 0, s, table, slot_of, V, label, is_root);
        if (const int rc = be::check_launch("be_mesh_cluster_f32(label)")) return rc;
    }
    if (const int rc = be_exclusive_scan_u8_i32(is_root, V, root_id, totals, ws, be_exclusive_scan_workspace_bytes(V), stream)) return rc;
    if (V > 0) hipLaunchKernelGGL(k_simplify_ids, grid_for(V), dim3(256), 0, s, label, root_id, V, cluster, members);
    return be::check_launch("be_mesh_cluster_f32(ids)");
}

extern "C" int be_mesh_simplify_sum_rows(int C, int normals) { return C >= 0 && C <= BE_FUSE_MAX_CHANNELS ? rows_of(C, normals != 0) : 0; }

extern "C" size_t be_mesh_simplify_workspace_bytes(int64_t T) {
    if (T < 0 || T > kMaxCount) return 0;
    return pad8(capacity(T) * 4) + pad8(capacity(T) * 8) + pad8((size_t)T * 4) + be_exclusive_scan_workspace_bytes(T);
}

extern "C" int be_mesh_simplify_count(const float* vertices, const int32_t* faces, int64_t V, int64_t T, const float* weight, const float* feat, int C,
                                      const float* normal, const uint8_t* normal_valid, const float* cell, const float* origin, const int32_t* cluster,
                                      int flaps, int64_t* sums, uint8_t* fflag, int32_t* foff, int64_t* totals, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    BE_REQUIRE(counts_ok(V, T), "be_mesh_simplify_count: V = %lld vertices and T = %lld triangles; both must be in [0, 2^29]", (long long)V,
               (long long)T);
    BE_REQUIRE(C >= 0 && C <= BE_FUSE_MAX_CHANNELS, "be_mesh_simplify_count: C must be in [0, %d]", BE_FUSE_MAX_CHANNELS);
    BE_REQUIRE(cell && origin && totals && workspace && (V == 0 || (vertices && cluster && sums && (C == 0 || feat))) && (T == 0 || (faces && fflag && foff)),
               "be_mesh_simplify_count: null pointer");
    BE_REQUIRE(!normal_valid || normal, "be_mesh_simplify_count: normal_valid needs normal");
    Grid g;
    BE_REQUIRE(make_grid(cell, origin, &g), "be_mesh_simplify_count: cell must be positive and finite (with a finite reciprocal) and origin finite");
    BE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && workspace_bytes >= be_mesh_simplify_workspace_bytes(T),
               "be_mesh_simplify_count: workspace must be 8-byte aligned and hold be_mesh_simplify_workspace_bytes(T) = %zu bytes, got %zu",
               be_mesh_simplify_workspace_bytes(T), workspace_bytes);
    const uint64_t cap = capacity(T);
    char* ws = static_cast<char*>(workspace);
    uint32_t* rep = reinterpret_cast<uint32_t*>(ws);
    ws += pad8(cap * 4);
    uint32_t* least = reinterpret_cast<uint32_t*>(ws);
    ws += pad8(cap * 8);
    uint32_t* code = reinterpret_cast<uint32_t*>(ws);
    ws += pad8((size_t)T * 4);
    hipStream_t s = be::as_stream(stream);
    hipError_t e = hipMemsetAsync(totals + 1, 0, sizeof(int64_t), s);    // the overflow word
    if (e == hipSuccess && V > 0) e = hipMemsetAsync(sums, 0, (size_t)rows_of(C, normal != nullptr) * (size_t)V * sizeof(int64_t), s);
    if (e == hipSuccess && T > 0) e = hipMemsetAsync(rep, 0xff, pad8(cap * 4) + cap * 8, s);   // rep and least lie together
    if (e != hipSuccess) return be::fail(BE_ELAUNCH, "be_mesh_simplify_count: hipMemsetAsync: %s", hipGetErrorString(e));
    if (V > 0)
        hipLaunchKernelGGL(k_simplify_sums, grid_for(V), dim3(256), 0, s, vertices, weight, feat, C, normal, normal_valid, V, g, cluster,
                           sums_of(sums, V, C, normal != nullptr));
    if (T > 0) {
        hipLaunchKernelGGL(k_simplify_face_insert, grid_for(T), dim3(256), 0, s, faces, V, T, cluster, rep, least, (uint32_t)(cap - 1), code, totals + 1);
        hipLaunchKernelGGL(k_simplify_face_flags, grid_for(T), dim3(256), 0, s, least, code, T, flaps ? 1 : 0, fflag);
    }
    if (const int rc = be::check_launch("be_mesh_simplify_count")) return rc;
    return be_exclusive_scan_u8_i32(fflag, T, foff, totals, ws, be_exclusive_scan_workspace_bytes(T), stream);
}

extern "C" int be_mesh_simplify_emit(const float* vertices, const int32_t* faces, int64_t V, int64_t T, const float* cell, const float* origin,
                                     const int32_t* label, const int32_t* cluster, const int32_t* members, const int64_t* sums, int C, int normals,
                                     const uint8_t* fflag, const int32_t* foff, int64_t V2, int64_t T2, float* vertices_out, int32_t* faces_out,
                                     float* weight_out, float* feat_out, float* normal_out, uint8_t* normal_valid_out, int32_t* face_index,
                                     void* stream) {
    BE_REQUIRE(counts_ok(V, T), "be_mesh_simplify_emit: V = %lld vertices and T = %lld triangles; both must be in [0, 2^29]", (long long)V, (long long)T);
    BE_REQUIRE(V2 >= 0 && V2 <= V && T2 >= 0 && T2 <= T, "be_mesh_simplify_emit: V2 = %lld and T2 = %lld must lie in [0, V] and [0, T]", (long long)V2,
               (long long)T2);
    BE_REQUIRE(C >= 0 && C <= BE_FUSE_MAX_CHANNELS, "be_mesh_simplify_emit: C must be in [0, %d]", BE_FUSE_MAX_CHANNELS);
    BE_REQUIRE(cell && origin && (V == 0 || (vertices && label && cluster && members && sums)) && (T == 0 || (faces && fflag && foff)),
               "be_mesh_simplify_emit: null input");
    BE_REQUIRE((V2 == 0 || (vertices_out && (C == 0 || feat_out))) && (T2 == 0 || (faces_out && face_index)), "be_mesh_simplify_emit: null output");
    BE_REQUIRE(V2 == 0 || ((normals != 0) == (normal_out != nullptr) && (normal_out != nullptr) == (normal_valid_out != nullptr)),
               "be_mesh_simplify_emit: normal_out and normal_valid_out are given exactly when the sums hold normals");
    Grid g;
    BE_REQUIRE(make_grid(cell, origin, &g), "be_mesh_simplify_emit: cell must be positive and finite (with a finite reciprocal) and origin finite");
    if (V2 == 0 && T2 == 0) return BE_OK;
    Emit e;
    e.vertices = vertices_out; e.weight = weight_out; e.feat = feat_out; e.normal = normal_out; e.normal_valid = normal_valid_out;
    e.faces = faces_out; e.face_index = face_index;
    const int64_t n = V > T ? V : T;
    hipLaunchKernelGGL(k_simplify_emit, grid_for(n), dim3(256), 0, be::as_stream(stream), vertices, faces, V, T, g, label, cluster, members,
                       sums_of(const_cast<int64_t*>(sums), V, C, normals != 0), V2 > 0 ? C : 0, fflag, foff, V2, T2, e);
    return be::check_launch("be_mesh_simplify_emit");
}
