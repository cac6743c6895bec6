// LocalStage.forward (eval) as a chain of launches on one stream: models/local_stage.py:63-73.
//   conv7x7+BN+Smish -> maxpool(3,2,1) -> block 64->96 @11^2 -> maxpool(3,2,1) -> blocks 96->256, 256->384,
//   384->256 @6^2 -> maxpool(2,2) -> flatten -> Linear 2304->1024 + BN1d + Smish -> Linear 1024->10
// Activations are NHWC in a caller-provided workspace; the batch is walked in sub-batches (default 8192 patches,
// measured best) so the workspace stays bounded whatever N is.  Per sub-batch: staging, conv1, 2-3 pools, layer0 as two direct
// launches (conv1; conv2 with the downsample fused in), the second pool with layer1's input transform in it, layers 1-3 each as
// the chained Winograd pair (40 GEMMs, output+input transform, 40 GEMMs - the 1x1 downsample a second K segment of 18 of them, over
// the block's own input transform -, output transform - layers 1 and 2's with the next layer's input transform in it, layer3's with
// the 2x2 max-pool in it; be_wino.hip), fc.1, fc.4: 21 launches.  BE_WINO_DS_GEMM=1 (read once per process; also BE_ROWS_F32=1,
// BE_WINO_F32=1): the downsample as its own 1x1 launch in front of each pair, joined behind conv2's output transform
// (24 launches; round 13's bits).
// BE_WINO_NO_CHAIN=1 (read once per process): the unchained launches - k_maxpool_nhwc, and every layer from k_wino_in to
// k_wino_out - with the same bits.  Sub-batches of 512 patches and more take the LDS-DMA kernels (be_conv_pm.hip for conv1 on a
// row-padded staging and for layer0, the row GEMM of be_wino.hip for the 1x1s and fc.1); smaller ones k_conv_igemm - same
// results bit for bit.  On the Winograd path the 1x1 downsamples of layers 1-3 and fc.1 run in split-bf16 arithmetic on ONE kernel for
// every sub-batch size (be::gemm_rows_bf6; BE_ROWS_F32=1 / BE_WINO_F32=1: the fp32 kernels just named), and so does layer0
// (be::conv3x3_pm_bf6, be_conv_pm_bf6.hip; BE_L0_F32=1 / BE_WINO_F32=1: the fp32 kernels; its LDS ring is 42 KB, three workgroups
// per CU), and so do conv1 + the first pool
// (be_conv1_pool_bf6.hip on the row-padded staging; BE_C1_F32=1 / BE_WINO_F32=1: the fp32 routing by sub-batch size).  No allocation, no
// synchronisation, no process-wide state: graph-capturable, re-entrant.  opts->winograd = 0 runs layers 1-3 as direct launches
// like layer0, all in fp32.
// Three facts are each stated once below: where a piece lies in the packed buffer (Layout: one ordered table of regions, asked
// for by (layer, form)), where a map lies in the workspace (the Span constants and their static_asserts; carve), and which
// kernels a sub-batch takes (Knobs, read once per process; route_of).
#include "be_common.h"
#include <cstdlib>
#include <initializer_list>

namespace {

struct LayerSpec { int cout, cin, ks, chw_hw; };
// state_dict() order; conv1 consumes the NHWC4 staging of the NCHW input
constexpr LayerSpec kLayers[15] = {
    {64, 3, 7, 0},
    {96, 64, 3, 0},   {96, 96, 3, 0},   {96, 64, 1, 0},
    {256, 96, 3, 0},  {256, 256, 3, 0}, {256, 96, 1, 0},
    {384, 256, 3, 0}, {384, 384, 3, 0}, {384, 256, 1, 0},
    {256, 384, 3, 0}, {256, 256, 3, 0}, {256, 384, 1, 0},
    {1024, 2304, 1, 9},
    {10, 1024, 1, 0},
};
// the residual blocks (layer0 .. layer3): their three layers and the side of the map they run on
struct Block { int conv1, conv2, ds, hw; };
constexpr Block kBlocks[4] = {{1, 2, 3, 11}, {4, 5, 6, 6}, {7, 8, 9, 6}, {10, 11, 12, 6}};
inline const Block* block_of(int layer) {
    for (const Block& b : kBlocks) if (layer == b.conv1 || layer == b.conv2 || layer == b.ds) return &b;
    return nullptr;
}

inline size_t cout_pad(int c) { return (size_t)((c + 31) / 32 * 32); }

// The forms a layer's parameters are packed in (be_local_stage_layout_debug reports these numbers)
enum Form {
    F32,        // the fp32 matrix and bias (be_conv_pack_f32): conv1, each block's conv1, fc.1, fc.4
    FUSED2,     // a block's conv2 with its downsample's columns, biases summed (be_conv_pack_fused2_f32)
    WINO,       // Winograd U with its planes, and the bias (be_wino_pack_f32; be_wino_math.h: 8x5 tiles): the 3x3s of the 6x6 blocks
    DS_F32,     // a 6x6 block's 1x1 downsample as a stand-alone fp32 convolution; its bias is ADDED to conv2's WINO bias after both are packed
    ROWS_BF6,   // hi / mid / lo bf16 planes of a DS_F32 / fc.1's F32 matrix (split-bf16 row GEMM)
    L0_BF6,     // layer0's pixel-major planes, made from its F32 / FUSED2 matrix; the bias is that form's
    WINO_DS,    // a 6x6 block's downsample as conv2's second K segment in the transform domain (be_wino_ds_pack_f32)
    ZERO,       // 384 zero floats: the "bias" of the bias-free fp32 downsample launch
    FORMS
};

// One piece of the packed buffer: a matrix part and a bias part (either may be empty), in floats.  reads: the table index of the
// region whose matrix this region's pack call reads (BatchNorm already folded there), -1: packed from the state-dict tensors.
struct Region { int layer, form; size_t w_off, w_n, b_off, b_n; int reads; };

struct Layout {
    Region r[32];
    int n = 0, zero = -1, at_[15][FORMS];
    size_t total = 0;
    int add(int layer, Form f, size_t w_n, size_t b_n, int reads = -1) {
        r[n] = {layer, f, total, w_n, total + w_n, b_n, reads};
        total += w_n + b_n;
        if (layer >= 0) at_[layer][f] = n;
        return n++;
    }
    // the table, in the order of the buffer
    Layout() {
        for (auto& row : at_) for (int& v : row) v = -1;
        for (int i = 0; i < 15; ++i) {                 // every layer in index order; a downsample lies in its conv2's FUSED2
            const LayerSpec& s = kLayers[i];
            const Block* b = block_of(i);
            if (b && i == b->ds) continue;
            if (b && i == b->conv2) add(i, FUSED2, be_conv_fused2_packed_floats(s.cout, s.cin, s.ks, kLayers[b->ds].cin), cout_pad(s.cout));
            else add(i, F32, be_conv_packed_floats(s.cout, s.cin, s.ks), cout_pad(s.cout));
        }
        for (int i = kBlocks[1].conv1; i <= kBlocks[3].ds; ++i) {      // the 6x6 blocks again, as the Winograd path reads them
            const LayerSpec& s = kLayers[i];
            if (i == block_of(i)->ds) add(i, DS_F32, be_conv_packed_floats(s.cout, s.cin, 1), cout_pad(s.cout));
            else add(i, WINO, be_wino_packed_floats(s.cout, s.cin), cout_pad(s.cout));
        }
        zero = add(-1, ZERO, 0, 384);
        for (int i : {kBlocks[1].ds, kBlocks[2].ds, kBlocks[3].ds, 13})
            add(i, ROWS_BF6, be_gemm_rows_bf6_packed_floats(kLayers[i].cout, kLayers[i].cin), 0, at_[i][i == 13 ? F32 : DS_F32]);
        const Block& l0 = kBlocks[0];                  // K order of the packed matrices = the pixel-major K walk
        add(l0.conv1, L0_BF6, be_conv3x3_pm_bf6_packed_floats(kLayers[l0.conv1].cout, kLayers[l0.conv1].cin, 0), 0, at_[l0.conv1][F32]);
        add(l0.conv2, L0_BF6, be_conv3x3_pm_bf6_packed_floats(kLayers[l0.conv2].cout, kLayers[l0.conv2].cin, kLayers[l0.ds].cin), 0,
            at_[l0.conv2][FUSED2]);
        for (int k = 1; k < 4; ++k)                    // (round 14: behind all else)
            add(kBlocks[k].ds, WINO_DS, be_wino_ds_packed_floats(kLayers[kBlocks[k].ds].cout, kLayers[kBlocks[k].ds].cin), 0);
    }
    const Region& at(int layer, Form f) const { return r[at_[layer][f]]; }
    const float* w(const float* packed, int layer, Form f) const { return packed + at(layer, f).w_off; }
    const float* b(const float* packed, int layer, Form f) const { return packed + at(layer, f).b_off; }
};
const Layout& layout() { static Layout l; return l; }

// The workspace, in floats per patch: a sub-batch of nb patches has nb times each number, regions and what lies in them alike.
struct Span { size_t at, n; };
constexpr size_t end(Span s) { return s.at + s.n; }
constexpr bool inside(Span s, Span host) { return s.at >= host.at && end(s) <= end(host); }
constexpr bool apart(Span a, Span b) { return end(a) <= b.at || end(b) <= a.at; }
// RA holds conv1's output, then each block's intermediate t and last fc.1's output; RB and RC the blocks' inputs and outputs in turn.
// Winograd path: RW = transform-domain input + output of the widest layer (room for 100 values per channel: 25 positions x 4 tiles;
// the 8x5 tiles use 80; 384 + 384 channels, and round 14: a block that folds its downsample into conv2's GEMMs keeps three
// transform-domain buffers, be_wino_pair_ds_workspace_floats), RR = the block's downsample branch [6,6,384]
constexpr Span RA = {0, 28224}, RB = {end(RA), 13824}, RC = {end(RB), 13824}, RW = {end(RC), 100 * (384 + 384 + 384)}, RR = {end(RW), 13824};
constexpr size_t WS_FLOATS_PER_PATCH = end(RR);
constexpr size_t map_floats(int hw, int c) { return (size_t)hw * hw * c; }
// the staging [21,21,4], or with 28 pixels per row (3 zero pixels left, 4 right: the pixel-major conv1 kernels); the first pool's
// output p1 lies behind it in RB, so that the staging can die into it: behind TWO plain stagings, which is behind one padded one
constexpr Span X4 = {RB.at, 21 * 21 * 4}, X4P = {RB.at, 21 * 28 * 4}, P1 = {RB.at + 2 * X4.n, map_floats(11, 64)};
constexpr Span C1 = {RA.at, map_floats(21, 64)};
// block k: its input, conv1's result t (which a Winograd block keeps in registers: k_wino_out_in) and its output
constexpr Span blk_in(int k, size_t at) { return {at, map_floats(kBlocks[k].hw, kLayers[kBlocks[k].conv1].cin)}; }
constexpr Span blk_out(int k, size_t at) { return {at, map_floats(kBlocks[k].hw, kLayers[kBlocks[k].conv1].cout)}; }
constexpr Span P2 = blk_in(1, RB.at);                  // the second pool's output
constexpr Span BIN[4] = {P1, P2, blk_in(2, RC.at), blk_in(3, RB.at)};
constexpr Span BT[4] = {blk_out(0, RA.at), blk_out(1, RA.at), blk_out(2, RA.at), blk_out(3, RA.at)};
constexpr Span BOUT[4] = {blk_out(0, RC.at), blk_out(1, RC.at), blk_out(2, RB.at), blk_out(3, RC.at)};
// maxpool(2,2) of layer3 = the (H,W,C) flatten.  Winograd path: layer3's output transform pools in registers and writes p3 where the
// direct path's full map would lie (RB is still the block's input); the direct path pools that map into RB
constexpr Span P3_WINO = {RC.at, map_floats(3, 256)}, P3_DIRECT = {RB.at, map_floats(3, 256)}, F1 = {RA.at, 1024};
constexpr Span DS = {RR.at, map_floats(6, 384)};       // the 1x1 downsample's raw accumulators where it is a launch of its own

static_assert(apart(X4, P1) && apart(X4P, P1) && inside(X4, RB) && inside(X4P, RB) && inside(P1, RB), "staging | p1 side by side in RB");
static_assert(inside(C1, RA) && apart(C1, P1), "conv1's map fills RA");
static_assert(inside(BIN[0], RB) && inside(BT[0], RA) && inside(BOUT[0], RC), "layer0: RB -> RA -> RC");
static_assert(inside(P2, RB) && apart(P2, BOUT[0]), "the second pool: RC -> RB");
static_assert(BIN[2].n == BOUT[1].n && BIN[2].at == BOUT[1].at && BIN[3].n == BOUT[2].n && BIN[3].at == BOUT[2].at, "a block reads what the last one wrote");
static_assert(inside(BIN[1], RB) && inside(BT[1], RA) && inside(BOUT[1], RC), "layer1: RB -> RA -> RC");
static_assert(inside(BIN[2], RC) && inside(BT[2], RA) && inside(BOUT[2], RB), "layer2: RC -> RA -> RB");
static_assert(inside(BIN[3], RB) && inside(BT[3], RA) && inside(BOUT[3], RC), "layer3: RB -> RA -> RC");
static_assert(inside(P3_WINO, RC) && apart(P3_WINO, BIN[3]) && inside(P3_DIRECT, RB) && apart(P3_DIRECT, BOUT[3]), "p3 beside what it is pooled from");
static_assert(inside(F1, RA) && apart(F1, P3_WINO) && apart(F1, P3_DIRECT), "fc.1: p3 -> RA");
static_assert(inside(DS, RR) && DS.n >= BOUT[1].n && DS.n >= BOUT[2].n && DS.n >= BOUT[3].n, "the downsample branch of the widest block");
static_assert(WS_FLOATS_PER_PATCH == 28224 + 3 * 13824 + 115200, "be_local_stage_workspace_bytes: 739 584 B per patch");

// one sub-batch's pointers
struct Carved {
    float *x4, *c1, *p1, *p2, *p3, *f1, *in[4], *t[4], *out[4], *wino, *ds;
    size_t wino_floats;
};
Carved carve(float* ws, int nb, bool wino) {
    const auto at = [&](Span s) { return ws + (size_t)nb * s.at; };
    Carved c;
    c.x4 = at(X4); c.c1 = at(C1); c.p1 = at(P1); c.p2 = at(P2); c.p3 = at(wino ? P3_WINO : P3_DIRECT); c.f1 = at(F1);
    for (int k = 0; k < 4; ++k) { c.in[k] = at(BIN[k]); c.t[k] = at(BT[k]); c.out[k] = at(BOUT[k]); }
    c.wino = at(RW); c.wino_floats = (size_t)nb * RW.n; c.ds = at(DS);
    return c;
}

constexpr int kDefaultChunk = 8192;   // measured: 8192 > 4096 > 2048 (fewer partial rounds of the 512 resident blocks)
inline int chunk_of(int chunk) { return chunk > 0 ? chunk : kDefaultChunk; }

// The knobs this file reads, once per process.  BE_NO_CONV_PM and BE_NO_CONV1_POOL (A/B knobs of the fp32 routing): set at all;
// BE_WINO_NO_CHAIN: set and not 0; the four arithmetic arms: their kernels' own answers (be_common.h)
struct Knobs { bool no_conv_pm, no_conv1_pool, no_chain, l0_bf6, rows_bf6, c1_bf6, ds_fold; };
const Knobs& knobs() {
    static const Knobs k = {getenv("BE_NO_CONV_PM") != nullptr, getenv("BE_NO_CONV1_POOL") != nullptr, be::knob_on("BE_WINO_NO_CHAIN"),
                            be::l0_bf6_enabled(), be::rows_bf6_enabled(), be::c1_bf6_enabled(), be::wino_ds_fold_enabled()};
    return k;
}

// Which kernels a sub-batch of nb patches takes (be_local_stage_route_debug reports these numbers, in this order)
enum Staging { STAGE_NHWC4, STAGE_NHWC4P };
enum Conv1 { C1_IGEMM, C1_PM, C1_POOL, C1_POOL_BF6 };       // k_conv_igemm; the pixel-major LDS-DMA kernel; fp32 / split-bf16 conv1 + pool
enum Blocks6 { B6_DIRECT, B6_WINO_FOLD, B6_WINO_DS_BF6, B6_WINO_DS_F32 };
struct Route {
    int staging;      // Staging: the padded rows are what the three pixel-major conv1 forms read
    int conv1;        // Conv1
    int conv1_pools;  // conv1's launch writes p1 (no k_maxpool_nhwc, conv1's map never reaches HBM)
    int l0_bf6;       // layer0 in split-bf16 arithmetic, else the fp32 kernels
    int chain;        // the Winograd blocks chained through the start of RW (header comment; be::wino_pair)
    int blocks6;      // Blocks6: direct fused convolutions, or Winograd with the downsample folded / a split-bf16 launch / an fp32 launch
    int store_maps;   // the second pool's map and the maps between the 6x6 blocks are written (chained and folded: nothing reads them)
    int fc1_bf6;      // fc.1 on the split-bf16 row GEMM, else the fp32 convolution
};
constexpr int kRouteFields = 8;
Route route_of(const Knobs& k, int winograd, int nb) {
    const bool wino = winograd != 0;
    // Winograd path: conv1 + Smish + the first max-pool in split-bf16 arithmetic at EVERY sub-batch size, so that a patch's bits
    // depend on neither batch nor chunk; else the fp32 routing: large sub-batches on the pixel-major kernels, fused with the pool
    // (bit-identical to the pair) unless BE_NO_CONV1_POOL
    const bool c1_bf6 = wino && k.c1_bf6 && !k.no_conv_pm && !k.no_conv1_pool;
    const bool padded = c1_bf6 || (nb >= 512 && !k.no_conv_pm);
    Route r;
    r.staging = padded ? STAGE_NHWC4P : STAGE_NHWC4;
    r.conv1 = !padded ? C1_IGEMM : c1_bf6 ? C1_POOL_BF6 : !k.no_conv1_pool ? C1_POOL : C1_PM;
    r.conv1_pools = r.conv1 == C1_POOL || r.conv1 == C1_POOL_BF6;
    r.l0_bf6 = wino && k.l0_bf6;
    r.chain = wino && !k.no_chain;
    r.blocks6 = !wino ? B6_DIRECT : k.ds_fold ? B6_WINO_FOLD : k.rows_bf6 ? B6_WINO_DS_BF6 : B6_WINO_DS_F32;
    r.store_maps = !(r.chain && r.blocks6 == B6_WINO_FOLD);
    r.fc1_bf6 = wino && k.rows_bf6;
    return r;
}

}  // namespace

extern "C" size_t be_local_stage_packed_floats(void) { return layout().total; }

extern "C" size_t be_local_stage_workspace_bytes(int64_t n, int chunk) {
    if (n <= 0) return 0;
    const int64_t nb = n < chunk_of(chunk) ? n : chunk_of(chunk);
    return (size_t)nb * WS_FLOATS_PER_PATCH * sizeof(float);
}

namespace {

// the pack call of one region
int pack_region(const Layout& L, const Region& r, const float* const* t, float bn_eps, float* packed, void* stream) {
    float *w = packed + r.w_off, *b = packed + r.b_off;
    if (r.form == ZERO)
        return hipMemsetAsync(b, 0, r.b_n * sizeof(float), be::as_stream(stream)) == hipSuccess
                   ? BE_OK : be::fail(BE_ELAUNCH, "be_local_stage_pack_f32: hipMemsetAsync failed");
    // weight, bias, then BatchNorm's gamma, beta, mean, var: 6 tensors per layer (fc.1's BatchNorm1d is fc.2), fc.4 has the first two
    const float* const* e = t + 6 * r.layer;
    const float *g = r.layer == 14 ? nullptr : e[2], *bt = g ? e[3] : nullptr, *m = g ? e[4] : nullptr, *v = g ? e[5] : nullptr;
    const LayerSpec& s = kLayers[r.layer];
    const Block* k = block_of(r.layer);
    const float* src = r.reads >= 0 ? packed + L.r[r.reads].w_off : nullptr;
    switch (r.form) {
    case F32: return be_conv_pack_f32(e[0], e[1], g, bt, m, v, bn_eps, s.cout, s.cin, s.ks, s.chw_hw, w, b, stream);
    case FUSED2: {
        const float* const* d = t + 6 * k->ds;         // the block's downsample conv + BN
        return be_conv_pack_fused2_f32(e[0], e[1], g, bt, m, v, d[0], d[1], d[2], d[3], d[4], d[5], bn_eps, s.cout, s.cin, s.ks,
                                       kLayers[k->ds].cin, w, b, stream);
    }
    case WINO: return be_wino_pack_f32(e[0], e[1], g, bt, m, v, bn_eps, s.cout, s.cin, w, b, stream);
    case DS_F32: return be_conv_pack_f32(e[0], e[1], g, bt, m, v, bn_eps, s.cout, s.cin, 1, 0, w, b, stream);
    case ROWS_BF6: return be_gemm_rows_bf6_pack_f32(src, s.cout, s.cin, w, stream);
    case L0_BF6: return be_conv3x3_pm_bf6_pack_f32(src, s.cout, s.cin, r.layer == k->conv2 ? kLayers[k->ds].cin : 0, w, stream);
    default: return be_wino_ds_pack_f32(e[0], e[1], g, bt, m, v, bn_eps, s.cout, s.cin, w, nullptr, stream);      // WINO_DS
    }
}

}  // namespace

// The order of the calls is part of the contract (profiles/HISTORY.md rounds 28-29: an open fault is sensitive to what follows
// what): each step packs, in table order, the regions of the named forms whose layer lies in [lo, hi]
extern "C" int be_local_stage_pack_f32(const float* const* t, float bn_eps, float* packed, void* stream) {
    BE_REQUIRE(t && packed, "be_local_stage_pack_f32: null pointer");
    for (int i = 0; i < BE_LOCAL_STAGE_NTENSORS; ++i) BE_REQUIRE(t[i], "be_local_stage_pack_f32: tensor %d is null", i);
    const Layout& L = layout();
    const auto step = [&](unsigned forms, int lo, int hi) {
        for (int k = 0; k < L.n; ++k) {
            if (!((forms >> L.r[k].form) & 1) || L.r[k].layer < lo || L.r[k].layer > hi) continue;
            if (int rc = pack_region(L, L.r[k], t, bn_eps, packed, stream)) return rc;
        }
        return (int)BE_OK;
    };
    int rc;
    if ((rc = step((1u << F32) | (1u << FUSED2), 0, 12))) return rc;        // conv + BatchNorm2d pairs
    if ((rc = step((1u << WINO) | (1u << DS_F32), 0, 12))) return rc;       // 6x6 blocks again, in the form the Winograd path reads
    // Winograd blocks: the downsample's (folded) bias moves into conv2's, so that the 1x1 downsample itself is a bias-free GEMM -
    // raw accumulators, which the weight-stationary GEMM kernel can write (be::gemm_rows_ws) - and joins in conv2's output
    // transform exactly as before: y = act(A^T M A + (b2 + b_ds) + x W_ds)
    for (int k = 1; k < 4; ++k) {
        const Block& b = kBlocks[k];
        if ((rc = be::vec_add_inplace(packed + L.at(b.conv2, WINO).b_off, L.b(packed, b.ds, DS_F32), (int)L.at(b.conv2, WINO).b_n, stream)))
            return rc;
    }
    if ((rc = step(1u << ZERO, -1, -1))) return rc;
    if ((rc = step(1u << F32, 13, 14))) return rc;                      // fc.1 (+ fc.2), fc.4
    // planes from the packed fp32 matrices (BatchNorm folded, fc.1's columns permuted), which stay for the fp32 arms: Region::reads
    if ((rc = step(1u << ROWS_BF6, 0, 14))) return rc;
    if ((rc = step(1u << WINO_DS, 0, 14))) return rc;
    return step(1u << L0_BF6, 0, 14);
}

namespace {

int conv(const Layout& L, const float* packed, int li, const float* x, const float* res, float* y, int n, int hw, int act, int ldy,
         void* stream) {
    be_conv_desc d;
    d.n = n; d.h = hw; d.w = hw;
    d.cin = li == 0 ? 4 : kLayers[li].cin;
    d.cout = kLayers[li].cout; d.ksize = kLayers[li].ks; d.act = act;
    return be_conv_nhwc_f32(&d, x, L.w(packed, li, F32), L.b(packed, li, F32), res, y, ldy, stream);
}

// ResidualBlock (models/local_stage.py:20-28): Smish(BN(conv3(Smish(BN(conv3(x))))) + BN(conv1x1(x))) in two launches:
// the downsample 1x1 rides in the K loop of conv2 (be_conv_nhwc_fused2_f32), no residual tensor in HBM
int block(const Layout& L, const float* packed, const Block& b, const float* x, float* t, float* o, int n, void* stream) {
    const int c = kLayers[b.conv1].cout;
    if (int rc = conv(L, packed, b.conv1, x, nullptr, t, n, b.hw, 1, c, stream)) return rc;
    be_conv_desc d;
    d.n = n; d.h = b.hw; d.w = b.hw; d.cin = kLayers[b.conv2].cin; d.cout = c; d.ksize = 3; d.act = 1;
    return be_conv_nhwc_fused2_f32(&d, t, x, kLayers[b.ds].cin, L.w(packed, b.conv2, FUSED2), L.b(packed, b.conv2, FUSED2), o, c, stream);
}

// layer0's block in split-bf16 arithmetic (be_conv_pm_bf6.hip): the same two launches on ONE kernel for every sub-batch size
int block_l0_bf6(const Layout& L, const float* packed, const float* x, float* t, float* o, int n, void* stream) {
    const Block& b = kBlocks[0];
    be_conv_desc d;
    d.n = n; d.h = b.hw; d.w = b.hw; d.cin = kLayers[b.conv1].cin; d.cout = 96; d.ksize = 3; d.act = 1;
    if (int rc = be::conv3x3_pm_bf6(&d, x, nullptr, 0, L.w(packed, b.conv1, L0_BF6), L.b(packed, b.conv1, F32), t, 96, stream)) return rc;
    d.cin = kLayers[b.conv2].cin;
    return be::conv3x3_pm_bf6(&d, t, x, kLayers[b.ds].cin, L.w(packed, b.conv2, L0_BF6), L.b(packed, b.conv2, FUSED2), o, 96, stream);
}

// The same block on a 6x6 map with both 3x3 convolutions in Winograd F(3x3,3x3) form (be_wino.hip): 2.56x fewer multiplies
// than the direct form; conv1's result only ever exists in registers (k_wino_out_in).  route.chain: the block as a link of the chain
// (be::wino_pair): x's transform is already in `w`, and with next_cmid > 0 the next block's is left there.
// B6_WINO_FOLD (round 14, the default): the downsample is a second K segment of conv2's GEMMs over x's transform (be::wino_pair's
// ds_planes); a chained block reads and writes transforms only, so x and - with next_cmid - o are not passed.  The other two
// forms run the 1x1 downsample as its own convolution into `r`, which joins in the output transform of conv2.
int block_wino(const Layout& L, const float* packed, const Route& route, const Block& b, const float* x, float* o, float* r, float* w,
               size_t w_floats, int n, void* stream, int pool2, int next_cmid) {
    const int c = kLayers[b.conv1].cout, cin = kLayers[b.conv1].cin, x_in_v = route.chain;
    const float *u1 = L.w(packed, b.conv1, WINO), *b1 = L.b(packed, b.conv1, WINO), *u2 = L.w(packed, b.conv2, WINO),
                *b2 = L.b(packed, b.conv2, WINO);
    if (route.blocks6 == B6_WINO_FOLD) {
        const bool bare = x_in_v && next_cmid > 0;    // nothing reads the block's output map
        return be::wino_pair(x_in_v ? nullptr : x, u1, b1, 1, u2, b2, nullptr, 1, bare ? nullptr : o, n, cin, c, c, w, w_floats, stream,
                             pool2, x_in_v, next_cmid, L.w(packed, b.ds, WINO_DS));
    }
    // the 1x1 downsample, bias-free (its bias sits in conv2's, see be_local_stage_pack_f32), raw accumulators: the split-bf16 row
    // GEMM at every batch size.  fp32 arm (BE_ROWS_F32=1 / BE_WINO_F32=1): large sub-batches on the weight-stationary GEMM
    // (128 TFLOP/s where the row GEMM does 92-119), others - its answer at run time - on the general kernel with a zero bias
    if (route.blocks6 == B6_WINO_DS_BF6) {
        if (int rc = be::gemm_rows_bf6(x, (int64_t)n * 36, cin, L.w(packed, b.ds, ROWS_BF6), c, nullptr, nullptr, 0, r, c, stream)) return rc;
    } else {
        int rc = be::gemm_rows_ws(x, (int64_t)n * 36, cin, L.w(packed, b.ds, DS_F32), c, r, c, stream);
        if (rc < 0) return rc;
        if (rc > 0) {
            be_conv_desc d;
            d.n = n; d.h = 6; d.w = 6; d.cin = cin; d.cout = c; d.ksize = 1; d.act = 0;
            if ((rc = be_conv_nhwc_f32(&d, x, L.w(packed, b.ds, DS_F32), packed + L.r[L.zero].b_off, nullptr, r, c, stream))) return rc;
        }
    }
    return be::wino_pair(x, u1, b1, 1, u2, b2, r, 1, o, n, cin, c, c, w, w_floats, stream, pool2, x_in_v, next_cmid);
}

// x != nullptr: flat patches [n,3,21,21]; else the patches are gathered from `view` (image pair, f2)
int forward_impl(const float* packed, const float* x, const be_patch_view* view, int64_t P, float* out, int64_t n,
                 void* workspace, size_t workspace_bytes, const be_local_stage_opts* opts, void* stream, const char* who) {
    BE_REQUIRE(n >= 0, "%s: n < 0", who);
    BE_REQUIRE(!opts || opts->chunk >= 0, "%s: opts->chunk < 0", who);
    const int g_wino = opts ? (opts->winograd != 0) : 1;
    const int g_chunk = chunk_of(opts ? opts->chunk : 0);
    if (n == 0) return BE_OK;
    BE_REQUIRE(packed && (x || view) && out && workspace, "%s: null pointer", who);
    BE_REQUIRE(be::aligned16(workspace) && be::aligned16(packed), "%s: workspace / packed must be 16-byte aligned", who);
    if (workspace_bytes < be_local_stage_workspace_bytes(n, g_chunk))
        return be::fail(BE_EWORKSPACE, "%s: workspace %zu B < %zu B needed", who, workspace_bytes,
                        be_local_stage_workspace_bytes(n, g_chunk));
    const Layout& L = layout();
    const float *w0 = L.w(packed, 0, F32), *b0 = L.b(packed, 0, F32);
    for (int64_t first = 0; first < n; first += g_chunk) {
        const int nb = (int)((n - first) < g_chunk ? (n - first) : g_chunk);
        const Route r = route_of(knobs(), g_wino, nb);
        const Carved c = carve(static_cast<float*>(workspace), nb, g_wino != 0);
        int rc;
        if (r.staging == STAGE_NHWC4P)
            rc = x ? be_nchw3_to_nhwc4p_f32(x + first * 3 * BE_NPIX, c.x4, nb, BE_R, BE_R, 28, stream)
                   : be_view_to_nhwc4p_f32(view, P, first, c.x4, nb, 28, stream);
        else
            rc = x ? be_nchw3_to_nhwc4_f32(x + first * 3 * BE_NPIX, c.x4, nb, BE_NPIX, stream) : be_view_to_nhwc4_f32(view, P, first, c.x4, nb, stream);
        if (rc) return rc;
        switch (r.conv1) {
        case C1_POOL_BF6: rc = be_conv7x7_pool_bf6_nhwc4p_f32(c.x4, nb, w0, b0, c.p1, stream); break;
        // conv1 + Smish + the first max-pool in one image-major launch (be_conv1_pool.hip)
        case C1_POOL: rc = be_conv7x7_pool_nhwc4p_f32(c.x4, nb, w0, b0, c.p1, stream); break;
        case C1_PM: {
            be_conv_desc d;
            d.n = nb; d.h = 21; d.w = 21; d.cin = 4; d.cout = 64; d.ksize = 7; d.act = 1;
            rc = be_conv7x7_nhwc4p_f32(&d, c.x4, 28, w0, b0, c.c1, 64, stream);
            break;
        }
        default: rc = conv(L, packed, 0, c.x4, nullptr, c.c1, nb, 21, 1, 64, stream);
        }
        if (rc) return rc;
        if (!r.conv1_pools && (rc = be_maxpool_nhwc_f32(c.c1, c.p1, nb, 21, 21, 64, 3, 2, 1, stream))) return rc;
        if ((rc = r.l0_bf6 ? block_l0_bf6(L, packed, c.in[0], c.t[0], c.out[0], nb, stream)
                           : block(L, packed, kBlocks[0], c.in[0], c.t[0], c.out[0], nb, stream))) return rc;
        // Chained (the Winograd path, at every sub-batch size): the blocks are linked through the start of RW.  The pool leaves
        // layer1's input transform there, layers 1 and 2 end in the kernel that also writes the next layer's, so no block reads its
        // input map a second time.  Lifetimes in RW: a block's V and M are dead once its last GEMMs ran, except M, which the boundary
        // kernel reads while it writes the next V below M's start.  With the downsamples folded into conv2's GEMMs x's transform
        // stays alive beside conv1's (three regions) and nothing reads the maps themselves (!store_maps); under BE_WINO_DS_GEMM=1
        // the 1x1 downsample launch reads them, and they are written.
        if (r.chain) rc = be::pool_wino_in(c.out[0], r.store_maps ? c.p2 : nullptr, nb, 96, kLayers[kBlocks[1].conv1].cout, c.wino, c.wino_floats, stream);
        else rc = be_maxpool_nhwc_f32(c.out[0], c.p2, nb, 11, 11, 96, 3, 2, 1, stream);
        if (rc) return rc;
        for (int k = 1; k < 4; ++k) {                     // layer3's Winograd block writes p3 itself (pool2)
            if (r.blocks6 == B6_DIRECT) rc = block(L, packed, kBlocks[k], c.in[k], c.t[k], c.out[k], nb, stream);
            else rc = block_wino(L, packed, r, kBlocks[k], c.in[k], k == 3 ? c.p3 : c.out[k], c.ds, c.wino, c.wino_floats, nb, stream, k == 3,
                                 r.chain && k < 3 ? kLayers[kBlocks[k + 1].conv1].cout : 0);
            if (rc) return rc;
        }
        if (r.blocks6 == B6_DIRECT && (rc = be_maxpool_nhwc_f32(c.out[3], c.p3, nb, 6, 6, 256, 2, 2, 0, stream))) return rc;
        // fc.1 (+ BN1d + Smish), fc.4
        if (r.fc1_bf6) rc = be::gemm_rows_bf6(c.p3, nb, 2304, L.w(packed, 13, ROWS_BF6), 1024, L.b(packed, 13, F32), nullptr, 1, c.f1, 1024, stream);
        else rc = conv(L, packed, 13, c.p3, nullptr, c.f1, nb, 1, 1, 1024, stream);
        if (rc) return rc;
        if ((rc = conv(L, packed, 14, c.f1, nullptr, out + first * BE_LOCAL_OUT, nb, 1, 0, BE_LOCAL_OUT, stream))) return rc;
    }
    return BE_OK;
}

}  // namespace

extern "C" int be_local_stage_forward_f32(const float* packed, const float* x, float* out, int64_t n,
                                          void* workspace, size_t workspace_bytes, const be_local_stage_opts* opts, void* stream) {
    BE_REQUIRE(x || n == 0, "be_local_stage_forward_f32: null pointer");
    return forward_impl(packed, x, nullptr, 1, out, n, workspace, workspace_bytes, opts, stream, "be_local_stage_forward_f32");
}

extern "C" int be_local_stage_forward_view_f32(const float* packed, const be_patch_view* view, int64_t patches_per_image,
                                               float* out, int64_t n, void* workspace, size_t workspace_bytes,
                                               const be_local_stage_opts* opts, void* stream) {
    BE_REQUIRE((view && view->base && view->wp > 0 && patches_per_image > 0) || n == 0,
               "be_local_stage_forward_view_f32: bad view");
    return forward_impl(packed, nullptr, view, patches_per_image, out, n, workspace, workspace_bytes, opts, stream,
                        "be_local_stage_forward_view_f32");
}

// HOST-ONLY inspection hooks (no device): the region table and a sub-batch's route, as the pack and the forward use them
extern "C" int be_local_stage_layout_debug(int* layer_form_reads, int64_t* w_b_off_n, int cap) {
    const Layout& L = layout();
    BE_REQUIRE(layer_form_reads && w_b_off_n && cap >= L.n, "be_local_stage_layout_debug: room for %d regions needed", L.n);
    for (int k = 0; k < L.n; ++k) {
        const Region& r = L.r[k];
        const int a[3] = {r.layer, r.form, r.reads};
        const size_t o[4] = {r.w_off, r.w_n, r.b_off, r.b_n};
        for (int j = 0; j < 3; ++j) layer_form_reads[3 * k + j] = a[j];
        for (int j = 0; j < 4; ++j) w_b_off_n[4 * k + j] = (int64_t)o[j];
    }
    return L.n;
}

extern "C" int be_local_stage_route_debug(int winograd, int nb, int* out) {
    BE_REQUIRE(out && nb >= 1, "be_local_stage_route_debug: bad arguments");
    const Route r = route_of(knobs(), winograd, nb);
    const int a[kRouteFields] = {r.staging, r.conv1, r.conv1_pools, r.l0_bf6, r.chain, r.blocks6, r.store_maps, r.fc1_bf6};
    for (int j = 0; j < kRouteFields; ++j) out[j] = a[j];
    return kRouteFields;
}
