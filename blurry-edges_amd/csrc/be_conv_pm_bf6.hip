// Pixel-major 3x3 convolution (optionally with a fused 1x1 on x2) for Cout <= 96 in split-bf16 arithmetic (gfx950): LocalStage's
// layer0 wherever the Winograd path runs.
//
// k_conv_pm<., ., PM_TAPS3>'s tile and K walk (be_conv_pm.hip) around k_wino_gemm_ps's loop (be_wino.hip):
//   - one output pixel of BM = 128 consecutive images per workgroup, so the list of taps inside the image is wave-uniform: taps
//     outside are skipped for the whole tile, nothing is zero-filled; interior pixels first, the border ring last; a group's pixel
//     tiles stay on one XCD; the K walk (32-channel chunk, valid tap, 16-float half), then the 16-float chunks of the 1x1 on x2, is
//     scalar arithmetic; A goes global -> LDS by global_load_lds_dwordx4 in 1-KB pieces with the quads XOR-swizzled; rows past
//     the batch load a valid row and are never stored;
//   - A stays fp32 in HBM and LDS and is split after the fragment read (split8); B's hi / mid / lo planes are read ready-made
//     from the 12-KB blocks of be_gemm_rows_bf6_pack_f32 applied to the packed fp32 matrix [96][Ktot] (whose K order is the
//     walk's order: chunk = (cc * 9 + tap) * 2 + half, the 1x1 behind ncc * 9 * 2); six v_mfma_f32_32x32x16_bf16 per 16-deep
//     chunk in the fixed order lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi, fp32 accumulation, K ascending from a zero
//     accumulator; counted vmcnt waits and one raw s_barrier per chunk; the next chunk's fragments are read and split between
//     the current chunk's MFMAs.
// Wave tile 32 images x 96 channels (all MFMAs useful: three 32-column accumulators, one A fragment): per chunk a wave issues
// 18 MFMAs for 2 + 9 fragment reads, one split8 and its DMA pieces - the SAME pieces in the tap segment and in the x2 segment,
// which is what the counted waits rely on.  Past the end of the walk the last chunk is fetched again (into slots nobody reads any
// more), so the counts never change; the last wait drains everything: no DMA into LDS outlives the workgroup.
// The LDS ring (no result bit depends on it): three 8-KB A slots and two 9-KB B slots, 42 KB: three workgroups per CU.  The two
// register sets free the slot of chunk c a chunk before its MFMAs, so a ring of N slots gives a lead of N - 1 chunks: A (from HBM,
// or L2 behind a sibling tile) keeps a lead of two chunk times, B (0.4-0.7 MB of planes shared by every tile: L2 hits) gets one.
// A B slot holds the 9 real pieces only - rows 96-127 of each plane, one 1-KB piece in four, are padding that no fragment read
// touches and are not fetched.  Per chunk the 8 A pieces go two to a wave and the 9 B pieces 3 / 2 / 2 / 2 (wave 0 takes the odd
// one); at the top of chunk c a wave issues B(c + 2), then A(c + 3), and the wait at the top of c + 1 is "vmcnt(2)": all but the
// two A pieces just issued - the same count for every wave.  The invariant is written out at the prologue below.
// The pieces live in two register sets; the next chunk's reads and split sit between this chunk's MFMAs, every gap closed by
// __builtin_amdgcn_sched_barrier(0) (L0_CHUNK; k_wino_gemm_ps's scheme and the reasons for it: be_wino.hip).  No result bit depends
// on it.  The emitted loop (hipcc -S, gfx950, read by hand; hipcc rotates the loop into four bodies, all alike):
//   top         vmcnt(2) lgkmcnt(0), s_barrier, 2 global_load_lds_dwordx4 of B (a third behind a branch on the wave), the walker's
//               scalar arithmetic, 2 global_load_lds_dwordx4 of A
//   gaps 0-4    MFMA, 2 ds_read_b128 each;  gap 5  MFMA, 1 ds_read_b128;  gaps 6-9  MFMA alone
//   gap 10      MFMA, s_waitcnt lgkmcnt(0) (the youngest read is four MFMAs old), half A: 6 VALU + 1 s_nop
//   gaps 11-17  MFMA, half B (5 VALU + s_nop) and half A (6 VALU + s_nop) in turn
//   consecutive MFMAs write different accumulators (v[32:47] v[16:31] v[0:15] in turn); no v_pk_* f32 instruction, no scratch.
// Compiler report (gfx950): 164 VGPRs (168 allocated: three waves per SIMD), 0 AGPRs, scratch 0, no VGPR or SGPR spills; LDS 42 KB:
// three workgroups per CU.
// One body for every batch size: an output element sees the same chain of operations whatever the batch, the position in it or
// the tile it falls in.
#include "be_common.h"
#include "be_device_math.h"
#include "be_split_bf16.h"
#include <cstdlib>

namespace {

using be::bf6::bf16x8;
using be::bf6::f32x4;
using be::bf6::split8;
using be::bf6::u32x4;
using be::bf6::PS_BLOCK;
using be::bf6::ps_slot;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

constexpr int L0_BM = 128, L0_BKT = 16;
constexpr int L0_ABYTES = L0_BM * L0_BKT * 4, L0_BBYTES = PS_BLOCK * 2;      // an A slot: 8 KB; a chunk's block of planes in HBM: 12 KB
// the ring: three A slots, then two B slots of the 9 real pieces - rows 0-95 of each plane, 3 KB a plane
constexpr int L0_ASLOTS = 3, L0_BSLOTS = 2, L0_BPLANE3 = 96 * 32, L0_BBYTES3 = 3 * L0_BPLANE3;
constexpr int L0_LDS3 = L0_ASLOTS * L0_ABYTES + L0_BSLOTS * L0_BBYTES3;      // 42 KB

struct PmBf6Args {
    const float* x;       // NHWC [N,H,W,Cin]
    const float* x2;      // optional second input [N,H,W,Cin2]: its 1x1 conv is appended to the K loop
    const float* planes;  // hi / mid / lo blocks of the packed [96][Ktot] matrix, one 12-KB block per 16-deep chunk
    const float* bias;
    float* y;             // NHWC [N,H,W,ldy]
    int Nimg, H, W, HW, Cin, Cin2, Cout, ldy, act, groups, ncc;
    int64_t istride, istride2;      // floats per image in x / x2
};

__global__ __launch_bounds__(256, 3)
void k_conv_pm_bf6(PmBf6Args a) {
    constexpr int BM = L0_BM, BKT = L0_BKT, ABYTES = L0_ABYTES, BBYTES = L0_BBYTES;
    constexpr int BBASE3 = L0_ASLOTS * ABYTES, BBYTES3 = L0_BBYTES3, BPLANE = L0_BPLANE3;
    extern __shared__ __attribute__((aligned(16))) float smem_l0[];
    char* const lds = reinterpret_cast<char*>(smem_l0);

    // ---- workgroup -> (group of BM images, pixel): a group's pixel tiles stay on one XCD (shared input lines)
    const int bid = blockIdx.x;
    const int xcd = bid & 7, t = bid >> 3;
    const int grp = (t / a.HW) * 8 + xcd;
    if (grp >= a.groups) return;
    const int img0 = grp * BM;
    int py, px;
    {   // interior pixels (all taps) first, the border ring (fewer taps) last: the short tiles fill the tail
        const int idx = t % a.HW, ni = (a.H - 2) * (a.W - 2);
        if (idx < ni) { py = 1 + idx / (a.W - 2); px = 1 + idx % (a.W - 2); }
        else {
            const int e = idx - ni;
            if (e < a.W) { py = 0; px = e; }
            else if (e < 2 * a.W) { py = a.H - 1; px = e - a.W; }
            else if (e < 2 * a.W + a.H - 2) { px = 0; py = 1 + e - 2 * a.W; }
            else { px = a.W - 1; py = 1 + e - 2 * a.W - (a.H - 2); }
        }
    }
    // taps of the 3x3 kernel this pixel has inside the image, 4 bits each
    unsigned long long tap_list = 0;
    int ntap = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const bool ok = (unsigned)(py + k / 3 - 1) < (unsigned)a.H && (unsigned)(px + k % 3 - 1) < (unsigned)a.W;
        if (ok) { tap_list |= (unsigned long long)k << (4 * ntap); ++ntap; }
    }

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    float bias_v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int c = j * 32 + li;
        bias_v[j] = (c < a.Cout && a.bias) ? a.bias[c] : 0.0f;
    }
    // ---- A staging: wave w fills pieces 2w, 2w+1 of the tile; lane -> (row lane >> 2 of the piece, the quad the swizzle puts there)
    const int srow = lane >> 2, sq = (lane & 3) ^ ((lane >> 4) & 3);
    unsigned a_off[2], a_off2[2];                      // byte offsets from the tile's first row
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = (2 * wave + p) * 16 + srow;
        const int rr = img0 + r < a.Nimg ? r : 0;      // images past the batch: a valid image (never stored)
        a_off[p] = (unsigned)(rr * a.istride + 4 * sq) * 4u;
        a_off2[p] = (unsigned)(rr * a.istride2 + 4 * sq) * 4u;
    }
    const float* xpix = a.x + (int64_t)img0 * a.istride + (py * a.W + px) * a.Cin;
    const float* x2pix = a.x2 ? a.x2 + (int64_t)img0 * a.istride2 + (py * a.W + px) * a.Cin2 : nullptr;
    // B: 1-KB pieces of the chunk's 12-KB block, whose rows 0-95 of each plane are already the LDS image (lane-linear: this lane's 16 B)
    const char* wt = reinterpret_cast<const char*>(a.planes) + lane * 16;

    // ---- K walk: main part (cc, valid tap j, half), then the 1x1 on x2 (16-float chunks)
    const int n_main = a.ncc * ntap * 2;
    const int total = n_main + (a.x2 ? a.Cin2 / BKT : 0);
    int w_cc = 0, w_j = 0, w_sub = 0, w_k = 0;         // walker state of the next chunk to load
    // A and B are fetched apart - B(c + 2), then A(c + 3).  The walker belongs to A; B's block is the walker's chunk one A
    // fetch ago (b_chunk).  A: pieces 2w, 2w+1 as above.  B: the 9 real pieces b = 3 plane + (32-row piece) dealt b = w, w + 4 and
    // b = 8 to wave 0 - 3 pieces for wave 0, 2 for the others; piece b is piece 4 (b / 3) + b % 3 of the block (every fourth is the
    // padding rows 96-127, which no fragment read touches: not fetched).
    int b_chunk = 0, l_a = 0, l_b = 0;                 // ... and the ring slots the next A and B fetches fill
#define L0_DMA_A()                                                                                              \
    do {                                                                                                        \
        char* st_ = lds + l_a * ABYTES;                                                                         \
        const char* xs_;                                                                                        \
        unsigned o0_, o1_;                                                                                      \
        if (w_k < n_main) {                                                                                     \
            const int tap_ = (int)((tap_list >> (4 * w_j)) & 15ull);                                            \
            const int ty_ = (tap_ * 11) >> 5, tx_ = tap_ - 3 * ty_;                    /* tap / 3, tap % 3 */     \
            xs_ = reinterpret_cast<const char*>(xpix + ((ty_ - 1) * a.W + tx_ - 1) * a.Cin + w_cc * 32 + w_sub * BKT); \
            b_chunk = (w_cc * 9 + tap_) * 2 + w_sub;                                                            \
            o0_ = a_off[0]; o1_ = a_off[1];                                                                     \
        } else {                                                                                                \
            const int k2_ = w_k - n_main;                                                                       \
            xs_ = reinterpret_cast<const char*>(x2pix + k2_ * BKT);                                             \
            b_chunk = a.ncc * 18 + k2_;                                                                         \
            o0_ = a_off2[0]; o1_ = a_off2[1];                                                                   \
        }                                                                                                       \
        __builtin_amdgcn_global_load_lds((glb_ptr_t)(xs_ + o0_), (lds_ptr_t)(st_ + (2 * wave) * 1024), 16, 0, 0);     \
        __builtin_amdgcn_global_load_lds((glb_ptr_t)(xs_ + o1_), (lds_ptr_t)(st_ + (2 * wave + 1) * 1024), 16, 0, 0); \
        if (w_k + 1 < total) {                         /* past the end: the last chunk again */                  \
            ++w_k;                                                                                              \
            if (++w_sub == 2) { w_sub = 0; if (++w_j == ntap) { w_j = 0; ++w_cc; } }                            \
        }                                                                                                       \
        l_a = l_a == L0_ASLOTS - 1 ? 0 : l_a + 1;                                                               \
    } while (0)
#define L0_DMA_B()                                                                                              \
    do {                                                                                                        \
        const char* ws_ = wt + (int64_t)b_chunk * BBYTES;                                                       \
        char* st_ = lds + BBASE3 + l_b * BBYTES3;                                                               \
        _Pragma("unroll") for (int p_ = 0; p_ < 2; ++p_) {                                                      \
            const int b_ = wave + 4 * p_;                                                                       \
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(ws_ + (4 * (b_ / 3) + b_ % 3) * 1024), (lds_ptr_t)(st_ + b_ * 1024), 16, 0, 0); \
        }                                                                                                       \
        if (wave == 0)                                                                                          \
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(ws_ + 10 * 1024), (lds_ptr_t)(st_ + 8 * 1024), 16, 0, 0); \
        l_b ^= 1;                                                                                               \
    } while (0)

    // ---- fragment reads: A row 32 wave + li, quads 2 lh, 2 lh + 1 (swizzled as stored); B plane p, row 32 j + li, half lh
    const int fsw = (li >> 2) & 3;
    const int a_fr0 = ((wave * 32 + li) * BKT + 4 * ((2 * lh) ^ fsw)) * 4;
    const int a_fr1 = ((wave * 32 + li) * BKT + 4 * ((2 * lh + 1) ^ fsw)) * 4;
    const int b_fr = li * 32 + ps_slot(li, lh) * 16;
    f32x16 acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    // two sets of pieces: chunk c's MFMAs read set c & 1 while chunk c + 1's fragments are read and split into the other set, one
    // piece of that work in every gap between two MFMAs (L0_CHUNK, k_wino_gemm_ps's scheme).  The set is a compile-time parameter
    // of the body (a run-time index would send the pieces to scratch): the loop walks two chunks per trip, an odd total ends
    // behind body 0.
    u32x4 ap[2][3];                                    // [set][hi, mid, lo], one dword per pair unit
    bf16x8 bp[2][3][3];                                // [set][hi, mid, lo][j]
    int r_buf = 0, r_b = 0;                            // the A slot and the B slot whose fragments are read next
    // One chunk: 18 groups, each closed by a sched_barrier(0) (nothing crosses it, so the order below is the emitted order).
    // Group g issues MFMA g - product p = g / 3 (lo.hi hi.lo mid.mid mid.hi hi.mid hi.hi), accumulator j = g % 3: consecutive
    // MFMAs never share an accumulator - and, for chunk + 1 out of ring slot r_buf into set S ^ 1:
    //   g = 0       the two fp32 A fragment reads (quads 2 lh, 2 lh + 1)
    //   g = 1..5    two B reads each (the last gap one), planes hi, mid, lo in turn
    //   g = 10..17  one half of one of the four pair units of the split8 (unit u = (g - 10) / 2; half A, then half B)
    // The LDS reads are plain loads and the compiler places their wait, a full lgkmcnt(0) in front of the first split group, where
    // the youngest read is four MFMAs old.
#define L0_CHUNK(S)                                                                                             \
    do {                                                                                                        \
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};                                   \
        const char* sb_ = lds + r_buf * ABYTES;                                                                 \
        const char* sw_ = lds + BBASE3 + r_b * BBYTES3;                                                         \
        f32x4 af_[2];                                  /* [quad] */                                             \
        float r0_[4], r1_[4];                                                                                   \
        _Pragma("unroll") for (int g_ = 0; g_ < 18; ++g_) {                                                     \
            acc[g_ % 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ap[S][PA[g_ / 3]]),\
                                                                  bp[S][PB[g_ / 3]][g_ % 3], acc[g_ % 3], 0, 0, 0); \
            if (g_ == 0) {                                                                                      \
                af_[0] = *reinterpret_cast<const f32x4*>(sb_ + a_fr0);                                          \
                af_[1] = *reinterpret_cast<const f32x4*>(sb_ + a_fr1);                                          \
            }                                                                                                   \
            if (g_ >= 1 && g_ < 6)                                                                              \
                _Pragma("unroll") for (int b_ = 2 * (g_ - 1); b_ < 2 * g_ && b_ < 9; ++b_)                      \
                    bp[(S) ^ 1][b_ / 3][b_ % 3] =                                                               \
                        *reinterpret_cast<const bf16x8*>(sw_ + b_fr + (b_ / 3) * BPLANE + (b_ % 3) * 32 * 32);  \
            if (g_ >= 10) {                                                                                     \
                const int u_ = (g_ - 10) >> 1;                                                                  \
                if ((g_ & 1) == 0) {                                                                            \
                    unsigned h_, m_;                                                                            \
                    be::bf6::split_pair_a(af_[u_ >> 1][(2 * u_) & 3], af_[u_ >> 1][(2 * u_ + 1) & 3], h_, m_, r0_[u_], r1_[u_]); \
                    ap[(S) ^ 1][0][u_] = h_;                                                                    \
                    ap[(S) ^ 1][1][u_] = m_;                                                                    \
                } else {                                                                                        \
                    unsigned l_ = be::bf6::split_pair_b(r0_[u_], r1_[u_], ap[(S) ^ 1][1][u_]);                  \
                    asm volatile("" : "+v"(l_));       /* (keeps the last cvt_pk in its group) */               \
                    ap[(S) ^ 1][2][u_] = l_;                                                                    \
                }                                                                                               \
            }                                                                                                   \
            __builtin_amdgcn_sched_barrier(0);                                                                  \
        }                                                                                                       \
        r_buf = r_buf == L0_ASLOTS - 1 ? 0 : r_buf + 1;                                                         \
        r_b ^= 1;                                                                                               \
    } while (0)

    __builtin_amdgcn_sched_barrier(0);                 // (the bias loads are older than every DMA: no count below depends on them)
    // The ring invariant.  A wave's DMA pieces in issue order (nB = 3 for wave 0, 2 for the others; nA = 2):
    //   A(0) B(0) A(1) B(1) A(2) | B(2) A(3) | B(3) A(4) | ... : the prologue, then "B(c + 2) A(c + 3)" at the top of chunk c.
    // vmcnt counts a wave's own pieces, oldest first, so "vmcnt(2)" = all but the A pieces just issued have landed:
    //   here           in flight A(2);      landed: chunks 0 and 1
    //   top of c + 1   in flight A(c + 3);  landed: B(c + 2), A(c + 2) and everything older - chunk c + 2, whose fragments
    //                  are read during chunk c + 1.  Nothing less would do: B(c + 2) is the youngest piece that must be in LDS.
    // Slots: A(c + 3) goes to A slot c % 3 and B(c + 2) to B slot c % 2, the slots of chunk c, whose fragments every wave read
    // during chunk c - 1 (two register sets) and holds in registers before it passes the barrier at the top of c (lgkmcnt(0)
    // there).  Chunk c + 1, read during chunk c, sits in A slot (c + 1) % 3 and B slot (c + 1) % 2: neither is written then.
    L0_DMA_A(); L0_DMA_B();                            // chunk 0
    L0_DMA_A(); L0_DMA_B();                            // chunk 1
    L0_DMA_A();                                        // A of chunk 2
    __builtin_amdgcn_s_waitcnt(0x0F72);                // vmcnt(2): chunks 0 and 1 have landed
    __builtin_amdgcn_s_barrier();                      // ... every wave's
    {                                                  // chunk 0's pieces into set 0, in one piece
        const f32x4 af0_ = *reinterpret_cast<const f32x4*>(lds + a_fr0);
        const f32x4 af1_ = *reinterpret_cast<const f32x4*>(lds + a_fr1);
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                bp[0][p][j] = *reinterpret_cast<const bf16x8*>(lds + BBASE3 + b_fr + p * BPLANE + j * 32 * 32);
        bf16x8 h, m, l;
        split8(af0_, af1_, h, m, l);
        ap[0][0] = __builtin_bit_cast(u32x4, h);
        ap[0][1] = __builtin_bit_cast(u32x4, m);
        ap[0][2] = __builtin_bit_cast(u32x4, l);
        r_buf = 1;
        r_b = 1;
    }
    bool landed = true;                                // the NEXT chunk's DMA is known to be in LDS
#define L0_TOP()                                                                                                \
    do {                                                                                                        \
        if (!landed) __builtin_amdgcn_s_waitcnt(0x0072);   /* vmcnt(2): all but A(chunk + 2): chunk + 1 has landed; lgkmcnt(0) */ \
        else __builtin_amdgcn_s_waitcnt(0xC07F);           /* lgkmcnt(0): this chunk's fragments are in registers */ \
        landed = false;                                                                                         \
        __builtin_amdgcn_s_barrier();                  /* ... every wave's; everyone holds this chunk's fragments */ \
        L0_DMA_B();                                    /* B of chunk + 2, into this chunk's B slot */           \
        L0_DMA_A();                                    /* A of chunk + 3, into this chunk's A slot */           \
        __builtin_amdgcn_sched_barrier(0);                                                                      \
    } while (0)
    for (int kc = 0; kc < total; kc += 2) {
        L0_TOP();
        L0_CHUNK(0);                                   // this chunk's MFMAs with chunk + 1's reads and split in their gaps
        __builtin_amdgcn_sched_barrier(0);
        if (kc + 1 < total) {
            L0_TOP();
            L0_CHUNK(1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef L0_TOP
#undef L0_DMA_A
#undef L0_DMA_B
#undef L0_CHUNK
    __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0): nothing left in flight into LDS
    __builtin_amdgcn_sched_barrier(0);

    // ---- epilogue: D[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); row = image of the group
    const int64_t rs = (int64_t)a.HW * a.ldy;          // floats between the same pixel of consecutive images
    char* yt = reinterpret_cast<char*>(a.y + ((int64_t)img0 * a.HW + py * a.W + px) * a.ldy);                 // uniform
    const unsigned y_off = (unsigned)((wave * 32 + 4 * lh) * rs + li) * 4u;
    const bool interior = img0 + BM <= a.Nimg && a.Cout == 96;
#define L0_STORE(J)                                                                                             \
    do {                                                                                                        \
        float v_ = acc[J][r] + bias_v[J];                                                                       \
        if (a.act == 1) v_ = be::smish(v_); else if (a.act == 2) v_ = fmaxf(v_, 0.0f);                          \
        reinterpret_cast<float*>(yt + (size_t)ro * rs * 4 + y_off)[(J) * 32] = v_;                              \
    } while (0)
    if (interior) {                                    // no per-element bounds checks
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ro = (r & 3) + 8 * (r >> 2);
#pragma unroll
            for (int j = 0; j < 3; ++j) L0_STORE(j);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const bool c_ok = j * 32 + li < a.Cout;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = (r & 3) + 8 * (r >> 2);
                if (c_ok && img0 + wave * 32 + 4 * lh + ro < a.Nimg) L0_STORE(j);
            }
        }
    }
#undef L0_STORE
}

inline int ktot_of(int cin, int cin2) { return 9 * cin + cin2; }
inline bool shape_ok(int cout, int cin, int cin2) {
    return cout > 0 && (cout + 31) / 32 * 32 == 96 && cin > 0 && cin % 32 == 0 && cin2 >= 0 && cin2 % 16 == 0;
}

}  // namespace

bool be::l0_bf6_enabled() {
    // A/B knobs: BE_L0_F32=1 sends only layer0 back to the fp32 kernels; BE_WINO_F32=1 restores fp32 everywhere
    static const bool f32 = be::knob_on("BE_L0_F32") || be::knob_on("BE_WINO_F32");
    return !f32;
}

extern "C" size_t be_conv3x3_pm_bf6_packed_floats(int cout, int cin, int cin2) {
    if (!shape_ok(cout, cin, cin2)) return 0;
    return be_gemm_rows_bf6_packed_floats(cout, ktot_of(cin, cin2));
}

extern "C" int be_conv3x3_pm_bf6_pack_f32(const float* packed_w, int cout, int cin, int cin2, float* planes, void* stream) {
    BE_REQUIRE(packed_w && planes, "be_conv3x3_pm_bf6_pack_f32: null pointer");
    BE_REQUIRE(shape_ok(cout, cin, cin2),
               "be_conv3x3_pm_bf6_pack_f32: unsupported shape (cout %d: cout_pad32 must be 96; cin %d %% 32; cin2 %d %% 16)", cout, cin, cin2);
    return be_gemm_rows_bf6_pack_f32(packed_w, cout, ktot_of(cin, cin2), planes, stream);
}

int be::conv3x3_pm_bf6(const be_conv_desc* d, const float* x, const float* x2, int cin2, const float* planes, const float* bias,
                       float* y, int ldy, void* stream) {
    BE_REQUIRE(d && x && planes && y, "be_conv3x3_pm_bf6_f32: null pointer");
    BE_REQUIRE(d->ksize == 3 && d->n >= 0 && (unsigned)d->act <= 2u, "be_conv3x3_pm_bf6_f32: bad descriptor (ksize %d, n %d, act %d)",
               d->ksize, d->n, d->act);
    BE_REQUIRE(x2 || cin2 == 0, "be_conv3x3_pm_bf6_f32: cin2 %d without x2", cin2);
    BE_REQUIRE(shape_ok(d->cout, d->cin, cin2) && (!x2 || cin2 > 0),
               "be_conv3x3_pm_bf6_f32: unsupported shape (cout %d: cout_pad32 must be 96; cin %d %% 32; cin2 %d %% 16)", d->cout, d->cin, cin2);
    BE_REQUIRE(d->h >= 3 && d->w >= 3 && ldy >= d->cout, "be_conv3x3_pm_bf6_f32: unsupported map (h %d, w %d >= 3; ldy %d >= cout)",
               d->h, d->w, ldy);
    BE_REQUIRE(be::aligned16(x) && be::aligned16(x2) && be::aligned16(planes) && (reinterpret_cast<uintptr_t>(y) & 3u) == 0 &&
               (!bias || (reinterpret_cast<uintptr_t>(bias) & 3u) == 0),
               "be_conv3x3_pm_bf6_f32: x / x2 / planes must be 16-byte aligned, y / bias 4-byte");
    if (d->n == 0) return BE_OK;
    PmBf6Args a;
    a.x = x; a.x2 = x2; a.planes = planes; a.bias = bias; a.y = y;
    a.Nimg = d->n; a.H = d->h; a.W = d->w; a.HW = d->h * d->w; a.Cin = d->cin; a.Cin2 = x2 ? cin2 : 0; a.Cout = d->cout; a.ldy = ldy;
    a.act = d->act; a.ncc = d->cin / 32;
    a.istride = (int64_t)a.HW * d->cin;
    a.istride2 = (int64_t)a.HW * a.Cin2;
    // 32-bit lane offsets: 256 images of input / output must span < 2^32 bytes
    const int64_t span = 256 * 4 * (a.istride > a.istride2 ? a.istride : a.istride2);
    BE_REQUIRE(span < ((int64_t)1 << 32) && 256 * 4 * (int64_t)a.HW * ldy < ((int64_t)1 << 32),
               "be_conv3x3_pm_bf6_f32: 256 images must span < 2^32 bytes");
    a.groups = (d->n + L0_BM - 1) / L0_BM;
    const int64_t grid = (int64_t)8 * ((a.groups + 7) / 8) * a.HW;
    BE_REQUIRE(grid < ((int64_t)1 << 31), "be_conv3x3_pm_bf6_f32: too many tiles (n %d, %d x %d)", d->n, d->h, d->w);
    hipStream_t s = be::as_stream(stream);
    const size_t lds = L0_LDS3;
    static be::DeviceFlags attr_set{};                      // dynamic-LDS cap raised once per device (thread-safe)
    if (int rc_ = be::ensure_dynamic_lds(reinterpret_cast<const void*>(&k_conv_pm_bf6), lds, attr_set)) return rc_;
    {   // algorithmic work: 2*M*K*Cout with the real K, in fp32-equivalent products; executed: the chunks the tiles visit x 2*BM*96*16
        const double M = (double)a.Nimg * a.HW, k_real = 9.0 * a.Cin, k2 = (double)a.Cin2;
        double chunks = 0.0;
        for (int py = 0; py < a.H; ++py)
            for (int px = 0; px < a.W; ++px) {
                int nt = 0;
                for (int k = 0; k < 9; ++k) nt += (unsigned)(py + k / 3 - 1) < (unsigned)a.H && (unsigned)(px + k % 3 - 1) < (unsigned)a.W;
                chunks += 2.0 * nt * a.ncc + a.Cin2 / 16;
            }
        chunks *= (double)a.groups;
        be::ProfileScope prof(s, BE_KERNEL_CONV_128x96, 2.0 * M * (k_real + k2) * a.Cout,
                              4.0 * (M * (a.Cin + k2) + M * a.Cout) + 6.0 * (k_real + k2) * 128,
                              chunks * 2.0 * L0_BM * 96 * 16);
        hipLaunchKernelGGL(k_conv_pm_bf6, dim3((unsigned)grid), dim3(256), lds, s, a);
    }
    return be::check_launch("be_conv3x3_pm_bf6_f32");
}

extern "C" int be_conv3x3_pm_bf6_f32(const be_conv_desc* desc_host, const float* x, const float* x2, int cin2, const float* planes,
                                     const float* packed_bias, float* y, int ldy, void* stream) {
    return be::conv3x3_pm_bf6(desc_host, x, x2, cin2, planes, packed_bias, y, ldy, stream);
}
