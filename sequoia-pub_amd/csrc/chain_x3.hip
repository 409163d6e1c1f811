// Split-mode ("x3") chain of the 56 x 56 stage: one launch does, for a tile of 64 consecutive pixels,
//     y   = relu(t2 . w3^T * s3 + b3 + identity)          src/resnet.py:83-91   (conv3 / bn3, += identity, relu)
//     t1' = relu(y . w1'^T * s1' + b1')                   src/resnet.py:75-77 of the NEXT block (conv1 / bn1 / relu)
// on hi / lo planes of 16-bit values (x3_fmt.h), three MFMAs per product.
//
// Why: in the split modes an activation costs 4 bytes per element, and the 56 x 56 stage's 1x1 convolutions run at what
// the fabric gives (4.2 - 4.4 TB/s): unfused, y (1 KB per pixel) is written by the expand and read back
// by the next block's reduce.  Here the reduce is fed from LDS: per pixel t2 (256 B) and the identity (1 KB) are read, y
// (1 KB) and t1' (256 / 512 B) written -- 2.5 KB instead of 3.75 KB, and two launches become one.
//
// Tile = 64 pixels x all 256 channels, 4 waves, 80 KiB of LDS, TWO blocks per CU (one block's memory phases run under the
// other's matrix phases).  All weights are read from fragment-ordered copies that a pack kernel writes in front of the
// launch (bottom of this file): every wave-wide weight request is one contiguous 1 KiB.
//   1. both 32-deep K-tiles of t2 (8 KiB) arrive by LDS-DMA; the B fragments of w3 (no other wave reads a wave's 64 rows)
//      go straight from L2 into registers; wave w multiplies pixels x channels [64 w, 64 w + 64): 48 MFMAs;
//   2. the fp32 tile goes to LDS (64 KiB) in 32-byte chunks of 8 channels whose position in the 1 KiB row is XOR-ed with
//      the row index; the epilogue thread of a chunk adds bias / identity (requested long before), applies ReLU, stores
//      the y planes (512-byte runs per row and plane) and writes hi (16 B) + lo (16 B) back INTO ITS OWN 32 bytes -- the
//      row-XOR makes exactly that image conflict-free for the A-fragment reads of the second product;
//   3. t1' = y . w1'^T with A from LDS and the B fragments (w1', L2-resident) in registers, requested before the first
//      epilogue (every fragment by one wave);
//   4. t1' through a small fp32 stage (over the dead y image) -> scale / bias / ReLU -> planes.
// Downsample form (first block of the stage): the identity x . wd^T is a second 64-deep product (x tile by LDS-DMA behind
// the first product's A tile, wd fragments in registers), joined in registers with the rounding the stored planes would have.
// Tail form: the block's 3x3 convolution (64 -> 64) runs in front of step 1 on the same tile -- the 64 + 2 W + 2 input rows of
// both 32-channel blocks resident in LDS (48 KiB), weights through a four-stage ring of contiguous 8 KiB tiles -- and hands t2
// to the first product through LDS: t2 is neither written nor read.  The w3 / wd fragments and the identity rows are
// requested four at a time behind the first eight 3x3 steps (vmcnt retires in order; the counted waits of the ring allow
// for them).
// Same K order, same MFMA order per accumulator and the same epilogue arithmetic as the gemm_x3.hip / conv_halo_x3.hip
// launches it replaces: bit-identical results (tests/test_gpu_x3.py).
#include "gemm.h"
#include "x3_fmt.h"
#include "cdna_prims.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

extern int g_dbg;                // sq_dbg_set key 1 (gemm.hip)

namespace {

// n is a constant after unrolling: the switch folds to one s_waitcnt
__device__ __forceinline__ void wait_vm_n(int n) {
    switch (n) {
        case 0: wait_vm<0>(); break;
        case 2: wait_vm<2>(); break;
        case 4: wait_vm<4>(); break;
        case 6: wait_vm<6>(); break;
        case 8: wait_vm<8>(); break;
        case 10: wait_vm<10>(); break;
        case 12: wait_vm<12>(); break;
        case 14: wait_vm<14>(); break;
        case 16: wait_vm<16>(); break;
        default: wait_vm<0>(); break;
    }
}

constexpr int PX = 64, K1 = 64, N1 = 256;
constexpr int A_PLANE = PX * 64;                 // one plane of one K-tile of t2: 4 KiB
constexpr int B_PLANE = N1 * 64;                 // ... of w3: 16 KiB
constexpr int KT_BYTES = 2 * A_PLANE + 2 * B_PLANE;    // 40 KiB
constexpr int LDS_BYTES = 2 * KT_BYTES;          // 80 KiB (the y image needs 64 KiB of it)
constexpr int YROW = N1 * 4;                     // 1 KiB per pixel: fp32, then 32 x [hi 16 B | lo 16 B]

struct ChainX3Args {
    const uint16_t* t2; long long plT2;          // [P, 64] planes
    const uint16_t* w3; const uint16_t* w1n; long long plW;     // [256, 64] / [N2, 256]; lo plane plW elements behind
    const float* b3; const float* cs3; const float* b1n; const float* cs1n;
    const uint16_t* res; long long plRes;        // identity [P, 256]
    uint16_t* y; long long plY;                  // [P, 256]
    uint16_t* t1n; long long plT1n;              // [P, N2]
    int P;
    uint32_t t2_bytes, w3_bytes;                 // descriptor extents of one plane
    // downsample form (first block of the stage): identity = xin . wd^T * sd + bd (src/resnet.py:87-88), computed here from
    // the block's 64-channel input instead of being written and read back as a 256-channel tensor; res is unused then
    const uint16_t* xin; long long plX;          // [P, 64]
    const uint16_t* wd;                          // [256, 64], lo plane plW behind
    const float* bd; const float* csd;
    uint32_t wd_bytes;
    // tail form: t2 is not read but computed here, t2 = relu(conv3x3(t1) * s2 + b2) (src/resnet.py:79-81), from t1 [P, 64]
    const uint16_t* t1; long long plT1;
    const uint16_t* w2;                          // [64, 576], k = (kh*3 + kw)*64 + cin; lo plane plW behind
    const float* b2; const float* cs2;
    uint32_t w2_bytes;
    int W, HW;                                   // map width and pixels per image (HW / W rows)
    int dbg;                                     // ablation switches (tools/chain_probe.py): 1 no stores, 2 no identity reads, 4 no 3x3, 8 no second product
    int xcd_walk;                                // tile walk (kernel comment)
};

template <int N2, bool F16, bool DS, bool TAIL, bool WIDE = false>
__global__ __launch_bounds__(256, 2) void chain_x3_kernel(const ChainX3Args p) {
    using Fmt = X3Fmt<F16>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;

    const auto rsTh = __builtin_amdgcn_make_buffer_rsrc((void*)p.t2, 0, (int)p.t2_bytes, SQ_RSRC_FLAGS);
    const auto rsTl = __builtin_amdgcn_make_buffer_rsrc((void*)(p.t2 + p.plT2), 0, (int)p.t2_bytes, SQ_RSRC_FLAGS);
    const auto rsXh = __builtin_amdgcn_make_buffer_rsrc((void*)(DS ? p.xin : p.t2), 0, (int)p.t2_bytes, SQ_RSRC_FLAGS);
    const auto rsXl = __builtin_amdgcn_make_buffer_rsrc((void*)(DS ? p.xin + p.plX : p.t2 + p.plT2), 0, (int)p.t2_bytes, SQ_RSRC_FLAGS);

    // B fragments of the second product come straight from L2 into registers (w1' is 64 / 128 KiB: no room in LDS beside the
    // y image), four k-steps per group, the next group requested while the current one is multiplied, the first one before
    // the first epilogue.  Every wave owns one 32-column tile of t1' (N2 = 64: waves (pi, cj) = 32 pixels x tile cj;
    // N2 = 128: wave w = all 64 pixels x tile w, so that no fragment is loaded twice).
    // lane (n = l31, half lh) of k-step s holds k = 16 s + 8 lh .. + 8 of row n.
    constexpr int NI2 = N2 == 64 ? 1 : 2;        // 32-pixel tiles of t1' per wave
    const int pi = N2 == 64 ? wave >> 1 : 0, cj = N2 == 64 ? wave & 1 : wave;
    const uint16_t* const w1src = p.w1n + (size_t)cj * 16 * 512 + lane * 8;      // fragment order: 1 KiB per (column tile, k-step)
    constexpr int W1PRE = DS ? 4 : 3;            // groups of w1' (of 4) requested before the first epilogue; the rest when the identity registers are free
    u32x4 wbh[4][4], wbl[4][4];
    auto load_w1 = [&](int g, int slot) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            wbh[slot][s] = *reinterpret_cast<const u32x4*>(w1src + (g * 4 + s) * 512);
            wbl[slot][s] = *reinterpret_cast<const u32x4*>(w1src + p.plW + (g * 4 + s) * 512);
        }
    };
    // Tile walk of the tail form (p.xcd_walk; SQ_X3_TAIL_XCD_WALK = 0 plain order, 1 one contiguous run per XCD, n chunks of n tiles;
    // default 64).  Workgroups go to the XCDs round-robin, so in the plain order the tiles that share the 3x3's 2 W + 2 halo rows run
    // under eight different L2s and every halo row crosses the fabric again: 1.17 / 1.19 / 1.27 x the algorithmic bytes by the
    // counters.  With chunks of 64 consecutive tiles per XCD (what its 32 CUs hold at a time) the re-reads are L2 hits: 1.007 / 1.02 /
    // 1.03 x, 4.3 GB less per 1000 patches -- at the SAME rate (profiles/r05_tail_xcd_walk_ab.txt: the re-reads were served by the
    // memory-side cache, never by DRAM; the launch is bound inside the CU).
    int tile_id = blockIdx.x;
    if (p.xcd_walk == 1) {
        // sq_xcd_tile (tile_walk.h) written out: through the call hipcc schedules this kernel differently
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, x = blockIdx.x & 7, i = blockIdx.x >> 3;
        tile_id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    } else if (p.xcd_walk > 1) {
        // chunked: XCD x takes chunks x, x + 8, ... of xcd_walk consecutive tiles (the chip as a whole still sweeps the tensor front to back)
        const int c = p.xcd_walk, x = blockIdx.x & 7, i = blockIdx.x >> 3;
        const int full = (int)(gridDim.x / (8 * c)) * (8 * c);          // tiles covered by whole rounds of eight chunks; the ragged rest keeps the plain order
        if ((int)blockIdx.x < full) tile_id = ((i / c) * 8 + x) * c + i % c;
    }
    const int p0 = tile_id * PX;
    // ---- the launch's long-latency reads are requested before anything else and land while the 3x3 runs:
    // (a) the B fragments of the 64-deep products.  Wave w multiplies all 64 pixels by channels [64 w, 64 w + 64): no other
    //     wave reads those rows of w3 / wd, so they go straight from L2 into registers (lane (n = l31, half lh) of k-step ks
    //     holds k = 16 ks + 8 lh .. + 8 of row 64 w + 32 j + n) instead of through LDS;
    // (b) the identity rows of this thread's eight epilogue chunks (1 KiB per pixel, the launch's largest HBM read).
    // In the tail form these 32 reads are dealt four at a time behind the first eight steps of the 3x3 (vmcnt retires in
    // order: requested in front of the input rows they would hold up the first step, requested at the end nothing hides them).
    u32x4 w3h[2][4], w3l[2][4], wdh[2][4], wdl[2][4];
    auto load_wfrag = [&](const uint16_t* w, u32x4 (&h)[2][4], u32x4 (&l)[2][4], int ks) {      // k-step ks: 4 reads
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint16_t* src = w + (size_t)((wave * 2 + j) * 4 + ks) * 512 + lane * 8;       // fragment order: 1 KiB per (row tile, k-step)
            h[j][ks] = *reinterpret_cast<const u32x4*>(src);
            l[j][ks] = *reinterpret_cast<const u32x4*>(src + p.plW);
        }
    };
    const int c8 = tid & 31, rsub = tid >> 5;      // epilogue thread = (8-channel chunk c8, rows rsub + 8 u)
    u32x4 rh[8], rl[8];
    auto load_res = [&](int u) {                   // identity chunk of row rsub + 8 u: 2 reads
        const int m = min(p0 + u * 8 + rsub, p.P - 1);      // rows past P repeat the last one (never stored): no branch around the read
        const u32x4* qh = reinterpret_cast<const u32x4*>(p.res + (size_t)m * N1 + c8 * 8);
        const u32x4* ql = reinterpret_cast<const u32x4*>(p.res + p.plRes + (size_t)m * N1 + c8 * 8);
        rh[u] = *qh; rl[u] = *ql;
    };
    constexpr int NEXTRA = 8;
    auto extra_reads = [&](int k) {                // group k of NEXTRA, 4 reads each
        if (k < 4) load_wfrag(p.w3, w3h, w3l, k);
        else if constexpr (DS) load_wfrag(p.wd, wdh, wdl, k - 4);
        else if (!(p.dbg & 2)) { load_res(2 * (k - 4)); load_res(2 * (k - 4) + 1); }
    };
    // A tile of a 64-deep product ([64 px][64 k] planes of t2 or of the block's input) by LDS-DMA: K-tile kt at
    // smem + kt * KT_BYTES + a_off, hi plane then lo plane, 64-byte rows, chunk ^= (row >> 2) & 3
    auto load_a = [&](__amdgpu_buffer_rsrc_t ah_, __amdgpu_buffer_rsrc_t al_, int a_off) {
        const int r0 = tid >> 2, gc = (tid & 3) ^ ((r0 >> 2) & 3);
        const int m = p0 + r0;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            char* buf = smem + kt * KT_BYTES + a_off + wave * 1024;
            const uint32_t oa = m < p.P ? ((uint32_t)m * K1 + (uint32_t)(kt * 32 + gc * 8)) * 2u : SQ_OOB;
            glds16(ah_, buf, oa);
            glds16(al_, buf + A_PLANE, oa);
        }
    };
    constexpr int X_OFF = 2 * A_PLANE;           // the downsample product's A tile sits behind the first product's
    if constexpr (TAIL) {
        // ---- 0. t2 = relu(conv3x3(t1) * s2 + b2) for this tile, never leaving the CU.  The tile's 64 flat pixels need the
        // contiguous rows [p0 - W - 1, p0 + 64 + W + 1) of t1 (<= 192 rows, W <= 62): both 32-channel blocks and both planes
        // arrive at once (48 KiB); the weights stream as 18 tiles [64 n][32 k] x 2 planes through a four-stage ring (32 KiB).
        // WIDE (maps 63 .. 70 wide -- the 64 x 64 maps of 256-pixel patches, the reference's default size,
        // pre_processing/patch_gen_hdf5.py:157): <= 206 rows in 208-row planes (52 KiB) and a THREE-stage ring (24 KiB), so
        // that the block still fits 80 KiB and two of them a CU.
        // 4 waves = 2 (32 pixels) x 2 (32 channels), 6 MFMAs per wave and step -- the same K order (channel block, tap) and
        // MFMA sequence as conv_halo_x3.hip.  The result goes to LDS as the A image of the first product.
        constexpr int HROWS = WIDE ? 208 : 192, HPL = HROWS * 64, HCB = 2 * HPL, WST = 8192;
        constexpr int NST = WIDE ? 3 : 4, DEPTH = NST - 1, NROUND = (HROWS + 63) / 64;
        static_assert(2 * HCB + NST * WST <= LDS_BYTES, "tail form: input rows + weight ring exceed the block's LDS");
        char* const HB = smem;
        char* const WR = smem + 2 * HCB;
        const int W = p.W;
        const auto rs1h = __builtin_amdgcn_make_buffer_rsrc((void*)p.t1, 0, (int)p.t2_bytes, SQ_RSRC_FLAGS);
        const auto rs1l = __builtin_amdgcn_make_buffer_rsrc((void*)(p.t1 + p.plT1), 0, (int)p.t2_bytes, SQ_RSRC_FLAGS);
        const auto rs2h = __builtin_amdgcn_make_buffer_rsrc((void*)p.w2, 0, (int)p.w2_bytes, SQ_RSRC_FLAGS);
        const auto rs2l = __builtin_amdgcn_make_buffer_rsrc((void*)(p.w2 + p.plW), 0, (int)p.w2_bytes, SQ_RSRC_FLAGS);
        {
            const int halo0 = p0 - W - 1, halo_slots = (PX + 2 * W + 2) * 4;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int u = 0; u < NROUND; ++u) {
                    if (u * 64 + wave * 16 >= HROWS) continue;          // (wave-uniform) the last round of the 208-row planes: one chunk of 16 rows
                    const int sl = u * 256 + tid;
                    const int row = sl >> 2, c = (sl & 3) ^ ((row >> 2) & 3);
                    const int px = halo0 + row;
                    const bool ok = sl < halo_slots && px >= 0 && px < p.P;
                    const uint32_t off = ok ? ((uint32_t)px * 64u + (uint32_t)(cb * 32 + c * 8)) * 2u : SQ_OOB;
                    char* dst = HB + cb * HCB + u * 4096 + wave * 1024;
                    glds16(rs1h, dst, off);
                    glds16(rs1l, dst + HPL, off);
                }
        }
        const int wn_ = tid >> 2, wc_ = (tid & 3) ^ ((wn_ >> 2) & 3);
        // step g of the K walk: (channel block, tap) = (g / 9, g % 9) -- conv_halo_x3.hip's order -- or, WIDE, (g & 1, g >> 1): the
        // tap-major order of the implicit-GEMM kernel that takes these maps when the 3x3 runs on its own (conv_halo_x3.hip stops
        // at 63 columns), so that either form stays bit-identical to its unfused path.  Weight tile of a step: cb * 9 + tap.
        auto issue_w2 = [&](int g, int stage) {
            const int tile = WIDE ? (g & 1) * 9 + (g >> 1) : g;
            const uint32_t off = ((uint32_t)tile * 2048u + (uint32_t)(wn_ * 32 + wc_ * 8)) * 2u;   // tile = [64 n][32 k], contiguous
            char* dst = WR + stage * WST + wave * 1024;
            glds16(rs2h, dst, off);
            glds16(rs2l, dst + 4096, off);
        };
#pragma unroll
        for (int g0 = 0; g0 < DEPTH; ++g0) issue_w2(g0, g0);
        asm volatile("" ::: "memory");
        const int pi3 = wave >> 1, cj3 = wave & 1;
        const int ml = pi3 * 32 + l31;
        uint32_t mask = 0;
        {
            const int px = p0 + ml;
            if (px < p.P) {
                const int rem = px % p.HW, r = rem / W, c = rem - r * W, H = p.HW / W;
#pragma unroll
                for (int tp = 0; tp < 9; ++tp) {
                    const int rr = r + tp / 3 - 1, cc = c + tp % 3 - 1;
                    if (rr >= 0 && rr < H && cc >= 0 && cc < W) mask |= 1u << tp;
                }
            }
        }
        const int jc = ml + W + 1;
        const int brow = cj3 * 32 + l31;
        f32x16 acc3;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc3[e] = 0.f;
        if (!(p.dbg & 4))
#pragma unroll
            for (int g = 0; g < 18; ++g) {
                const int cb = WIDE ? (g & 1) : g / 9, tap = WIDE ? (g >> 1) : g % 9;
                // tile g (and everything older) landed.  Requested after it, in this order (DEPTH = 3): extra group g-3 (4 reads),
                // tile g+1 (2), extra g-2, tile g+2, extra g-1 -- those that exist may stay in flight
                {
                    int n = 0;
#pragma unroll
                    for (int k = g - DEPTH; k < g; ++k) n += (k >= 0 && k < NEXTRA) ? 4 : 0;
#pragma unroll
                    for (int j = g + 1; j <= g + DEPTH - 1; ++j) n += j < 18 ? 2 : 0;
                    wait_vm_n(n);
                }
                __builtin_amdgcn_s_barrier();
                const int j = jc + (tap / 3 - 1) * W + (tap % 3 - 1);
                const char* arow = HB + cb * HCB + j * 64;
                const int asw = (j >> 2) & 3;
                const bool aok = (mask >> tap) & 1u;
                const char* wt = WR + (g % NST) * WST + brow * 64;
                const int bsw = (brow >> 2) & 3;
                u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    ah[s2] = lds128(arow + (((2 * s2 + lh) ^ asw) << 4)); al[s2] = lds128(arow + HPL + (((2 * s2 + lh) ^ asw) << 4));
                    if (!aok) { ah[s2] = u32x4{0, 0, 0, 0}; al[s2] = u32x4{0, 0, 0, 0}; }
                    bh[s2] = lds128(wt + (((2 * s2 + lh) ^ bsw) << 4)); bl[s2] = lds128(wt + 4096 + (((2 * s2 + lh) ^ bsw) << 4));
                }
                if (g + DEPTH < 18) issue_w2(g + DEPTH, (g + DEPTH) % NST);     // into the stage read at step g - 1; behind the fragment reads, whose latency covers the DMA issue
                asm volatile("" ::: "memory");           // (the counted waits above rely on this order)
                if (g < NEXTRA) extra_reads(g);
                asm volatile("" ::: "memory");
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    Fmt::mma(al[s2], bh[s2], acc3);
                    Fmt::mma(ah[s2], bl[s2], acc3);
                    Fmt::mma(ah[s2], bh[s2], acc3);
                }
            }
        __syncthreads();                         // the input rows and the weight ring are dead
        if constexpr (DS) load_a(rsXh, rsXl, X_OFF);           // the block's input tile for the downsample product
        {
            const float s2v = p.cs2 ? p.cs2[brow] : 1.f, b2v = p.b2[brow];
            const int ck = (brow & 31) >> 3;       // K-tile of the image = channel / 32 (= cj3), 16-byte chunk ck, byte (channel & 7) * 2
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float v0 = x3_relu(s2v * acc3[r] + b2v), v1 = x3_relu(s2v * acc3[r + 1] + b2v);
                const uint32_t h = Fmt::pack2(v0, v1);
                const uint32_t l = Fmt::rest2(v0, v1, h);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int row = pi3 * 32 + (r & 3) + e + 8 * (r >> 2) + 4 * lh;
                    char* dst = smem + cj3 * KT_BYTES + row * 64 + ((ck ^ ((row >> 2) & 3)) << 4) + (brow & 7) * 2;
                    *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(e ? h >> 16 : h & 0xffffu);
                    *reinterpret_cast<uint16_t*>(dst + A_PLANE) = (uint16_t)(e ? l >> 16 : l & 0xffffu);
                }
            }
        }
    } else {
        load_a(rsTh, rsTl, 0);
        if constexpr (DS) load_a(rsXh, rsXl, X_OFF);
#pragma unroll
        for (int k = 0; k < NEXTRA; ++k) extra_reads(k);
    }
    // epilogue constants of this thread's 8-channel chunk
    float bias8[8], scale8[8];
    {
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.b3 + c8 * 8), b1 = *reinterpret_cast<const f32x4*>(p.b3 + c8 * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { bias8[e] = b0[e]; bias8[4 + e] = b1[e]; scale8[e] = 1.f; scale8[4 + e] = 1.f; }
        if (p.cs3) {
            const f32x4 s0 = *reinterpret_cast<const f32x4*>(p.cs3 + c8 * 8), s1 = *reinterpret_cast<const f32x4*>(p.cs3 + c8 * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { scale8[e] = s0[e]; scale8[4 + e] = s1[e]; }
        }
    }

    // ---- a 64-deep product: 64 px (A tile in LDS at a_off) x channels [64 wave, +64) (B in registers), 48 MFMAs per wave
    auto product = [&](f32x16 (&acc_)[2][2], const u32x4 (&bh)[2][4], const u32x4 (&bl)[2][4], int a_off) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc_[i][j][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const char* st = smem + (ks >> 1) * KT_BYTES + a_off;
            const int s = ks & 1;
            u32x4 ah[2], al[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = i * 32 + l31;
                const int off = row * 64 + (((2 * s + lh) ^ ((row >> 2) & 3)) << 4);
                ah[i] = lds128(st + off); al[i] = lds128(st + A_PLANE + off);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) Fmt::mma(al[i], bh[j][ks], acc_[i][j]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) Fmt::mma(ah[i], bl[j][ks], acc_[i][j]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) Fmt::mma(ah[i], bh[j][ks], acc_[i][j]);
        }
    };
    f32x16 acc[2][2];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    product(acc, w3h, w3l, 0);
    if constexpr (DS) {
        // the downsample product; its result joins the first one in registers exactly as the two launches would:
        // identity = join(split(acc_d * s_d + b_d)) (the stored planes' rounding), y = relu((acc * s3 + b3) + identity)
        f32x16 accd[2][2];
        product(accd, wdh, wdl, X_OFF);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = wave * 64 + j * 32 + l31;
            const float s3 = p.cs3 ? p.cs3[col] : 1.f, b3 = p.b3[col], sd = p.csd ? p.csd[col] : 1.f, bd = p.bd[col];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const float d0 = sd * accd[i][j][r] + bd, d1 = sd * accd[i][j][r + 1] + bd;
                    const uint32_t h = Fmt::pack2(d0, d1);
                    const uint32_t l = Fmt::rest2(d0, d1, h);
                    acc[i][j][r] = x3_relu((s3 * acc[i][j][r] + b3) + Fmt::sum_lo(h, l));
                    acc[i][j][r + 1] = x3_relu((s3 * acc[i][j][r + 1] + b3) + Fmt::sum_hi(h, l));
                }
        }
    }
    __syncthreads();                             // every wave has read its fragments: the buffers become the y image

    // ---- 2. fp32 tile -> LDS, chunk position ^= row
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int col = wave * 64 + j * 32 + l31;
                *reinterpret_cast<float*>(smem + row * YROW + ((((col >> 3) ^ (row & 31))) << 5) + (col & 7) * 4) = acc[i][j][r];
            }
#pragma unroll
    for (int g = 0; g < W1PRE; ++g) load_w1(g, g);
    __syncthreads();
    // epilogue of the first product: thread = (chunk c8, rows rsub + 8 u); the identity has been in registers since the top
    {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = u * 8 + rsub;
            const int m = p0 + row;
            char* chunk = smem + row * YROW + ((c8 ^ (row & 31)) << 5);
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(chunk), a1 = *reinterpret_cast<const f32x4*>(chunk + 16);
            float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            if constexpr (!DS) {                 // (downsample form: the stage already holds y)
                float idn[8];
                x3_join8<F16>(rh[u], rl[u], idn);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = x3_relu((scale8[e] * v[e] + bias8[e]) + idn[e]);
            }
            u32x4 hi, lo;
            x3_split8<F16>(v, hi, lo);
            *reinterpret_cast<u32x4*>(chunk) = hi;                  // rows past P: never stored, and their t1' rows neither
            *reinterpret_cast<u32x4*>(chunk + 16) = lo;
            if (m < p.P && !(p.dbg & 1)) {
                u32x4* qh = reinterpret_cast<u32x4*>(p.y + (size_t)m * N1 + c8 * 8);
                u32x4* ql = reinterpret_cast<u32x4*>(p.y + p.plY + (size_t)m * N1 + c8 * 8);
                *qh = hi; *ql = lo;
            }
        }
    }
    __syncthreads();                             // y image complete

    // ---- 3. second product: t1'[64 px][N2], K = 256, A from the y image, B from registers
    f32x16 acc2[NI2];
#pragma unroll
    for (int i = 0; i < NI2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc2[i][e] = 0.f;
    if (!(p.dbg & 8))
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (g == 0)
#pragma unroll
            for (int g2 = W1PRE; g2 < 4; ++g2) load_w1(g2, g2);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int s = g * 4 + s4;
            u32x4 ah[NI2], al[NI2];
#pragma unroll
            for (int i = 0; i < NI2; ++i) {
                const int row = (pi + i) * 32 + l31;
                const char* cp = smem + row * YROW + (((2 * s + lh) ^ (row & 31)) << 5);     // 8-channel chunk of this lane's half of the k-step
                ah[i] = lds128(cp); al[i] = lds128(cp + 16);
            }
#pragma unroll
            for (int i = 0; i < NI2; ++i) Fmt::mma(al[i], wbh[g][s4], acc2[i]);
#pragma unroll
            for (int i = 0; i < NI2; ++i) Fmt::mma(ah[i], wbl[g][s4], acc2[i]);
#pragma unroll
            for (int i = 0; i < NI2; ++i) Fmt::mma(ah[i], wbh[g][s4], acc2[i]);
        }
    }
    __syncthreads();                             // the y image is dead: its head becomes the t1' stage

    // ---- 4. t1' = relu(acc2 * s1' + b1') -> planes
    float* stage = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < NI2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (pi + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            stage[row * N2 + cj * 32 + l31] = acc2[i][r];
        }
    __syncthreads();
    {
        constexpr int NC = N2 / 8, RPP = 256 / NC, PASSES = PX / RPP;
        const int e_c8 = tid % NC, e_r = tid / NC;
        float b8[8], s8[8];
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.b1n + e_c8 * 8), b1 = *reinterpret_cast<const f32x4*>(p.b1n + e_c8 * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { b8[e] = b0[e]; b8[4 + e] = b1[e]; s8[e] = 1.f; s8[4 + e] = 1.f; }
        if (p.cs1n) {
            const f32x4 s0 = *reinterpret_cast<const f32x4*>(p.cs1n + e_c8 * 8), s1 = *reinterpret_cast<const f32x4*>(p.cs1n + e_c8 * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s8[e] = s0[e]; s8[4 + e] = s1[e]; }
        }
#pragma unroll
        for (int u = 0; u < PASSES; ++u) {
            const int row = u * RPP + e_r;
            const int m = p0 + row;
            if (m >= p.P || (p.dbg & 1)) continue;
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(stage + row * N2 + e_c8 * 8);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(stage + row * N2 + e_c8 * 8 + 4);
            float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = x3_relu(s8[e] * v[e] + b8[e]);
            u32x4 hi, lo;
            x3_split8<F16>(v, hi, lo);
            *reinterpret_cast<u32x4*>(p.t1n + (size_t)m * N2 + e_c8 * 8) = hi;
            *reinterpret_cast<u32x4*>(p.t1n + p.plT1n + (size_t)m * N2 + e_c8 * 8) = lo;
        }
    }
}

// ---- fragment-ordered weight copies.  The launch above streams ~275 KiB of weights per 64-pixel tile through the CU's
// vector-memory path, which is as busy as HBM here: read row-major, a B-fragment request touches 32
// cache lines for 1 KiB (w3 / wd / w1': 16 bytes per lane from 32 rows) and a ring tile request 16 (w2: 64 bytes from 16
// rows).  This kernel lays the block's weights out in the order the requests want them -- every wave-wide request one
// contiguous 1 KiB -- in front of each launch (a few microseconds; the weights' ABI layout stays row-major):
//   plane of SQ_CHAIN_X3_FRAG elements:  w3 @0        [(wave, j)][ks][lane][8]   row = 32 (2 wave + j) + lane % 32, k = 16 ks + 8 (lane / 32)
//                                        w1' @16384   [cj][ks 0..15][lane][8]    row = 32 cj + lane % 32,          k = 16 ks + 8 (lane / 32)
//                                        wd @49152    as w3
//                                        w2 @65536    [g = cb * 9 + tap][n][32]  k = tap * 64 + cb * 32 + ..
constexpr int FRAG = 102400, FRAG_W1 = 16384, FRAG_WD = 49152, FRAG_W2 = 65536;
// Source weights: row-major [n][K], or K-tile-major (tiled: element (n, k) at ((k / 32) * N + n) * 32 + k % 32, the layout the
// split modes' GEMM launches read, gemm.h b_tiled).
__global__ __launch_bounds__(256) void chain_x3_pack_kernel(const uint16_t* w3, const uint16_t* w1n, const uint16_t* wd, const uint16_t* w2,
                                                            long long plSrc, int n2, int tiled, uint16_t* dst) {
    auto at = [&](const uint16_t* w, int n, int k, int N, int K) { return tiled ? w + ((size_t)(k >> 5) * N + n) * 32 + (k & 31) : w + (size_t)n * K + k; };
    const int c = blockIdx.x * 256 + threadIdx.x;            // one 16-byte chunk of one plane
    if (c >= 2 * (FRAG / 8)) return;
    const int pl = c >= FRAG / 8, e0 = (c - pl * (FRAG / 8)) * 8;
    const uint16_t* src = nullptr;
    if (e0 < FRAG_W1 || (e0 >= FRAG_WD && e0 < FRAG_W2)) {
        const bool d = e0 >= FRAG_WD;
        const int r = e0 - (d ? FRAG_WD : 0), q = r >> 9, lane = (r & 511) >> 3;
        const uint16_t* w = d ? wd : w3;
        if (w) src = at(w, (q >> 2) * 32 + (lane & 31), (q & 3) * 16 + (lane >> 5) * 8, N1, K1);
    } else if (e0 < FRAG_WD) {
        const int r = e0 - FRAG_W1, q = r >> 9, lane = (r & 511) >> 3;
        if ((q >> 4) * 32 < n2) src = at(w1n, (q >> 4) * 32 + (lane & 31), (q & 15) * 16 + (lane >> 5) * 8, n2, N1);
    } else if (w2) {
        const int r = e0 - FRAG_W2, g = r >> 11, n = (r & 2047) >> 5, kk = r & 31;
        const int cb = g / 9, tap = g - cb * 9;
        src = at(w2, n, tap * 64 + cb * 32 + kk, 64, 576);
    }
    if (src) *reinterpret_cast<u32x4*>(dst + (size_t)pl * FRAG + e0) = *reinterpret_cast<const u32x4*>(src + (size_t)pl * plSrc);
}

}  // namespace

size_t sq_chain_x3_frag_bytes() { return (size_t)2 * FRAG * 2; }

// t2 [P, 64], res / y [P, 256], t1n [P, n2] (n2 = 64 or 128) as hi / lo planes (pl* = elements between the planes);
// w3 [256, 64] and w1n [n2, 256] planes plW apart (row-major, or K-tile-major when w_tiled), biases / per-channel scales fp32 (scales may be null).
// Downsample form: res == nullptr, the identity is xin [P, 64] . wd^T * csd + bd (wd [256, 64], planes plW apart).
// Tail form: t1 != nullptr -- t2 is not read but computed in the launch as relu(conv3x3(t1) * cs2 + b2) (w2 [64, 576]).
// w3_bytes / wd_bytes: bytes from the pointer to the end of one weight plane's allocation (descriptor extent).
int sq_launch_chain_x3_c64(int f16, const uint16_t* t2, long long plT2, const uint16_t* res, long long plRes, uint16_t* y, long long plY,
                           uint16_t* t1n, long long plT1n, int n2, const uint16_t* w3, const uint16_t* w1n, long long plW, size_t w3_bytes,
                           const float* b3, const float* cs3, const float* b1n, const float* cs1n,
                           const uint16_t* xin, long long plX, const uint16_t* wd, size_t wd_bytes, const float* bd, const float* csd,
                           const uint16_t* t1, long long plT1, const uint16_t* w2, size_t w2_bytes, const float* b2, const float* cs2, int W, int HW,
                           long long P, uint16_t* frag, int w_tiled, hipStream_t stream) {
    SQ_REQUIRE(n2 == 64 || n2 == 128, "chain_x3: next width %d (64 or 128)", n2);
    SQ_REQUIRE(P > 0 && P * N1 * 2 < (1ll << 31), "chain_x3: %lld pixels exceed the 2 GiB descriptor limit", P);
    const bool tail = t1 != nullptr;
    SQ_REQUIRE((t2 || tail) && y && t1n && w3 && w1n && b3 && b1n && frag && w3_bytes >= (size_t)N1 * K1 * 2, "chain_x3: null pointer / weight extent");
    SQ_REQUIRE(!tail || (w2 && b2 && w2_bytes >= (size_t)64 * 576 * 2 && W >= 3 && W <= 70 && HW >= W && HW % W == 0 && P % HW == 0),
               "chain_x3: tail form needs the 3x3 weights and maps up to 70 wide (W=%d, HW=%d)", W, HW);
    const bool wide = tail && W > 62;             // 63 .. 70: 208-row planes, three-stage weight ring
    const bool ds = res == nullptr;
    SQ_REQUIRE(!ds || (xin && wd && bd && wd_bytes >= (size_t)N1 * K1 * 2), "chain_x3: neither an identity tensor nor a downsample branch");
    ChainX3Args a;
    // the kernel reads the fragment-ordered copies (frag: sq_chain_x3_frag_bytes() of scratch, rewritten by every launch)
    hipLaunchKernelGGL(chain_x3_pack_kernel, dim3((2 * (FRAG / 8) + 255) / 256), dim3(256), 0, stream, w3, w1n, ds ? wd : nullptr,
                       tail ? w2 : nullptr, plW, n2, w_tiled, frag);
    SQ_LAUNCH_CHECK();
    a.t2 = t2; a.plT2 = plT2; a.w3 = frag; a.w1n = frag + FRAG_W1; a.plW = FRAG; a.b3 = b3; a.cs3 = cs3; a.b1n = b1n; a.cs1n = cs1n;
    a.res = res; a.plRes = plRes; a.y = y; a.plY = plY; a.t1n = t1n; a.plT1n = plT1n; a.P = (int)P;
    a.t2_bytes = (uint32_t)(P * K1 * 2);
    a.w3_bytes = sq_desc_extent(w3_bytes);
    a.xin = xin; a.plX = plX; a.wd = frag + FRAG_WD; a.bd = bd; a.csd = csd; a.wd_bytes = sq_desc_extent(wd_bytes);
    a.t1 = t1; a.plT1 = plT1; a.w2 = frag + FRAG_W2; a.b2 = b2; a.cs2 = cs2; a.w2_bytes = (uint32_t)((FRAG - FRAG_W2) * 2); a.W = W; a.HW = HW; a.dbg = g_dbg;
    { const char* e = getenv("SQ_X3_TAIL_XCD_WALK"); a.xcd_walk = tail ? (e ? atoi(e) : 64) : 0; }      // (read per launch: the tests flip it inside one process)
    using I64 = std::integral_constant<int, 64>; using I128 = std::integral_constant<int, 128>;
    using T = std::true_type; using F = std::false_type;
    auto pick_tail = [&](auto n2c, auto f16c, auto dsc) {
        return wide ? (const void*)chain_x3_kernel<decltype(n2c)::value, decltype(f16c)::value, decltype(dsc)::value, true, true>
             : tail ? (const void*)chain_x3_kernel<decltype(n2c)::value, decltype(f16c)::value, decltype(dsc)::value, true>
                    : (const void*)chain_x3_kernel<decltype(n2c)::value, decltype(f16c)::value, decltype(dsc)::value, false>;
    };
    auto pick_ds = [&](auto n2c, auto f16c) { return ds ? pick_tail(n2c, f16c, T{}) : pick_tail(n2c, f16c, F{}); };
    auto pick_f16 = [&](auto n2c) { return f16 ? pick_ds(n2c, T{}) : pick_ds(n2c, F{}); };
    const void* fn = n2 == 64 ? pick_f16(I64{}) : pick_f16(I128{});
    SQ_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    SqProf prof(stream);
    if (prof.on()) {
        char name[96];
        snprintf(name, sizeof(name), "%s_%s_c64_cn%d%s_P%lld", tail ? "tail" : "chain", f16 ? "f16x3" : "bf16x3", n2, ds ? "_ds" : "", P);
        prof.begin(name, 2.0 * P * ((tail ? 576.0 * 64 : 0.0) + 64.0 * 256 * (ds ? 2 : 1) + 256.0 * n2), (double)P * 4.0 * (64 + (ds ? 64 : 256) + 256 + n2));
    }
    const dim3 grid((unsigned)((P + PX - 1) / PX)), block(256);
    void* kargs[] = {(void*)&a};
    SQ_HIP_CHECK(hipLaunchKernel(fn, grid, block, kargs, LDS_BYTES, stream));
    return SQ_OK;
}

// Probe entry (tools/chain_probe.py): one launch over caller-provided scratch, laid out as
//   act (uint16): t1 [2][P*64] | res [2][P*256] | y [2][P*256] | t1n [2][P*128]      (hi plane, lo plane)
//   wts (uint16): two planes of 102400 elements, row-major: w3 @0, w1n @16384, wd @49152, w2 @65536;  frag: as much again
//   fp  (float):  b3 @0, cs3 @256, b1n @512, cs1n @640, bd @768, csd @1024, b2 @1280, cs2 @1344
extern "C" int sq_dbg_chain_x3(int f16, int n2, int ds, int tail, long long P, int W, void* act, void* wts, void* fp, void* frag, void* stream) {
    uint16_t* a = (uint16_t*)act;
    const uint16_t* w = (const uint16_t*)wts;
    const float* f = (const float*)fp;
    uint16_t* t1 = a; uint16_t* res = t1 + 2 * P * 64; uint16_t* y = res + 2 * P * 256; uint16_t* t1n = y + 2 * P * 256;
    const long long plW = 102400;
    return sq_launch_chain_x3_c64(f16, tail ? nullptr : t1, P * 64, ds ? nullptr : res, P * 256, y, P * 256, t1n, P * 128, n2,
                                  w, w + 16384, plW, (size_t)(plW * 2), f, f + 256, f + 512, f + 640,
                                  ds ? t1 : nullptr, P * 64, ds ? w + 49152 : nullptr, (size_t)(plW - 49152) * 2, ds ? f + 768 : nullptr, ds ? f + 1024 : nullptr,
                                  tail ? t1 : nullptr, P * 64, tail ? w + 65536 : nullptr, (size_t)(plW - 65536) * 2, tail ? f + 1280 : nullptr,
                                  tail ? f + 1344 : nullptr, W, W * W, P, (uint16_t*)frag, 0, (hipStream_t)stream);
}
