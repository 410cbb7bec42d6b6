// The 256 x 256 ring kernel of the SVM path (exact codes, and general rows as int8 digits).  Shares the operand layout, the
// source addresses and the C/D map with the 128 x 128 tile (mfma_tile.h) and the epilogue arithmetic with every decision kernel
// (svm_epilogue.h); the schedule is its own.  Overview of the SVM path: svm_tile.h.
#pragma once
#include "mfma_tile.h"
#include "svm_epilogue.h"
#include <type_traits>

namespace {

// I8 hot path, large batches: 256 SVs x 256 samples per workgroup (512 threads, 8 waves as 2 x 4, wave tile 128 x 64 =
// 4 x 2 MFMA tiles of 32x32, 128 accumulator registers), K-step 128 B per row, two 64 KiB stages.
//
// Why: what a CU can pull from L2 into LDS is ~28 B/clk (measured: exp_l2bw, and the per-K-step cycle counters of the
// 128x128 kernel), and an i8 MFMA eats operand bytes twice as fast as bf16.  A 128x128 tile needs 64 B/clk per CU at full
// matrix rate (ceiling 44 %: measured 40-43 %); 256x256 needs 32 B/clk (ceiling ~87 %).  Round 1 measured this tile at
// 574 us vs 501 us on 8192 x 2560: that was the GRID, not the tile -- 32 x 10 = 320 workgroups on 256 CUs are two rounds
// with the second one a quarter full.  It is therefore only used when the launch has enough tiles for >= ~2.5 rounds
// (rml_project_svm sizes its chunks for it), and the 128x128 kernel keeps the small batches.
// Sample tiles are paired: tile_exact[] is evaluated per 256 samples (k_tile_flags group = 2); the partial slots 2*stile and
// 2*stile+1 carry the two 128-row halves, summed exactly like the 128x128 kernel sums them.
// ------------------------------------------------------------------------------------------
constexpr int kBig = 256;

// (The two-stage 64 KiB kernel that first ran this tile -- k_svm_gemm_i8_256, rounds 2-3: 0.46-0.50 of the int8 peak -- lost to the
// ring schedule below in every same-process A/B and left the tree in round 4; its numbers are in tools/exp/README.md.)

// ------------------------------------------------------------------------------------------
// k_svm_gemm_ring<PT, DIG>: the 256 x 256 tile with a 5-slot operand-stage ring and interleaved DMA issue (round 3).
//
// What limited the two-stage kernel that ran this tile in round 2 (A/B in one process, tools/gemm_ab.py, 16 384 x 2 562 x 20 480): all 64 DMA
// instructions of a stage leave in one burst after the barrier; the burst fills the CU's VMEM queue, every wave sits in its
// in-order issue stage until its eight instructions are accepted (~100 cycles each) and no MFMA is issued meanwhile:
// step = burst (~800-1000 cycles) + 2048 MFMA cycles.  Spreading the instructions between the MFMAs hides their issue under
// the SIMD partner's matrix work, but in a two-stage scheme a late issue is a late landing (measured slower in round 2).
// So the ring: the unit is one OPERAND stage (256 rows x 128 B = 32 KiB), all 160 KiB of LDS are ring, operand-stage n
// (n = 2t: SV rows of step t, 2t+1: sample rows of step t) lives in slot n % 5.  Step t sends the sample stage of step t+1 in
// its first half and the SV stage of step t+2 in its second half, one DMA instruction after every four MFMAs, into the
// two slots step t-1 has just released: every stage has 1 to 1.5 steps to land.  Waves wait with a counted
// s_waitcnt vmcnt(4) (everything but the newest stage) and meet at a raw s_barrier -- __syncthreads() would drain the queue.
// Measured: burst issue into the ring 0.99 ms (worse than two stages: 0.87), interleaved 0.80 ms = 2.15 PetaOP/s.
// The per-SV epilogue table is loaded after the K loop into slot 4 (the epilogue's G image takes slots 0-3).
//
// Tile order: block b runs on XCD b % 8 (observed, used for speed only).  The tiles are laid out as a sequence
// [group of 8 sample tiles][SV tile][sample tile of the group] and XCD x takes the x-th eighth of it (+-1 tile): the ~32
// tiles resident on an XCD are 8 sample tiles x 4 SV tiles sharing K-slices through that XCD's L2, and every XCD gets the
// same number of tiles whatever the batch (the previous map gave XCD x the sample tiles x, x+8, ...: 69 sample tiles ->
// nine on five XCDs, eight on three, i.e. a fourth round on five eighths of the chip).
//
// DIG = 1: general rows as four balanced int8 digits of a 32-bit fixed-point value (SURVEY 8 a-5 for data that is not on
// the code grid: train.py:496-517 augmentation, a non-unit proj_zoom of predict.py:109-116, the reference's generated_data
// pickles).  Every value v (sample feature or SV component) is read as u = (v - c0) / s in [-1, 1) (c0, s per model; s a
// power of two, so float32 inputs >= s 2^-8 are represented exactly and smaller ones to 2^-32 s), I = rint(u 2^31), split
// I = a0 2^24 + a1 2^16 + a2 2^8 + a3 with a_i in [-128, 127].  Then  u_x . u_s = 2^-14 sum_{i,j} 2^-8(i+j) (a_i^x . a_j^s)
// and every digit-plane product is an exact int32 GEMM (|.| <= 2^14 K < 2^29).  The ten pairs with i + j <= 3 are kept (the
// dropped ones weigh 2^-46 per digit product: typical 1e-8 on u.u), grouped by g = i + j and accumulated from
// the least significant group up IN THE SAME int32 accumulator: after g = 3 it is divided by 256 with rounding, (acc + 128) >> 8
// (2^-31 on u.u), after g = 2 it is split R2 = 256 q + r -- q stays, R2 is parked -- and the next group accumulates on top
// (4 x 2^28.3 < 2^31), which leaves R1 = G1 + floor(R2 / 2^8) and the remainder r for the epilogue.
// The top group G0 needs its own 32 bits (u.u = 2^-14 (G0 + R1/256) is a 38-bit quantity): it is computed FIRST and parked in a
// per-workgroup HBM scratch tile (256 KiB, written once, read once in the epilogue by the lane that wrote it: L2 traffic that
// is nothing next to ten K loops) -- a second accumulator set or packed remainders in registers pushed the kernel over 256
// VGPRs and the spills landed in the K loop.  u.u carries 2^-31 absolute precision on a quantity of magnitude <= D/4 -- the
// arithmetic class of the float64 path at ~3x its rate.  d^2 = s^2 (||u_x||^2 + ||u_s||^2 - 2 u_x.u_s) with the norms of the QUANTISED
// values in float64.  The K loop runs over (pair, K-step); the DMA cursors run one and two steps ahead across pair boundaries.
// ------------------------------------------------------------------------------------------
constexpr int kOpStageBytes = kBig * kStepBytes;          // 32 KiB
constexpr int kRingSlots = 5;
constexpr int kDigPairs = 10;
constexpr uint64_t kDigI = 0x1021032100ull;     // nibble p: sample digit of pair p   (0 = most significant)
constexpr uint64_t kDigJ = 0x0101201230ull;     // nibble p: SV digit of pair p; pair 0: g = 0, 1-4: g = 3, 5-7: g = 2, 8-9: g = 1
constexpr int kDigStashBytes = kBig * kBig * 4;  // the parked top-group accumulators of one workgroup

struct RingArgs {
    const uint8_t* sv; const uint8_t* x;       // operand bases (digit plane 0)
    int64_t ld_sv, ld_x;                       // bytes per row
    int64_t sv_plane, x_plane;                 // DIG: bytes between digit planes
    int KT;                                    // K-steps (per digit pair)
    int64_t N, Mpad, sv_rows; int ST, FT;      // ST / FT count 128-row tiles like GemmArgs
    const int32_t* tile_exact; int want;
    const int32_t* x_isum; const int64_t* x_isq;   // exact path row statistics
    const double* x_nsq;                            // DIG: ||u_x||^2
    const double* sv_term;                          // exact: per-SV term; DIG: ||u_s||^2
    const double* W;
    double gs; int kernel;
    double* partial; int64_t Npart;
    int32_t* stash;                            // DIG: gridDim.x * 2 * 256 KiB of scratch: the top digit group and the g = 2 level
};

// ring tile of block b: false = nothing to do
__device__ __forceinline__ bool ring_tile(int b, int FT2, int ST2, int& ftile, int& stile) {
    const int T = FT2 * ST2, q = T >> 3, r = T & 7;
    const int xcd = b & 7, k = b >> 3;
    if (k >= q + (xcd < r ? 1 : 0)) return false;
    const int pos = xcd * q + (xcd < r ? xcd : r) + k;
    const int G = 8 * ST2, fg = pos / G, rem = pos - fg * G;
    const int left = FT2 - 8 * fg, scnt = left < 8 ? left : 8;
    stile = rem / scnt;
    ftile = fg * 8 + (rem - stile * scnt);
    return true;
}
inline unsigned ring_grid(int FT2, int ST2) { const int T = FT2 * ST2; return (unsigned)(8 * ((T + 7) / 8)); }

// The parked accumulators of the DIG kernel: 16 bytes per lane and visit, 512 lanes apart.  A running pointer with a register
// anchor: 32 hoisted 64-bit addresses would be spilled.
struct StashCursor {
    v4i* sp;
    __device__ __forceinline__ v4i at(int off) const { return *(sp + off); }
    __device__ __forceinline__ void next() { sp += 512; asm volatile("" : "+v"(sp)); }
    __device__ __forceinline__ void park(int off, v4i v) { *(sp + off) = v; next(); }
};
// visit(cursor, i, j, r4) for every group of four accumulator registers of the wave tile, in the order they are parked
template <class Visit>
__device__ __forceinline__ void stash_walk(v4i* base, Visit visit) {
    StashCursor sc{base};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) visit(sc, i, j, r4);
}

template <int PT, int DIG>
__global__ __launch_bounds__(512, 2) void k_svm_gemm_ring(RingArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3;           // 2 x 4 waves; wave tile = 128 SVs x 64 samples
    const int FT2 = (a.FT + 1) >> 1, ST2 = (int)((a.Mpad + kBig - 1) / kBig);
    int ftile, stile;
    if (!ring_tile(blockIdx.x, FT2, ST2, ftile, stile)) return;
    if (a.tile_exact && a.tile_exact[2 * ftile] != a.want) return;
    const int64_t f0 = (int64_t)ftile * kBig;
    const int64_t m0 = (int64_t)stile * kBig;

    const uint8_t* gsv[4];
    const uint8_t* gx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        gsv[q] = stage_src<true>(a.sv, a.ld_sv, m0, a.sv_rows, wave, q, lane);
        gx[q] = stage_src<true>(a.x, a.ld_x, f0, a.N, wave, q, lane);
    }
    // DMA cursors: byte offset (digit plane + K-step) of the next sample stage / SV stage to send, and their ring slots
    const int64_t kbytes = (int64_t)a.KT * kStepBytes;
    int64_t ox = 0, os = 0;                            // offsets within the current pair
    int64_t px = 0, ps = 0;                            // plane offsets of the current pair
    int qx = 0, qs = 0;                                // pair indices (DIG)
    if constexpr (DIG) { px = (int64_t)(kDigI & 15) * a.x_plane; ps = (int64_t)(kDigJ & 15) * a.sv_plane; }
    auto adv_x = [&]() __attribute__((always_inline)) {
        ox += kStepBytes;
        if constexpr (DIG) { if (ox == kbytes) { ox = 0; ++qx; px = (int64_t)((kDigI >> (4 * qx)) & 15) * a.x_plane; } }
    };
    auto adv_s = [&]() __attribute__((always_inline)) {
        os += kStepBytes;
        if constexpr (DIG) { if (os == kbytes) { os = 0; ++qs; ps = (int64_t)((kDigJ >> (4 * qs)) & 15) * a.sv_plane; } }
    };
    auto burst_s = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) glds16(gsv[q] + ps + os, smem + slot * kOpStageBytes + wave * 4096 + q * 1024);
        adv_s();
    };
    auto burst_x = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) glds16(gx[q] + px + ox, smem + slot * kOpStageBytes + wave * 4096 + q * 1024);
        adv_x();
    };

    int aoff[4], asw[4], boff[2], bsw[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        int ra = wr * 128 + t * 32 + (lane & 31);
        aoff[t] = ra * kStepBytes; asw[t] = (ra >> 1) & 7;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        int rb = wc * 64 + t * 32 + (lane & 31);
        boff[t] = rb * kStepBytes; bsw[t] = (rb >> 1) & 7;
    }
    const int chalf = lane >> 5;

    v16i acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    const int TT = (DIG ? kDigPairs : 1) * a.KT;       // steps in all
    burst_s(0); burst_x(1);                            // SV_0, X_0
    if (TT > 1) burst_s(2);                            // SV_1
    int sa = 0;                                        // slot of the SV stage of the step being computed
    int sx = 3, ss = 4;                                // slots of the two stages step 0 sends
    int t = 0;                                         // global step
    // Fragment registers: two sets.  The loop is ROTATED by one MFMA group: the last sub-step (kk = 3) of a step is issued
    // after the next step's barrier, right behind that step's first fragment reads.  After a barrier all eight waves read
    // fragments at once (128 KiB per step through a 256 B/clk LDS = ~500 cycles in which, unrotated, no wave has an MFMA to
    // issue); the deferred group is matrix work that needs no LDS.
    v4i af[2][4], bf[2][2];
    auto mfma_half = [&](int set, int half) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 2 * half; i < 2 * half + 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[set][i], bf[set][j], acc[i][j], 0, 0, 0);
    };
    auto step = [&](auto first_) __attribute__((always_inline)) {
        constexpr bool FIRST = decltype(first_)::value;      // first step of a segment: no deferred group pending
        const bool hx = t + 1 < TT, hs = t + 2 < TT;
        // stages 2t and 2t+1 landed: everything this wave sent except the newest stage (the SV stage of step t+1); and this
        // wave's fragment reads of step t-1 are complete (their slots are released at the barrier)
        if (hx) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                  // ... for every wave's pieces; and step t-1 is consumed by everyone
        asm volatile("" ::: "memory");
        const int sbx = sa + 1 == kRingSlots ? 0 : sa + 1;
        const unsigned char* pa = smem + sa * kOpStageBytes;
        const unsigned char* pb = smem + sbx * kOpStageBytes;
        sa = sa + 2 >= kRingSlots ? sa + 2 - kRingSlots : sa + 2;
        unsigned char* dx = smem + sx * kOpStageBytes + wave * 4096;
        unsigned char* dsv = smem + ss * kOpStageBytes + wave * 4096;
        sx = sx + 2 >= kRingSlots ? sx + 2 - kRingSlots : sx + 2;
        ss = ss + 2 >= kRingSlots ? ss + 2 - kRingSlots : ss + 2;
        const int64_t offx = px + ox, offs = ps + os;
        auto reads = [&](int set, int kk) __attribute__((always_inline)) {
            const int ch = 2 * kk + chalf;
#pragma unroll
            for (int u = 0; u < 4; ++u) af[set][u] = *reinterpret_cast<const v4i*>(pa + aoff[u] + ((ch ^ asw[u]) << 4));
#pragma unroll
            for (int u = 0; u < 2; ++u) bf[set][u] = *reinterpret_cast<const v4i*>(pb + boff[u] + ((ch ^ bsw[u]) << 4));
        };
        auto dma = [&](int g) __attribute__((always_inline)) {                         // DMA instruction 0..7 of this step
            if (g < 4) { if (hx) glds16(gx[g] + offx, dx + g * 1024); }
            else       { if (hs) glds16(gsv[g - 4] + offs, dsv + (g - 4) * 1024); }
        };
        // group r of the step: r = 0 is the deferred kk = 3 of the previous step (set 1), r = 1..3 are kk = 0..2 of this one
        reads(0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int set = (r + 1) & 1;                // r = 0 -> set 1 (deferred), r = 1 -> set 0 (kk = 0), ...
            if (r >= 1) {
                reads(r & 1, r);                        // fragments of kk = r into the set the previous group has just used
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                if (!(FIRST && r == 0)) mfma_half(set, half);
                __builtin_amdgcn_sched_barrier(0);
                dma(2 * r + half);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (hx) adv_x();
        if (hs) adv_s();
        ++t;
    };
    auto flush = [&]() __attribute__((always_inline)) {                               // the deferred kk = 3 of a segment's last step
        __builtin_amdgcn_sched_barrier(0);
        mfma_half(1, 0); mfma_half(1, 1);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto segment = [&](int nsteps) __attribute__((always_inline)) {
        step(std::true_type{});
        for (int n = nsteps - 1; n > 0; --n) step(std::false_type{});
        flush();
    };

    // DIG: the top group's accumulators are parked in this workgroup's scratch tile, 16 bytes per lane and store, coalesced
    v4i* stash = nullptr;
    if constexpr (DIG) {
        stash = reinterpret_cast<v4i*>(a.stash) + (int64_t)blockIdx.x * (2 * kDigStashBytes / 16) + tid;
        segment(a.KT);                                 // pair 0: g = 0
        stash_walk(stash, [&](StashCursor& sc, int i, int j, int r4) {
            sc.park(0, v4i{acc[i][j][4 * r4], acc[i][j][4 * r4 + 1], acc[i][j][4 * r4 + 2], acc[i][j][4 * r4 + 3]});
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][4 * r4 + r] = 0;
        });
        // stores and DMA loads share the VM counter and may complete out of order with respect to each other: drain once, so
        // that the counted waits of the next segment see DMA instructions only
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // groups g = 3 (pairs 1-4), g = 2 (5-7), g = 1 (8-9).  After g = 3 the accumulator is divided by 256 with rounding (2^-31
        // on u.u); after g = 2 it is split R2 = 256 q + r: q stays and g = 1 accumulates on top, R2 itself is parked in the second
        // scratch tile so that the epilogue puts the remainder r back -- no rounding at the 2^-23 level
#pragma nounroll                                       // one copy of the step bodies for the three groups (instruction cache)
        for (int g = 0; g < 3; ++g) {
            segment((4 - g) * a.KT);
            if (g == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[i][j][r] = (acc[i][j][r] + 128) >> 8;
            } else if (g == 1) {
                stash_walk(stash + kDigStashBytes / 16, [&](StashCursor& sc, int i, int j, int r4) {     // second tile of this workgroup
                    sc.park(0, v4i{acc[i][j][4 * r4], acc[i][j][4 * r4 + 1], acc[i][j][4 * r4 + 2], acc[i][j][4 * r4 + 3]});
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][j][4 * r4 + r] >>= 8;      // floor: the remainder comes back in the epilogue
                });
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // stores and DMA loads share the VM counter (see above)
            }
        }
    } else {
        segment(a.KT);
    }

    // ---- fused float64 epilogue; the per-SV table is loaded now, into slot 4 ----
    const bool rbf = (a.kernel == RML_KERNEL_RBF);
    double* svw = reinterpret_cast<double*>(smem + 4 * kOpStageBytes);     // [256][1+PT] + exp table
    __syncthreads();                                   // every wave is done with the ring
    const double* etab = load_sv_table<PT, kBig, 512, true>(svw, a.sv_term, a.W, a.Mpad, m0, tid);
    if constexpr (DIG) {
        // one 64-sample quarter (= one wave column wc) at a time through LDS as float64:
        // u.u = 2^-22 (256 G0 + R1), G0 from the scratch tile;  d^2 = s^2 (||u_x||^2 + ||u_s||^2 - 2 u.u);  a.gs = gamma s^2
        double* gd = reinterpret_cast<double*>(smem);      // [256 SVs][64 samples]
        const int nq = tid & 63, qd = tid >> 6;            // sample column of the quarter, SV group (32 rows)
        for (int pass = 0; pass < 4; ++pass) {
            __syncthreads();
            if (wc == pass) {
                stash_walk(stash, [&](StashCursor& sc, int i, int j, int r4) {
                    const v4i g0 = sc.at(0);
                    const v4i r2 = sc.at(kDigStashBytes / 16);
                    sc.next();
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int r = 4 * r4 + rr;
                        const int ml = cd32_row(wr * 128 + i * 32, r, lane);
                        const int nn = cd32_col(j * 32, lane);
                        // 2^22 u.u = 256 G0 + (G1 + floor(R2 / 256)) + (R2 mod 256) / 256
                        gd[ml * 64 + nn] = ((double)g0[rr] * 256.0 + (double)acc[i][j][r] + (double)(r2[rr] & 255) * 0x1p-8) * 0x1p-22;
                    }
                });
            }
            __syncthreads();
            const int64_t n = f0 + pass * 64 + nq;
            const int64_t nc = n < a.N ? n : a.N - 1;
            const double xt = a.x_nsq[nc];
            double S[PT];
            chain_run<PT, 32, false>(S, svw, qd * 32, true, xt, a.gs, etab, [&](int ml) { return gd[ml * 64 + nq]; }, [](int, double) {});
            __syncthreads();                               // G quarter consumed: reuse its LDS for the exchange
            double* x8 = gd;                               // [8 groups][64][PT]
#pragma unroll
            for (int p = 0; p < PT; ++p) x8[(qd * 64 + nq) * PT + p] = S[p];
            __syncthreads();
            if (qd == 0 && n < a.N) {
#pragma unroll
                for (int p = 0; p < PT; ++p) {
                    double tsum = 0.0;
#pragma unroll
                    for (int g = 0; g < 8; ++g) tsum += x8[(g * 64 + nq) * PT + p];
                    a.partial[((int64_t)(2 * stile) * a.Npart + n) * PT + p] = tsum;
                    if (2 * stile + 1 < a.ST) a.partial[((int64_t)(2 * stile + 1) * a.Npart + n) * PT + p] = 0.0;
                }
            }
        }
    } else {
        int* gl = reinterpret_cast<int*>(smem);
        const int nl = tid & 127, h = tid >> 7;
        for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();
            if ((wc >> 1) == pass) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int ml = cd32_row(wr * 128 + i * 32, r, lane);
                            const int nn = cd32_col((wc & 1) * 64 + j * 32, lane);
                            gl[ml * kTile + nn] = acc[i][j][r];
                        }
            }
            __syncthreads();
            const int64_t n = f0 + pass * kTile + nl;
            const int64_t nc = n < a.N ? n : a.N - 1;
            const double xt = exact_sample_term(rbf, a.x_isum, a.x_isq, nc);
            double S[PT];
            const int* gcol = gl + nl;
            chain_run<PT, 64, true>(S, svw, h * 64, rbf, xt, a.gs, etab, [&](int ml) { return (double)gcol[ml * kTile]; }, [](int, double) {});
            __syncthreads();
            double* x4 = reinterpret_cast<double*>(smem);  // [4][128][PT]
#pragma unroll
            for (int p = 0; p < PT; ++p) x4[(h * kTile + nl) * PT + p] = S[p];
            __syncthreads();
            if (h == 0 && n < a.N) {
#pragma unroll
                for (int p = 0; p < PT; ++p) {
                    // one partial per 128 SV rows, each the sum of two 64-row in-lane chains: the very values, in the very order,
                    // the 128 x 128 kernel writes for these rows -- decision values do not depend on which kernel ran
                    a.partial[((int64_t)(2 * stile) * a.Npart + n) * PT + p] = x4[(0 * kTile + nl) * PT + p] + x4[(1 * kTile + nl) * PT + p];
                    if (2 * stile + 1 < a.ST)
                        a.partial[((int64_t)(2 * stile + 1) * a.Npart + n) * PT + p] = x4[(2 * kTile + nl) * PT + p] + x4[(3 * kTile + nl) * PT + p];
                }
            }
        }
    }
}

template <int DIG>
int launch_gemm_ring(const rml_svm* m, const RingArgs& ra, hipStream_t st) {
    const int FT2 = (ra.FT + 1) / 2, ST2 = (int)((m->Mpad + kBig - 1) / kBig);
    dim3 grid(ring_grid(FT2, ST2)), block(512);
    const size_t lds = (size_t)kRingSlots * kOpStageBytes;
#define RML_RING_CASE(PTV)                                                                                         \
    case PTV: {                                                                                                    \
        RML_MAX_DYN_LDS(160 * 1024, &k_svm_gemm_ring<PTV, DIG>);                                                   \
        hipLaunchKernelGGL((k_svm_gemm_ring<PTV, DIG>), grid, block, lds, st, ra);                                 \
    } break;
    switch (m->PT) {
        RML_RING_CASE(1)
        RML_RING_CASE(3)
        RML_RING_CASE(6)
        default: RML_REQUIRE(false, RML_ERR_UNSUPPORTED, "svm: unsupported pair count for the 256x256 kernel");
    }
#undef RML_RING_CASE
    RML_HIP(hipGetLastError());
    return RML_OK;
}

}  // namespace
