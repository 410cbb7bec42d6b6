// The 128 x 128 staged MFMA tile.  Who uses what:
//   k_svm_gemm<PATH_I8 / PATH_F32> (svm_tile.h)   TileStager or SparseStager, tile_k_loop, Frag32, kstep_32
//   k_svm_gemm<PATH_F64> (svm_tile.h)             TileStager, tile_k_loop, Frag64, kstep_f64
//   k_svm_gemm_splitk (svm_tile.h)                TileStager, tile_k_loop over its K range, Frag32, kstep_i8_plain
//   k_gram, k_gseg (gram.hip: gram_tile)          TileStager (no clamp), tile_k_loop over a segment's K range, Frag64, kstep_f64
//   k_svm_gemm_ring (svm_ring.h, 256 x 256)       glds16, stage_src and the C/D map; it keeps its own schedule
//
// Workgroup tile 128 rows of A x 128 rows of B, 4 waves as 2 x 2.  K-step = 128 bytes per row (128 codes or 32 floats).  LDS image
// of an operand tile: row-major [128 rows][128 B] with the 16-byte chunk index XOR-swizzled by (row >> 1) & 7, which makes the
// ds_read_b128 fragment reads (lane = row, 16 B each) bank-conflict free.  LDS-DMA writes lane-linear, so the swizzle is applied
// to the per-lane GLOBAL source address and again on the read (both-sides rule).  Two stages of (A image, B image): the DMA of
// K-step t+1 is in flight while the MFMAs of K-step t run.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kTile = 128;                          // rows per operand tile
constexpr int kStepBytes = 128;                     // K-step bytes per row
constexpr int kTileBytes = kTile * kStepBytes;      // 16 KiB
constexpr int PATH_I8 = 0, PATH_F32 = 1, PATH_F64 = 2;

__device__ __forceinline__ void glds16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// Global source of this lane's 16 bytes of wave-instruction q (of 4 per wave; 1 KiB each) of an operand stage whose first row is
// row0: LDS slot s holds chunk (s & 7) ^ swizzle of row s >> 3.  CLAMP: rows at or past `rows` read row rows - 1.
template <bool CLAMP>
__device__ __forceinline__ const uint8_t* stage_src(const uint8_t* base, int64_t ld, int64_t row0, int64_t rows, int wave, int q, int lane) {
    const int s = (wave * 4 + q) * 64 + lane;       // 16-byte slot in the LDS image
    const int r = s >> 3;
    const int c = (s & 7) ^ ((r >> 1) & 7);         // inverse swizzle on the source
    int64_t gr = row0 + r;
    if (CLAMP) gr = gr < rows ? gr : rows - 1;
    return base + gr * ld + c * 16;
}

// staging of the two operand tiles: 16 wave-instructions of 1 KiB per tile, 4 per wave
struct TileStager {
    const uint8_t* ga[4];
    const uint8_t* gb[4];
    int wave;
    template <bool CLAMP_B>
    __device__ __forceinline__ void init(const uint8_t* a, int64_t lda, int64_t a0, const uint8_t* b, int64_t ldb, int64_t b0, int64_t b_rows,
                                         int wave_, int lane) {
        wave = wave_;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ga[q] = stage_src<false>(a, lda, a0, 0, wave, q, lane);
            gb[q] = stage_src<CLAMP_B>(b, ldb, b0, b_rows, wave, q, lane);
        }
    }
    __device__ __forceinline__ void take(int) {}    // nothing per block of 32 K-steps (SparseStager has)
    __device__ __forceinline__ void stage(unsigned char* smem, int kt, int buf) const {
        unsigned char* base = smem + buf * 2 * kTileBytes;
        const int64_t ko = (int64_t)kt * kStepBytes;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            glds16(ga[q] + ko, base + (wave * 4 + q) * 1024);
            glds16(gb[q] + ko, base + kTileBytes + (wave * 4 + q) * 1024);
        }
    }
};

// Staging that honours occupancy words (k_svm_gemm<PATH_I8, PT, false, true> only).  Radar code rows are mostly the background code:
// about two thirds of the 128-byte lines of a 64x64x128 row hold nothing else (tools/exp/README.md, "sparse code rows").  Every row
// has one bit per K-step (= one line), packed into `ow` dwords: 1 unless the line is all 0x80 and wholly inside D.  For a clear bit
// the lane issues the SAME global_load_lds from a 128-byte line of 0x80 that stays in L1 / L2 (rml_ctx::bg_line) instead of from its
// row: the same bytes reach LDS, so the MFMAs run on identical operands -- every accumulator is bit-identical to the dense stager's --
// and the instruction count, the LDS addresses, the swizzle and the vmcnt accounting are unchanged; nothing is exec-masked.
// The eight lanes of a row share its bit.  The words of the tile's 256 rows wait in LDS ([256][ow] dwords behind the epilogue
// tables, filled once per tile); a lane takes the words of its eight rows from there once per 32 K-steps.  (Words kept in registers
// one block ahead: hipcc loads them into temporaries and copies them into the loop-carried set behind a vmcnt wait at every block
// boundary -- a memory latency per 32 steps with the DMA queue drained.)
constexpr int kSparseMaxWords = 8;                  // ow <= 8 (K <= 32 768 codes): 8 KiB of LDS for the words
struct SparseStager {
    const uint8_t* ga[4];
    const uint8_t* gb[4];
    const uint8_t* bg;                              // this lane's 16 bytes of the background line (every chunk of it is the same)
    const uint32_t* la;                             // LDS: the words of the lane's first A row; row q is 8 rows on, B rows 128 rows on
    uint32_t ca[4], cb[4];                          // the words in use, shifted so that bit 0 is the next step's
    int wave, ow;
    // the tile's words into LDS: thread t < 128 owns A row a0 + t, thread t >= 128 B row b0 + t - 128 (clamped like the row itself);
    // the caller's barrier makes them visible
    static __device__ __forceinline__ void fill(uint32_t* occ_l, const uint32_t* a_occ, int64_t a0, const uint32_t* b_occ, int64_t b0,
                                                int64_t b_rows, int ow, int tid) {
        int64_t gr = b0 + (tid - kTile);
        gr = gr < b_rows ? gr : b_rows - 1;
        const uint32_t* src = tid < kTile ? a_occ + (a0 + tid) * ow : b_occ + gr * ow;
        for (int w = 0; w < ow; ++w) occ_l[tid * ow + w] = src[w];
    }
    __device__ __forceinline__ void init(const uint8_t* a, int64_t lda, int64_t a0, const uint8_t* b, int64_t ldb, int64_t b0, int64_t b_rows,
                                         const uint32_t* occ_l, int ow_, const uint8_t* bg_line, int wave_, int lane) {
        wave = wave_; ow = ow_;
        bg = bg_line + (lane & 7) * 16;
        la = occ_l + (((wave * 4) * 64 + lane) >> 3) * ow;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ga[q] = stage_src<false>(a, lda, a0, 0, wave, q, lane);
            gb[q] = stage_src<true>(b, ldb, b0, b_rows, wave, q, lane);
        }
    }
    // the words of K-steps [32 blk, 32 blk + 32)
    __device__ __forceinline__ void take(int blk) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ca[q] = la[q * 8 * ow + blk];
            cb[q] = la[(kTile + q * 8) * ow + blk];
        }
    }
    // stage K-step kt (bit 0 of the words in use) and move on to the next bit
    __device__ __forceinline__ void stage(unsigned char* smem, int kt, int buf) {
        unsigned char* base = smem + buf * 2 * kTileBytes;
        const int64_t ko = (int64_t)kt * kStepBytes;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            glds16((ca[q] & 1u) ? ga[q] + ko : bg, base + (wave * 4 + q) * 1024);
            glds16((cb[q] & 1u) ? gb[q] + ko : bg, base + kTileBytes + (wave * 4 + q) * 1024);
            ca[q] >>= 1; cb[q] >>= 1;
        }
    }
};

// The double-buffered K loop over steps [kt0, kt1) with either stager: kstep(sA, sB) consumes one staged step.  The stager is told
// (take) which block of 32 K-steps the next staged step opens; SparseStager's words start at bit 0, so its kt0 is a multiple of 32.
template <class Stager, class KStep>
__device__ __forceinline__ void tile_k_loop(Stager& sg, unsigned char* smem, int kt0, int kt1, KStep kstep) {
    sg.take(kt0 >> 5);
    sg.stage(smem, kt0, 0);
    for (int kt = kt0; kt < kt1; ++kt) {
        __syncthreads();                            // DMA of step kt landed (vmcnt(0)) and visible; step kt-1's buffer is free
        if (kt + 1 < kt1) {
            if (((kt + 1) & 31) == 0) sg.take((kt + 1) >> 5);      // the next step opens a block of 32
            sg.stage(smem, kt + 1, (kt + 1 - kt0) & 1);
        }
        const unsigned char* sA = smem + ((kt - kt0) & 1) * 2 * kTileBytes;
        kstep(sA, sA + kTileBytes);
    }
}

// fragment read offsets (bytes within a tile image) of the 32-row MFMAs; lane = row, swizzled chunk; T tiles of 32 rows from row0
template <int T>
struct Frag32 {
    int off[T], sw[T];
    __device__ __forceinline__ void init(int row0, int lane) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int r = row0 + t * 32 + (lane & 31);
            off[t] = r * kStepBytes; sw[t] = (r >> 1) & 7;
        }
    }
    __device__ __forceinline__ v4i read(const unsigned char* img, int t, int ch) const {
        return *reinterpret_cast<const v4i*>(img + off[t] + ((ch ^ sw[t]) << 4));
    }
};

// ... and of the 16-row f64 MFMA: lane = (row l & 15, k-group l >> 4) of a 16-row tile; 4 tiles from row0
struct Frag64 {
    int off[4], sw[4];
    __device__ __forceinline__ void init(int row0, int lane) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int r = row0 + t * 16 + (lane & 15);
            off[t] = r * kStepBytes; sw[t] = (r >> 1) & 7;
        }
    }
    __device__ __forceinline__ v4f read(const unsigned char* img, int t, int ch) const {
        return *reinterpret_cast<const v4f*>(img + off[t] + ((ch ^ sw[t]) << 4));
    }
};

// C/D maps: which (row of A, row of B) register r of a lane holds, for the accumulator tile at (row0, col0).
// 32x32 int32 / f32 accumulator (16 registers): row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column = lane & 31
__device__ __forceinline__ int cd32_row(int row0, int r, int lane) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ int cd32_col(int col0, int lane) { return col0 + (lane & 31); }
// 16x16 f64 accumulator (4 registers): row = (lane >> 4) + 4 r, column = lane & 15
__device__ __forceinline__ int cd64_row(int row0, int r, int lane) { return row0 + (lane >> 4) + 4 * r; }
__device__ __forceinline__ int cd64_col(int col0, int lane) { return col0 + (lane & 15); }

// kstep_i8 / kstep_f32 = kstep_32<PATH_I8 / PATH_F32>: one K-step of the wave tile (2 x 2 MFMA tiles of 32 x 32).
// Software-pipelined fragments: the ds_read_b128 of sub-step kk+1 are in flight while the MFMAs of kk run (two register sets + sched_barrier; left alone hipcc reuses one set and waits
// lgkmcnt(0) every 4 MFMAs).
template <int PATH, class Acc>
__device__ __forceinline__ void kstep_32(Acc (&acc)[2][2], const unsigned char* sA, const unsigned char* sB, const Frag32<2>& fa,
                                         const Frag32<2>& fb, int chalf) {
    v4i af[2][2], bf[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        af[0][t] = fa.read(sA, t, chalf);
        bf[0][t] = fb.read(sB, t, chalf);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        if (kk < 3) {
            const int ch = 2 * (kk + 1) + chalf;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                af[(kk + 1) & 1][t] = fa.read(sA, t, ch);
                bf[(kk + 1) & 1][t] = fb.read(sB, t, ch);
            }
        }
        __builtin_amdgcn_sched_barrier(0);          // keep the prefetch ahead of this sub-step's MFMAs
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (PATH == PATH_I8) {
                    acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[kk & 1][i], bf[kk & 1][j], acc[i][j], 0, 0, 0);
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__int_as_float(af[kk & 1][i][c]),
                                                                        __int_as_float(bf[kk & 1][j][c]), acc[i][j], 0, 0, 0);
                }
            }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The same K-step with one fragment set and no scheduling fences: what the split-K kernel runs (its ranges are a few steps long).
__device__ __forceinline__ void kstep_i8_plain(v16i (&acc)[2][2], const unsigned char* sA, const unsigned char* sB, const Frag32<2>& fa,
                                               const Frag32<2>& fb, int chalf) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int ch = 2 * kk + chalf;
        v4i af[2], bf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            af[t] = fa.read(sA, t, ch);
            bf[t] = fb.read(sB, t, ch);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
}

// One K-step of the f64 wave tile (4 x 4 MFMA tiles of 16 x 16): 32 floats per row per K-step = 8 chunks of 4; pass h covers
// chunks 4h..4h+3, one per k-group; MFMA c of a pass multiplies element c of every lane's chunk (k = 4*chunk + c), widened to
// float64 in registers.
__device__ __forceinline__ void kstep_f64(v4d (&acc)[4][4], const unsigned char* sA, const unsigned char* sB, const Frag64& fa,
                                          const Frag64& fb, int kgrp) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const int ch = 4 * hh + kgrp;
        v4f af[4], bf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            af[t] = fa.read(sA, t, ch);
            bf[t] = fb.read(sB, t, ch);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double ad[4], bd[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { ad[t] = (double)af[t][c]; bd[t] = (double)bf[t][c]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[i], bd[j], acc[i][j], 0, 0, 0);
        }
    }
}



template <class V, int R, int C>
__device__ __forceinline__ void zero_acc(V (&acc)[R][C]) {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int r = 0; r < (int)(sizeof(V) / sizeof(acc[0][0][0])); ++r) acc[i][j][r] = 0;
}

}  // namespace
