// The 128 x 128 staged MFMA tile shared by k_svm_gemm, k_svm_gemm_splitk (svm_tile.h) and k_gram (gram.hip); the 256 x 256 ring
// kernel (svm_ring.h) takes glds16, the source addresses and the C/D map from here and keeps its own schedule.
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

// The double-buffered K loop over steps [kt0, kt1): kstep(sA, sB) consumes one staged step.
template <class KStep>
__device__ __forceinline__ void tile_k_loop(const TileStager& sg, unsigned char* smem, int kt0, int kt1, KStep kstep) {
    sg.stage(smem, kt0, 0);
    for (int kt = kt0; kt < kt1; ++kt) {
        __syncthreads();                            // DMA of step kt landed (vmcnt(0)) and visible; step kt-1's buffer is free
        if (kt + 1 < kt1) sg.stage(smem, kt + 1, (kt + 1 - kt0) & 1);
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
