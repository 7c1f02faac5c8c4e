// The split-fp16 operand machinery of K1 (dual_softmax_f16s.hip), shared with the Sinkhorn matcher (sinkhorn_f16s.hip):
//   k1_prep      feat -> fp16 hi / lo planes, scaled by 2^4, stored in the LDS image ([rows][256] fp16, 16-byte
//                slot ^= row & 15) so that a 64-row tile is one linear LDS-DMA
//   RowFrags     a lane's row of both planes in registers
//   dma_tile     one 64-row tile of both planes into LDS
//   score_tile   three v_mfma_f32_32x32x16_f16 per 16 channels (hi.hi + hi.lo + lo.hi, fp32 accumulate)
// Each including file gets its own copy in its anonymous namespace (one translation unit per .hip file).
// The training files include k1_train_f16s.h, which adds the 32-column gradient tile, its prep kernel and the dense focal loss's
// shared pieces on top of this header.  The library-internal functions through which they reach the two matchers (far_k1_*,
// far_skh_history_launch) are declared at the end of this file, which their defining files include as well.
#pragma once
#include "dual_softmax_common.h"

namespace {

using namespace far_ds;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int C = 256;               // channels (the FAR coarse level)
constexpr int NS = C / 16;           // MFMA k-steps
constexpr int KT = 64;               // columns per tile
constexpr int ROWB = C * 2;          // bytes per fp16 row
constexpr float PRESCALE = 16.0f;
constexpr float HUGE_F = 1.0e30f;
constexpr int TILE_PLANE = KT * ROWB;   // 32 KiB

__device__ __forceinline__ void split1(float x, _Float16& hi, _Float16& lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}

// x [Z][N][256] fp32 -> hi / lo [Z][Np][256] fp16 (rows >= N zero), slot ^= row & 15
// overflow (device int or null): |= 1 when a feature is beyond the range of the 2^4-scaled split (|x| > 4094: hi = inf)
// nmax (device uint or null): atomic maximum of the bit pattern of max_rows sum_c (2^4 x)^2 -- the squared norm bound of the match
// pass's tile prescreen (non-negative floats order like unsigned integers); the caller zeroes it.
__global__ void k1_prep(const float* __restrict__ x, int Z, int N, int Np, _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                        int* __restrict__ overflow, unsigned* __restrict__ nmax) {
    const long total = (long)Z * Np * 32;
    bool bad = false;
    float n2max = 0.f;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int slot = (int)(t & 31);
        const long row = t >> 5;
        const unsigned urow = (unsigned)row, uz = urow / (unsigned)Np;      // Z Np < 2^31 (host check): 32-bit division
        const int i = (int)(urow - uz * (unsigned)Np);
        const long z = uz;
        f16x8 vh, vl;
        if (i < N) {
            const float* src = x + ((size_t)z * N + i) * C + slot * 8;
            const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
            const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                _Float16 h, l;
                split1(v[e] * PRESCALE, h, l);
                vh[e] = h; vl[e] = l;
                bad |= !(fabsf(v[e]) <= 65504.0f / PRESCALE);          // also true for NaN inputs
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) { vh[e] = (_Float16)0.f; vl[e] = (_Float16)0.f; }
        }
        const int s2 = slot ^ (i & 15);
        *reinterpret_cast<f16x8*>(hi + (size_t)row * C + s2 * 8) = vh;
        *reinterpret_cast<f16x8*>(lo + (size_t)row * C + s2 * 8) = vl;
        if (nmax) {                                  // the row's 32 slots are the 32 lanes of a half-wave (total is a multiple of 32)
            float n2 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float q = (float)vh[e] + (float)vl[e]; n2 = fmaf(q, q, n2); }
#pragma unroll
            for (int m = 1; m < 32; m <<= 1) n2 += shfl_xor_f(n2, m);
            n2max = fmaxf(n2max, n2);
        }
    }
    if (nmax) {
        n2max = fmaxf(n2max, shfl_xor_f(n2max, 32));
        // one atomic per wave on one address would serialise 78 k of them in L2 (0.8 ms): only a wave that can still raise the
        // maximum issues it (the plain read may be stale -- then the atomic is merely redundant; the maximum only grows)
        if ((threadIdx.x & 63) == 0 && n2max > __uint_as_float(*reinterpret_cast<volatile unsigned*>(nmax))) atomicMax(nmax, __float_as_uint(n2max));
    }
    if (overflow && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(overflow, 1);
}

// Row-side fragments: row i, channels 16 s + 8 h .. + 7, both planes (128 registers)
struct RowFrags {
    f16x8 hi[NS], lo[NS];
    __device__ __forceinline__ void load(const _Float16* ph, const _Float16* pl, size_t row, int irow, int h) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int slot = (2 * s + h) ^ (irow & 15);
            hi[s] = *reinterpret_cast<const f16x8*>(ph + row * C + 8 * slot);
            lo[s] = *reinterpret_cast<const f16x8*>(pl + row * C + 8 * slot);
        }
    }
};

__device__ __forceinline__ void dma_tile(unsigned char* lds, const _Float16* gh, const _Float16* gl, size_t row0, int tid, int wave) {
    const unsigned char* sh = reinterpret_cast<const unsigned char*>(gh + row0 * C) + tid * 16;
    const unsigned char* sl = reinterpret_cast<const unsigned char*>(gl + row0 * C) + tid * 16;
#pragma unroll
    for (int j = 0; j < TILE_PLANE / 4096; ++j) {
        __builtin_amdgcn_global_load_lds((gptr_t)(sh + j * 4096), (lptr_t)(lds + j * 4096 + wave * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(sl + j * 4096), (lptr_t)(lds + TILE_PLANE + j * 4096 + wave * 1024), 16, 0, 0);
    }
}

// acc[ct]: D[m = tile row 32 ct + ..][n = this lane's row]
__device__ __forceinline__ void score_tile(f32x16 (&acc)[2], const unsigned char* lds, const RowFrags& rf, int l31, int h) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        f16x8 ch[2], cl[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int row = 32 * ct + l31;
            const int off = row * ROWB + (((2 * s + h) ^ (row & 15)) * 16);
            ch[ct] = *reinterpret_cast<const f16x8*>(lds + off);
            cl[ct] = *reinterpret_cast<const f16x8*>(lds + TILE_PLANE + off);
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], rf.hi[s], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[ct], rf.lo[s], acc[ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl[ct], rf.hi[s], acc[ct], 0, 0, 0);
    }
}

}  // namespace

// ---- library-internal glue between the matchers and the training files (not part of the C ABI) ----
// dual_softmax_f16s.hip -> dual_softmax_bwd_f16.hip, dual_softmax_dense_f16s.hip: the forward workspace (the training workspaces begin
// behind it), its statistics passes (operand planes + row statistics + dense column statistics, as far_coarse_match_f16s prepares them;
// masked: with optional padded masks (Z, L) / (Z, S)), and views of what they left: the hi planes with the column (max, 1 / sum) of the
// sparse form (c1 is set by the caller), or all four planes with the (max, sum) statistics of both axes
size_t far_k1_fwd_ws_bytes(int Z, int L, int S);
int far_k1_stats_launch(const float* f0, const float* f1, int Z, int L, int S, float temperature, void* ws, int* overflow,
                        hipStream_t stream);
int far_k1_stats_launch_masked(const float* f0, const float* f1, int Z, int L, int S, float temperature, const uint8_t* mask0,
                               const uint8_t* mask1, void* ws, int* overflow, hipStream_t stream);
void far_k1_fwd_views(void* ws, int Z, int L, int S, const _Float16** ah, const _Float16** bh, const float2** rowstat,
                      const float** cmax, const float** cinv, float* c1);
void far_k1_fwd_planes(void* ws, int Z, int L, int S, const _Float16** ah, const _Float16** al, const _Float16** bh,
                       const _Float16** bl, const float2** rowstat, const float2** colstat);

// sinkhorn_f16s.hip -> sinkhorn_train_f16s.hip (library-internal, not part of the C ABI): the matcher's operand preparation and its T
// iterations (the same k_skh_stats launches: the bits of inference) with every (u^t, v^t) kept.  uh [(T+1)][Z][Lp], vh [(T+1)][Z][Sp],
// binh [(T+1)][2][Z] (U_L, V_S) in log2 units; slice 0 is u = v = 0
int far_skh_history_launch(const float* f0, const float* f1, int Z, int L, int S, const float* bin_score, int iters,
                           const uint8_t* mask0, const uint8_t* mask1, _Float16* ah, _Float16* al, _Float16* bh, _Float16* bl,
                           float* uh, float* vh, float* binh, int* overflow, hipStream_t stream);
