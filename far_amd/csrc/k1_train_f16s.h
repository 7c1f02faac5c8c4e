// What the three training files of the coarse matcher share on top of k1_f16s.h -- dual_softmax_bwd_f16.hip (sparse dual-softmax),
// dual_softmax_dense_f16s.hip (dense dual-softmax focal) and sinkhorn_train_f16s.hip (sparse and dense optimal transport):
//   GT, PLANE32, TROW, TILE_T   the 32-column gradient tile: a row-major plane tile (the LDS image of k1_prep) for the score
//                               recompute, a channel-major "transposed" tile as the B operand of the second MFMA (G F)
//   k1_prep_t                   feat -> transposed fp16 tiles, columns in the order in which the accumulator registers hold G
//   dma_lin                     a linear piece of global memory into LDS (LDS-DMA: far_amd/build.py lists this header in LDS_DMA_HEADERS)
//   score_step, _x, _both       one 16-channel step of a 32 x 32 split-fp16 score in either order of its cross terms, or in both
//   grad_scale_exp              the power of two that brings a device maximum under a given head-room
//   FocalK, make_plan, k1_focal_loss   the dense focal loss's constants, normalisers and final reduction.  The dense forms rely on one
//                               expression giving the same bits in the loss pass, the labels' correction and the gradient kernel:
//                               the clamp's range and its constants exist here only
//   pad128, gridp, Carver       host helpers
// Each including file gets its own copy in its anonymous namespace, as with k1_f16s.h.
#pragma once
#include "k1_f16s.h"
#include <cmath>

namespace {

constexpr int GT = 32;                   // columns per tile of the gradient kernels and the dense loss passes
constexpr int PLANE32 = GT * ROWB;       // 16 KiB: one row-major (swizzled) plane of a tile
constexpr int TROW = 80;                 // bytes per channel row of a transposed tile: 32 positions x 2 B + 16 B pad
constexpr int TILE_T = C * TROW;         // 20 KiB

// x [Z][N][256] fp32 -> transposed fp16 tiles [Z][Np / 32][256 ch][TROW], value * 2^4; rows >= N zero, and with a mask the MASKED rows
// as well (a masked row may hold anything, also non-finite values).  Position p = 8 q + e of a channel row holds the tile's column
// 16 u + 4 h + (e & 3) + 8 (e >> 2), u = q >> 1, h = q & 1: MFMA step u takes, from lane half h, the eight accumulator registers
// r = 8 u + e, and those are the columns they hold (as K2 does for P v).
__global__ void k1_prep_t(const float* __restrict__ x, int Z, int N, int Np, const uint8_t* __restrict__ mask,
                          unsigned char* __restrict__ out) {
    const long total = (long)Z * (Np / GT) * C * 4;                       // one thread = 8 positions of one channel row
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int q = (int)(t & 3);
        const int ch = (int)((t >> 2) & (C - 1));
        const long zt = t >> 10;                                          // z * ntile + tile
        const int ntile = Np / GT;
        const int jt = (int)(zt % ntile);
        const long z = zt / ntile;
        f16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 16 * (q >> 1) + 4 * (q & 1) + (e & 3) + 8 * (e >> 2);
            const int i = jt * GT + c;
            const bool ok = i < N && !(mask && !mask[(size_t)z * N + i]);
            v[e] = ok ? (_Float16)(x[((size_t)z * N + i) * C + ch] * PRESCALE) : (_Float16)0.f;
        }
        *reinterpret_cast<f16x8*>(out + (size_t)zt * TILE_T + ch * TROW + q * 16) = v;
    }
}

__device__ __forceinline__ void dma_lin(unsigned char* lds, const unsigned char* g, int bytes, int tid, int wave) {
    for (int o = 0; o < bytes; o += 4096)
        __builtin_amdgcn_global_load_lds((gptr_t)(g + o + tid * 16), (lptr_t)(lds + o + wave * 1024), 16, 0, 0);
}

// One 16-channel step of a 32 x 32 score (tile side ch / cl, row side rh / rl; fp32 accumulate) in the two orders in which the
// statistics passes sum its terms: score_step is score_tile's hi.hi + hi.lo + lo.hi, score_step_x the order the same entry has in
// the launch with the maps' roles swapped, hi.hi + lo.hi + hi.lo.  Only the score a statistic was summed FROM cancels against it.
__device__ __forceinline__ void score_step(f32x16& sc, f16x8 ch, f16x8 cl, f16x8 rh, f16x8 rl) {
    sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rh, sc, 0, 0, 0);
    sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rl, sc, 0, 0, 0);
    sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl, rh, sc, 0, 0, 0);
}
__device__ __forceinline__ void score_step_x(f32x16& sx, f16x8 ch, f16x8 cl, f16x8 rh, f16x8 rl) {
    sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rh, sx, 0, 0, 0);
    sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl, rh, sx, 0, 0, 0);
    sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rl, sx, 0, 0, 0);
}
// both at once, interleaved (the dense dual-softmax passes: R meets sc, C meets sx)
__device__ __forceinline__ void score_step_both(f32x16& sc, f32x16& sx, f16x8 ch, f16x8 cl, f16x8 rh, f16x8 rl) {
    sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rh, sc, 0, 0, 0);
    sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rh, sx, 0, 0, 0);
    sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rl, sc, 0, 0, 0);
    sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl, rh, sx, 0, 0, 0);
    sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl, rh, sc, 0, 0, 0);
    sx = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch, rl, sx, 0, 0, 0);
}

// The exponent e of the power of two that scales gradient weights for an fp16 tile: 2^headroom * max * 2^e lies in [1/2, 1), max being
// the non-negative float whose bits a device maximum holds (e = 0 while it is 0).  Each caller names its head-room and keeps its own
// clamp of e.
__device__ __forceinline__ int grad_scale_exp(const unsigned* max_bits, int headroom) {
    const float mx = __uint_as_float(*max_bits);
    int e = 0;
    if (mx > 0.f) { (void)frexpf(mx, &e); e = -(e + headroom); }
    return e;
}

// ---- dense focal supervision (loftr_loss.py:56-75): the loss reads q = clamp(p, 1e-6, 1 - 1e-6)
constexpr float P_LO = 1e-6f;
constexpr float P_HI = (float)(1.0 - 1e-6);

struct FocalK {
    float alpha, gamma, cneg;              // cneg = neg_weight / (N L S - #positives)
    double c_lo, c_hi;                     // the negative term of an entry clamped from below / from above
};
struct FocalPlan {
    FocalK fk;
    double cpos;                           // pos_weight / #positives
};
// the normalisers of a call (loftr_loss.py:63-70: without ground truth the positive term has weight 0 and every entry is a negative)
inline FocalPlan make_plan(int Z, int L, int S, int M, float alpha, float gamma, float pos_weight, float neg_weight, int no_gt) {
    FocalPlan pl;
    const long npos = no_gt ? 0 : M;
    const double nneg = (double)Z * (double)L * (double)S - (double)npos;
    pl.fk.alpha = alpha;
    pl.fk.gamma = gamma;
    pl.fk.cneg = nneg > 0 ? (float)((double)neg_weight / nneg) : 0.f;
    pl.fk.c_lo = -(double)alpha * pow(1e-6, (double)gamma) * log1p(-1e-6);
    pl.fk.c_hi = -(double)alpha * pow(1.0 - 1e-6, (double)gamma) * log(1e-6);
    pl.cpos = npos > 0 ? (double)pos_weight / (double)npos : 0.0;
    return pl;
}

// loss = cneg * sum of the workgroups' partials + sum of the labels' corrections: one workgroup, a fixed order
__global__ __launch_bounds__(256) void k1_focal_loss(const double* __restrict__ lossp, int nparts, const double* __restrict__ dl, int M,
                                                     double cneg, float* __restrict__ loss_out) {
    __shared__ double sh[256];
    double a = 0.0, b = 0.0;
    for (int t = threadIdx.x; t < nparts; t += 256) a += lossp[t];
    for (int t = threadIdx.x; t < M; t += 256) b += dl[t];
    sh[threadIdx.x] = cneg * a + b;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[0] = (float)sh[0];
}

// ---- host helpers
inline int pad128(int n) { return (n + 127) / 128 * 128; }           // rows of the operand planes: whole 128-row workgroups

inline unsigned gridp(long n) { long g = (n + 255) / 256; return (unsigned)(g < 16384 ? (g > 0 ? g : 1) : 16384); }

// hands out 256-byte-aligned pieces of a workspace from offset o on; with a null base only the sizes are counted
struct Carver {
    unsigned char* p;
    size_t o;
    template <class T = unsigned char>
    T* take(size_t bytes) {
        T* r = p ? reinterpret_cast<T*>(p + o) : nullptr;
        o += align256(bytes);
        return r;
    }
};

}  // namespace
