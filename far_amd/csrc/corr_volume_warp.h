// K12's tile recipe and its two forward kernels, shared by corr_volume_warp_f32.hip (inference) and corr_volume_warp_bwd_f32.hip
// (training forward + backward).  See corr_volume_warp_f32.hip for the operator and the operand layouts.
#pragma once
#include "common.h"

namespace {

constexpr int D = 32;                 // feature channels (ENCODER.NUM_OUT_LAYERS)
constexpr int KT = 32;                // columns per tile
constexpr int LROW = KT + 1;          // padded LDS row (floats)
constexpr float LOG2E = 1.44269504088896341f;
constexpr float NEG_HUGE = -1.0e30f;

// stage vol1[b][0..31][j0 .. j0+31] -> lds[ch][LROW] (zeros past HW), grid[0..1][j0..] -> gl[2][KT]
__device__ __forceinline__ void stage_tile(float* lds, float* gl, const float* __restrict__ v1, const float* __restrict__ grid,
                                           int HW, int j0, int tid) {
    for (int e = tid; e < D * KT; e += 256) {
        const int ch = e >> 5, c = e & 31;
        lds[ch * LROW + c] = j0 + c < HW ? v1[(size_t)ch * HW + j0 + c] : 0.f;
    }
    if (tid < 2 * KT) {
        const int g = tid >> 5, c = tid & 31;
        gl[g * KT + c] = j0 + c < HW ? grid[(size_t)g * HW + j0 + c] : 0.f;
    }
}

// scores of one 32 x 32 tile, transposed: D[m = column][n = this lane's row]
__device__ __forceinline__ void score_tile(f32x16& sc, const float* lds, const float (&q)[16], int l31, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[(2 * t + h) * LROW + l31], q[t], sc, 0, 0, 0);
}

// ARG (the training forward): also the row's arg-max column j*, lowest index among equal scores (torch's rule for max(dim) on the CPU);
// the maximum and the sum are the same instructions in both instantiations.
template <bool ARG>
__global__ __launch_bounds__(256) void k_cvw_stats(const float* __restrict__ vol0, const float* __restrict__ vol1, int B, int HW,
                                                   float2* __restrict__ stat, int* __restrict__ jstar) {
    __shared__ float lds[D * LROW];
    __shared__ float gl[2 * KT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int nI = (HW + 127) / 128;
    const int b = blockIdx.x / nI, Ib = blockIdx.x - b * nI;
    const int row = Ib * 128 + 32 * wave + l31;
    const float* v0 = vol0 + (size_t)b * D * HW;
    const float* v1 = vol1 + (size_t)b * D * HW;
    float q[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) q[t] = row < HW ? v0[(size_t)(2 * t + h) * HW + row] : 0.f;
    float m = NEG_HUGE, s = 0.f;
    float bv = NEG_HUGE;
    int bi = 0x7fffffff;
    for (int j0 = 0; j0 < HW; j0 += KT) {
        __syncthreads();
        stage_tile(lds, gl, v1, vol1, HW, j0, tid);          // (grid staging unused here: harmless reads of vol1)
        __syncthreads();
        f32x16 sc;
        score_tile(sc, lds, q, l31, h);
        float tm = NEG_HUGE;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + mfma32_row(r, h);
            if (ARG) {                                       // index compared on equal values: within the lane and across tiles
                const float raw = sc[r];
                if (j < HW && (raw > bv || (raw == bv && j < bi))) { bv = raw; bi = j; }
            }
            float x = sc[r] * LOG2E;
            if (j >= HW) x = NEG_HUGE;
            sc[r] = x;
            tm = fmaxf(tm, x);
        }
        const float mn = fmaxf(m, tm);
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += __builtin_amdgcn_exp2f(sc[r] - mn);
        s = s * __builtin_amdgcn_exp2f(m - mn) + t;
        m = mn;
    }
    const float mo = shfl_xor_f(m, 32), so = shfl_xor_f(s, 32);
    const float mn = fmaxf(m, mo);
    const float st = s * __builtin_amdgcn_exp2f(m - mn) + so * __builtin_amdgcn_exp2f(mo - mn);
    if (h == 0 && row < HW) stat[(size_t)b * HW + row] = make_float2(mn, st);
    if (ARG) {                                               // the two half-waves hold disjoint columns of the same row
        const float ov = shfl_xor_f(bv, 32);
        const int oi = shfl_xor_i(bi, 32);
        if (ov > bv || (ov == bv && oi < bi)) bi = oi;
        if (h == 0 && row < HW) jstar[(size_t)b * HW + row] = bi;
    }
}

__global__ __launch_bounds__(256) void k_cvw_apply(const float* __restrict__ vol0, const float* __restrict__ vol1,
                                                   const float* __restrict__ grid, const float2* __restrict__ stat, int B, int HW,
                                                   float* __restrict__ agg) {
    __shared__ float lds[D * LROW];
    __shared__ float gl[2 * KT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int nI = (HW + 127) / 128;
    const int b = blockIdx.x / nI, Ib = blockIdx.x - b * nI;
    const int row = Ib * 128 + 32 * wave + l31;
    const float* v0 = vol0 + (size_t)b * D * HW;
    const float* v1 = vol1 + (size_t)b * D * HW;
    float q[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) q[t] = row < HW ? v0[(size_t)(2 * t + h) * HW + row] : 0.f;
    const float2 st = row < HW ? stat[(size_t)b * HW + row] : make_float2(0.f, 1.f);
    const float rinv = 1.0f / st.y;
    f32x16 acc;                                          // D[m = channel][n = row]
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float pu = 0.f, pv = 0.f;
    for (int j0 = 0; j0 < HW; j0 += KT) {
        __syncthreads();
        stage_tile(lds, gl, v1, grid, HW, j0, tid);
        __syncthreads();
        f32x16 sc;
        score_tile(sc, lds, q, l31, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = mfma32_row(r, h);
            float p = __builtin_amdgcn_exp2f(sc[r] * LOG2E - st.x) * rinv;
            if (j0 + c >= HW) p = 0.f;
            sc[r] = p;
            pu = fmaf(p, gl[c], pu);
            pv = fmaf(p, gl[KT + c], pv);
        }
        // vol1w^T[ch][row] += sum_col vol1[ch][col] p[row][col]: k-slot h of step r = column mfma32_row(r, h)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[l31 * LROW + mfma32_row(r, h)], sc[r], acc, 0, 0, 0);
    }
    pu += shfl_xor_f(pu, 32);
    pv += shfl_xor_f(pv, 32);
    if (row < HW) {
        float* o = agg + (size_t)b * (2 * D + 3) * HW + row;
        // lane (row, h) holds channels mfma32_row(r, h): per register 32 consecutive rows of one channel = 128 B per half-wave
#pragma unroll
        for (int r = 0; r < 16; ++r) o[(size_t)(D + mfma32_row(r, h)) * HW] = acc[r];
#pragma unroll
        for (int t = 0; t < 16; ++t) o[(size_t)(2 * t + h) * HW] = q[t];           // the vol0 block of the concatenation
        if (h == 0) {
            o[(size_t)(2 * D) * HW] = pu;
            o[(size_t)(2 * D + 1) * HW] = pv;
            o[(size_t)(2 * D + 2) * HW] = rinv;                                     // max_j softmax = 2^(max - max) / sum
        }
    }
}

}  // namespace
