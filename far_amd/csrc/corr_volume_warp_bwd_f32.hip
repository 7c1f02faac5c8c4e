// K12 training: the forward that keeps the row statistics, and the gradient of the correlation-volume warp.
//
// With x_ij = vol0[:, i] . vol1[:, j], p_ij = softmax_j(x_ij) and the forward output (corr_volume_warp_f32.hip)
//     agg = cat[ a_i = vol0[:, i] | w_i = sum_j p_ij vol1[:, j] | e_i = sum_j p_ij grid[:, j] | m_i = p_{i, j*(i)} ],   j*(i) = argmax_j x_ij,
// split the upstream gradient dagg [B][67][HW] into ga (32) | gw (32) | ge (2) | gm (1):
//     t_ij        = gw_i . vol1[:, j] + ge_i . grid[:, j] + gm_i [j == j*(i)]
//     delta_i     = sum_j p_ij t_ij = gw_i . w_i + ge_i . e_i + gm_i m_i            (row-local: from agg and dagg alone)
//     dx_ij       = p_ij (t_ij - delta_i)
//     dvol0[:, i] = ga_i + sum_j dx_ij vol1[:, j]
//     dvol1[:, j] = sum_i (p_ij gw_i + dx_ij vol0[:, i])
// No (HW, HW) tensor in either direction: the training forward (k_cvw_stats<true> + k_cvw_apply, the inference launches plus j*) saves
// per row the log2-domain maximum, the sum and j*; the backward recomputes p tile by tile from them, as K22 / K23 do.
//   k_cvw_delta   delta_i (one thread per row, channel-major reads)
//   k_cvw_dvol0   a workgroup owns 128 rows (a lane one row, as k_cvw_apply) and walks the 32-column tiles: scores and t on the matrix core
//                 (16 + 16 MFMAs, gw_i in place of vol0_i), grid and arg-max terms on the VALU, dvol0^T[ch][row] += vol1[ch][col] dx (16)
//   k_cvw_dvol1   a workgroup owns 128 columns (a lane one column) and walks the 32-row tiles in ascending order: vol0, gw and the row
//                 scalars staged in LDS; scores and t (16 + 16), dvol1^T[ch][col] += gw[ch][row] p + vol0[ch][row] dx (16 + 16)
// Exact fp32 on v_mfma_f32_32x32x2_f32 throughout.  Every output element is summed by one lane in a fixed order: no atomics, the same
// bits from run to run and for a pair alone or in a batch (the blocking depends on HW only).
#include "corr_volume_warp.h"

namespace {

constexpr int CA = 2 * D + 3;         // channels of agg / dagg

__global__ __launch_bounds__(256) void k_cvw_delta(const float* __restrict__ agg, const float* __restrict__ dagg, int B, int HW,
                                                   float* __restrict__ delta) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= (long)B * HW) return;
    const int b = (int)(n / HW), i = (int)(n - (long)b * HW);
    const float* a = agg + (size_t)b * CA * HW + i;
    const float* g = dagg + (size_t)b * CA * HW + i;
    float d = 0.f;
    for (int c = D; c < CA; ++c) d = fmaf(g[(size_t)c * HW], a[(size_t)c * HW], d);
    delta[n] = d;
}

__global__ __launch_bounds__(256) void k_cvw_dvol0(const float* __restrict__ vol0, const float* __restrict__ vol1,
                                                   const float* __restrict__ grid, const float2* __restrict__ stat,
                                                   const int* __restrict__ jstar, const float* __restrict__ dagg,
                                                   const float* __restrict__ delta, int B, int HW, float* __restrict__ dvol0) {
    __shared__ float lds[D * LROW];
    __shared__ float gl[2 * KT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int nI = (HW + 127) / 128;
    const int b = blockIdx.x / nI, Ib = blockIdx.x - b * nI;
    const int row = Ib * 128 + 32 * wave + l31;
    const bool live = row < HW;
    const float* v0 = vol0 + (size_t)b * D * HW;
    const float* v1 = vol1 + (size_t)b * D * HW;
    const float* dg = dagg + (size_t)b * CA * HW;
    float q[16], gq[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        q[t] = live ? v0[(size_t)(2 * t + h) * HW + row] : 0.f;
        gq[t] = live ? dg[(size_t)(D + 2 * t + h) * HW + row] : 0.f;
    }
    const float2 st = live ? stat[(size_t)b * HW + row] : make_float2(0.f, 1.f);
    const float rinv = 1.0f / st.y;
    const float ge0 = live ? dg[(size_t)(2 * D) * HW + row] : 0.f, ge1 = live ? dg[(size_t)(2 * D + 1) * HW + row] : 0.f;
    const float gm = live ? dg[(size_t)(2 * D + 2) * HW + row] : 0.f;
    const float dl = live ? delta[(size_t)b * HW + row] : 0.f;
    const int js = live ? jstar[(size_t)b * HW + row] : -1;
    f32x16 acc;                                          // D[m = channel][n = row]
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int j0 = 0; j0 < HW; j0 += KT) {
        __syncthreads();
        stage_tile(lds, gl, v1, grid, HW, j0, tid);
        __syncthreads();
        f32x16 sc, tt;
        score_tile(sc, lds, q, l31, h);
        score_tile(tt, lds, gq, l31, h);                 // gw_i . vol1[:, col]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = mfma32_row(r, h);
            float p = __builtin_amdgcn_exp2f(sc[r] * LOG2E - st.x) * rinv;
            if (j0 + c >= HW) p = 0.f;
            float t = fmaf(ge1, gl[KT + c], fmaf(ge0, gl[c], tt[r]));
            if (j0 + c == js) t += gm;
            sc[r] = p * (t - dl);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[l31 * LROW + mfma32_row(r, h)], sc[r], acc, 0, 0, 0);
    }
    if (live) {
        float* o = dvol0 + (size_t)b * D * HW + row;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = mfma32_row(r, h);
            o[(size_t)ch * HW] = dg[(size_t)ch * HW + row] + acc[r];
        }
    }
}

constexpr int NSC = 6;                // staged row scalars: max, 1 / sum, delta, ge0, ge1, gm (j* beside them, as int)

__global__ __launch_bounds__(256) void k_cvw_dvol1(const float* __restrict__ vol0, const float* __restrict__ vol1,
                                                   const float* __restrict__ grid, const float2* __restrict__ stat,
                                                   const int* __restrict__ jstar, const float* __restrict__ dagg,
                                                   const float* __restrict__ delta, int B, int HW, float* __restrict__ dvol1) {
    __shared__ float l0[D * LROW];                       // vol0[ch][row of the tile]
    __shared__ float lg[D * LROW];                       // gw[ch][row of the tile]
    __shared__ float rs[NSC * KT];
    __shared__ int rj[KT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int nJ = (HW + 127) / 128;
    const int b = blockIdx.x / nJ, Jb = blockIdx.x - b * nJ;
    const int col = Jb * 128 + 32 * wave + l31;
    const bool live = col < HW;
    const float* v0 = vol0 + (size_t)b * D * HW;
    const float* v1 = vol1 + (size_t)b * D * HW;
    const float* dg = dagg + (size_t)b * CA * HW;
    float k[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) k[t] = live ? v1[(size_t)(2 * t + h) * HW + col] : 0.f;
    const float gu = live ? grid[col] : 0.f, gv = live ? grid[(size_t)HW + col] : 0.f;
    f32x16 acc;                                          // D[m = channel][n = column]
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int i0 = 0; i0 < HW; i0 += KT) {
        __syncthreads();
        for (int e = tid; e < D * KT; e += 256) {
            const int ch = e >> 5, c = e & 31;
            const bool in = i0 + c < HW;
            l0[ch * LROW + c] = in ? v0[(size_t)ch * HW + i0 + c] : 0.f;
            lg[ch * LROW + c] = in ? dg[(size_t)(D + ch) * HW + i0 + c] : 0.f;
        }
        if (tid < NSC * KT) {                            // a padded row: 1 / sum = 0, so p = dx = 0
            const int w = tid >> 5, c = tid & 31, i = i0 + c;
            float v = 0.f;
            if (i < HW) {
                const size_t n = (size_t)b * HW + i;
                if (w == 0) v = stat[n].x;
                else if (w == 1) v = 1.0f / stat[n].y;
                else if (w == 2) v = delta[n];
                else v = dg[(size_t)(2 * D + w - 3) * HW + i];
            }
            rs[tid] = v;
        } else if (tid < (NSC + 1) * KT) {
            const int c = tid & 31;
            rj[c] = i0 + c < HW ? jstar[(size_t)b * HW + i0 + c] : -1;
        }
        __syncthreads();
        f32x16 sc, tt;                                   // D[m = row of the tile][n = this lane's column]
        score_tile(sc, l0, k, l31, h);
        score_tile(tt, lg, k, l31, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = mfma32_row(r, h);
            float p = __builtin_amdgcn_exp2f(sc[r] * LOG2E - rs[c]) * rs[KT + c];
            if (!live) p = 0.f;
            float t = fmaf(rs[4 * KT + c], gv, fmaf(rs[3 * KT + c], gu, tt[r]));
            if (col == rj[c]) t += rs[5 * KT + c];
            sc[r] = p;
            tt[r] = p * (t - rs[2 * KT + c]);
        }
        // dvol1^T[ch][col] += sum_row gw[ch][row] p[row][col] + vol0[ch][row] dx[row][col]: k-slot h of step r = row mfma32_row(r, h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lg[l31 * LROW + mfma32_row(r, h)], sc[r], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(l0[l31 * LROW + mfma32_row(r, h)], tt[r], acc, 0, 0, 0);
        }
    }
    if (live) {
        float* o = dvol1 + (size_t)b * D * HW + col;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[(size_t)mfma32_row(r, h) * HW] = acc[r];
    }
}

}  // namespace

extern "C" {

// saved: [B HW] float2 (log2-domain row maximum, sum of 2^(x log2 e - max)) | [B HW] int32 j*
size_t far_corr_volume_warp_train_saved_bytes(int B, int HW) {
    return B > 0 && HW > 0 ? (size_t)B * HW * (sizeof(float2) + sizeof(int)) : 0;
}

size_t far_corr_volume_warp_bwd_workspace_bytes(int B, int HW) { return B > 0 && HW > 0 ? (size_t)B * HW * sizeof(float) : 0; }

// far_corr_volume_warp_f32 (the same launches, the same bits in agg) that also fills `saved` for far_corr_volume_warp_bwd_f32.
int far_corr_volume_warp_train_f32(const float* vol0, const float* vol1, const float* grid, int B, int Dch, int HW, float* agg,
                                   void* saved, hipStream_t stream) {
    far_clear_errors();
    if (!vol0 || !vol1 || !grid || !agg || !saved || B <= 0 || HW <= 0 || Dch != D) return FAR_EINVAL;
    const int nI = (HW + 127) / 128;
    float2* stat = (float2*)saved;
    int* js = (int*)(stat + (size_t)B * HW);
    hipLaunchKernelGGL(k_cvw_stats<true>, dim3(nI * B), dim3(256), 0, stream, vol0, vol1, B, HW, stat, js);
    hipLaunchKernelGGL(k_cvw_apply, dim3(nI * B), dim3(256), 0, stream, vol0, vol1, grid, (const float2*)stat, B, HW, agg);
    return far_check_launch();
}

// dvol0, dvol1 [B][D][HW] (either may be NULL: its kernel is skipped) from dagg [B][2 D + 3][HW], the forward's agg and `saved`.
int far_corr_volume_warp_bwd_f32(const float* vol0, const float* vol1, const float* grid, const float* agg, const void* saved,
                                 const float* dagg, int B, int Dch, int HW, float* dvol0, float* dvol1, void* ws, hipStream_t stream) {
    far_clear_errors();
    if (!vol0 || !vol1 || !grid || !agg || !saved || !dagg || !ws || B <= 0 || HW <= 0 || Dch != D) return FAR_EINVAL;
    if (!dvol0 && !dvol1) return FAR_OK;
    const int nI = (HW + 127) / 128;
    const float2* stat = (const float2*)saved;
    const int* js = (const int*)(stat + (size_t)B * HW);
    float* delta = (float*)ws;
    const long n = (long)B * HW;
    hipLaunchKernelGGL(k_cvw_delta, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, agg, dagg, B, HW, delta);
    if (dvol0)
        hipLaunchKernelGGL(k_cvw_dvol0, dim3(nI * B), dim3(256), 0, stream, vol0, vol1, grid, stat, js, dagg, delta, B, HW, dvol0);
    if (dvol1)
        hipLaunchKernelGGL(k_cvw_dvol1, dim3(nI * B), dim3(256), 0, stream, vol0, vol1, grid, stat, js, dagg, delta, B, HW, dvol1);
    return far_check_launch();
}

}  // extern "C"
