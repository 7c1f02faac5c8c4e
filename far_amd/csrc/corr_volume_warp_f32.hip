// K12: the correlation-volume warp of the Map-free 6DReg aggregator.
//
// Replaces mapfree_6dreg/lib/models/regression/aggregator.py:44-115 (CorrelationVolumeWarping.forward) in the FAR
// configuration (config/regression/mapfree/rot6d_trans_with_loftr.yaml: POSITION_ENCODER, MAX_SCORE_CHANNEL; no dustbin,
// no normalisation, no half channels; 32 feature channels on a 92 x 68 grid):
//     cvolume  = softmax_j(vol0_i . vol1_j)                      (B, HW, HW)  = 156 MB per pair at HW = 6256, fp32
//     vol1w    = vol1 cvolume^T                                   (B, 32, HW)
//     pos_enc  = grid cvolume^T                                   (B, 2, HW)   grid = meshgrid(linspace(-1,1,H), linspace(-1,1,W))
//     max_sc   = max_j cvolume_ij                                 (B, 1, HW)
//     agg      = cat[vol0, vol1w, pos_enc, max_sc]                (B, 67, H, W)
// A single softmax (rows only), so it is a two-pass "attention" with q = vol0, k = v = vol1, never materialising
// cvolume.  Arithmetic: EXACT fp32 on the f32-input matrix core (v_mfma_f32_32x32x2_f32 is bitwise an fmaf chain): with
// K = 32 channels the contractions are 5 GFLOP per pair -- 40 us at the f32 MFMA rate -- so there is nothing to gain
// from split-fp16 operands here, and nothing to argue about parity.
//   pass 1 (k_cvw_stats)  row maximum and sum of exp over all columns (online, lane = row in the transposed score tile)
//   pass 2 (k_cvw_apply)  p = exp(x - max) / sum;  vol1w^T[ch][row] += vol1[ch][col] p[row][col] on the matrix core
//                         (D[m = channel][n = row]: a lane owns a row, so the 32 lanes of a half-wave store 128 contiguous
//                         bytes of one output channel); the two grid channels on the VALU (2 FMAs per score);
//                         max_sc = 1 / sum.
// The channel-major layout of the reference ((B, D, HW): position contiguous) is exactly what the MFMA operands want:
// A[k = channel][col] and B[k = channel][row] are 128-byte contiguous global reads; the column tile is staged once per
// workgroup in LDS ([32 ch][33] floats, conflict-free both as score operand and as warp operand).
#include "corr_volume_warp.h"

extern "C" {

size_t far_corr_volume_warp_workspace_bytes(int B, int HW) { return B > 0 && HW > 0 ? (size_t)B * HW * sizeof(float2) : 0; }

// agg [B][2 D + 3][HW] = cat[vol0, vol1 softmax(vol0^T vol1)^T, grid softmax(..)^T, rowmax softmax(..)]  (D = 32)
// vol0, vol1 [B][D][HW] fp32 (the reference's (B, D, H, W) tensors), grid [2][HW].
int far_corr_volume_warp_f32(const float* vol0, const float* vol1, const float* grid, int B, int Dch, int HW, float* agg, void* ws,
                             hipStream_t stream) {
    far_clear_errors();
    if (!vol0 || !vol1 || !grid || !agg || !ws || B <= 0 || HW <= 0 || Dch != D) return FAR_EINVAL;
    const int nI = (HW + 127) / 128;
    hipLaunchKernelGGL(k_cvw_stats<false>, dim3(nI * B), dim3(256), 0, stream, vol0, vol1, B, HW, (float2*)ws, (int*)nullptr);
    hipLaunchKernelGGL(k_cvw_apply, dim3(nI * B), dim3(256), 0, stream, vol0, vol1, grid, (const float2*)ws, B, HW, agg);
    return far_check_launch();
}

}  // extern "C"
