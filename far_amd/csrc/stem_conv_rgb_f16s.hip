// K27: the RGB stem of the Map-free regressor's ResUNet encoder at any image size, one launch -- 7x7 stride-2 pad-3 convolution (3 -> 64),
// folded BatchNorm, ReLU -- writing NHWC (N, (H - 1) / 2 + 1, (W - 1) / 2 + 1, 64) for K26 / K9.
//
// Replaces mapfree_6dreg/lib/models/regression/encoder/resunet.py:106-108 (firstconv, firstbn, firstrelu).
// K25's GEMM layout (stem_rgb_f16s.hip) without its image preparation: M = output pixels, K = 147 taps (c, ky, kx; padded to 160 = ten
// k-steps of v_mfma_f32_32x32x16_f16), N = 64; one workgroup = 4 waves = 4 output rows x 32 columns per tile, YB tiles of rows per
// workgroup (the 40 KB weight image is staged once for them); the 3 x 13 x 69 patch of the image and the pre-split weight fragments live
// in LDS.  No channel flip, no / 255, no normalisation, no resize tables: the image arrives as the network consumes it, and the zero
// padding is the image's.  The weight image is K25's (far_stem_rgb_pack_f32).  Split-precision operands (hi.hi + hi.lo + lo.hi, fp32
// accumulation) around 2^act_exp as K9's activations: |pixel| <= 65504 / 2^act_exp survives, beyond it the sums are not finite and the
// launch ORs the overflow flag (as K9 / K24).
#include "common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int C = 64, NTILES = 2;
constexpr int SR = 4, SC = 32;                     // output rows / columns per tile
constexpr int PH = 2 * SR + 5, PW = 2 * SC + 5;    // 13 x 69
constexpr int PLANE = PH * PW;
constexpr int TAPS = 147, KSTEPS = 10;             // 3 x 7 x 7, padded to 160
constexpr int YB = 7;                              // tiles (of 4 output rows) per workgroup
constexpr int WF = KSTEPS * NTILES * 2 * 512;      // fp16 values of the weight fragments (K25's image)
constexpr int ACT_EXP_DEFAULT = 4;                 // the exponent the packed scale vector folds (2^-(w_exp + 4))

__global__ __launch_bounds__(256) void k_stem_conv_rgb(const float* __restrict__ img, int H, int W, int Ho, int Wo, int tiles_x, int tiles_y,
                                                       const _Float16* __restrict__ packed, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, float act_scale, float out_mul,
                                                       int* __restrict__ overflow, float* __restrict__ y) {
    __shared__ float patch[3 * PLANE];
    __shared__ __attribute__((aligned(16))) _Float16 wf[WF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nby = (tiles_y + YB - 1) / YB;
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int tyb = t % nby, n = t / nby;
    const int ox0 = tx * SC;
    const float* im = img + (size_t)n * 3 * H * W;
    for (int i = tid; i < WF / 8; i += 256) reinterpret_cast<f16x8*>(wf)[i] = reinterpret_cast<const f16x8*>(packed)[i];
    float sc[NTILES], sh[NTILES];
#pragma unroll
    for (int nt = 0; nt < NTILES; ++nt) { sc[nt] = scale[32 * nt + l31] * out_mul; sh[nt] = shift[32 * nt + l31]; }
    // patch offsets of this lane's 8 taps per k-step (the pad taps read offset 0: their weights are zero)
    int toff[KSTEPS][8];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int tap = 16 * ks + 8 * h + e;
            const int c = tap / 49, r = tap - 49 * c;
            toff[ks][e] = tap < TAPS ? c * PLANE + (r / 7) * PW + r % 7 : 0;
        }
    constexpr int PIT = (3 * PLANE + 255) / 256;
    float nxt[PIT];
    auto request = [&](int ty) {
        const int oy0 = ty * SR;
#pragma unroll
        for (int j = 0; j < PIT; ++j) {
            const int i = tid + 256 * j;
            const int c = i / PLANE, q = i - c * PLANE;
            const int py = q / PW, px = q - py * PW;
            const int iy = 2 * oy0 - 3 + py, ix = 2 * ox0 - 3 + px;
            float v = 0.f;
            if (i < 3 * PLANE && iy >= 0 && iy < H && ix >= 0 && ix < W) v = im[((size_t)c * H + iy) * W + ix] * act_scale;
            nxt[j] = v;
        }
    };
    const int ty_begin = tyb * YB, ty_end = min((tyb + 1) * YB, tiles_y);
    float chk = 0.f;
    request(ty_begin);
    for (int ty = ty_begin; ty < ty_end; ++ty) {
        const int oy0 = ty * SR;
        __syncthreads();                                       // the previous tile's patch is consumed (and wf is written)
#pragma unroll
        for (int j = 0; j < PIT; ++j)
            if (tid + 256 * j < 3 * PLANE) patch[tid + 256 * j] = nxt[j];
        __syncthreads();
        if (ty + 1 < ty_end) request(ty + 1);                  // in flight under this tile's gathers, MFMAs and stores
        f32x16 acc[NTILES];
#pragma unroll
        for (int nt = 0; nt < NTILES; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
        const int abase = (2 * wave) * PW + 2 * l31;           // patch offset of this lane's output pixel (row wave, col l31)
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            f16x8 ah, al;
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                f16x2 hh, ll;
                split2(f32x2{patch[abase + toff[ks][e]], patch[abase + toff[ks][e + 1]]}, hh, ll);
                ah[e] = hh.x; ah[e + 1] = hh.y; al[e] = ll.x; al[e + 1] = ll.y;
            }
#pragma unroll
            for (int nt = 0; nt < NTILES; ++nt) {
                const _Float16* src = wf + (size_t)((ks * NTILES + nt) * 2) * 512 + lane * 8;
                const f16x8 bh = *reinterpret_cast<const f16x8*>(src), bl = *reinterpret_cast<const f16x8*>(src + 512);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[nt], 0, 0, 0);
            }
        }
        const int oy = oy0 + wave;
#pragma unroll
        for (int nt = 0; nt < NTILES; ++nt) {
            const int co = 32 * nt + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ox = ox0 + mfma32_row(r, h);
                chk += acc[nt][r];
                const float v = acc[nt][r] * sc[nt] + sh[nt];  // a ReLU that keeps NaN (as K10)
                if (ox < Wo && oy < Ho) y[(((size_t)n * Ho + oy) * Wo + ox) * C + co] = v < 0.f ? 0.f : v;
            }
        }
    }
    // Range guard (as K9 / K24): a pixel beyond the split's range (|a| 2^act_exp > 65504) or a non-finite one reaches the accumulators as
    // inf / NaN, and the sum of a lane's accumulators is not finite exactly then; one integer atomic per wave that saw it, none otherwise.
    if (overflow && __any(!(fabsf(chk) <= FLT_MAX)) && lane == 0) atomicOr(overflow, 1);
}

}  // namespace

extern "C" {

// y[n][oy][ox][co] = relu(scale[co] 2^(4 - act_exp) sum_{c, ky, kx} X[n][c][2 oy + ky - 3][2 ox + kx - 3] w[co][c][ky][kx] + shift[co]) with
// X = img inside the image and 0 outside.  img [N][3][H][W] fp32 contiguous, left as it is; packed / scale: far_stem_rgb_pack_f32's
// image and scale vector (which includes 2^-(w_exp + 4)); y [N][(H - 1) / 2 + 1][(W - 1) / 2 + 1][64] NHWC.  act_exp and overflow as
// far_conv_nhwc_f32: pixels are split around 2^act_exp, the device int is OR-ed with 1 when one left the split's range.
int far_stem_conv_rgb_f16s(const float* img, long N, int H, int W, const void* packed, const float* scale, const float* shift, float* y,
                           int act_exp, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (act_exp < -24 || act_exp > 8 || N < 0) return FAR_EINVAL;
    if (N == 0) return FAR_OK;
    if (!img || !packed || !scale || !shift || !y || H <= 0 || W <= 0 || H > (1 << 20) || W > (1 << 20) ||
        (reinterpret_cast<uintptr_t>(packed) & 15))
        return FAR_EINVAL;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int tiles_x = (Wo + SC - 1) / SC, tiles_y = (Ho + SR - 1) / SR;
    const long nb = N * tiles_x * ((tiles_y + YB - 1) / YB);
    if (nb > 0x7fffffffL) return FAR_EINVAL;
    hipLaunchKernelGGL(k_stem_conv_rgb, dim3((unsigned)nb), dim3(256), 0, stream, img, H, W, Ho, Wo, tiles_x, tiles_y, (const _Float16*)packed,
                       scale, shift, ldexpf(1.0f, act_exp), ldexpf(1.0f, ACT_EXP_DEFAULT - act_exp), overflow, y);
    return far_check_launch();
}

}  // extern "C"
