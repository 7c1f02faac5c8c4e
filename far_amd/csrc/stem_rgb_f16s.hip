// K25: the RGB stem of the 8-Point-ViT's extractor in one launch -- channel flip, / 255, (x - mean) / std, nearest-neighbour resize to
// 224 x 224, 7x7 stride-2 pad-3 convolution (3 -> 64), folded BatchNorm, ReLU -- writing NHWC (N, 112, 112, 64) for K26 / K9.
//
// Replaces interiornetStreetlearn_8ptVit/src/model.py:135-138 (flip, normalisation), :145 (F.interpolate(size=224)), :147-149
// (resnet.conv1, bn1, relu).
// K10's layout with three input planes: a GEMM with M = output pixels, K = 147 taps (c, ky, kx; padded to 160 = ten k-steps of
// v_mfma_f32_32x32x16_f16), N = 64; one workgroup = 4 waves = 4 output rows x 32 columns; the 3 x 13 x 69 patch OF THE NORMALISED,
// RESIZED image and the pre-split weight fragments live in LDS.  The convolution's zero padding is zero in normalised space, so the
// normalisation cannot be folded into the weights: it is applied where a pixel is loaded, and a padded position stores 0.  The
// resize reads the source through two index tables (row, column) the host takes from torch's own interpolate.  Split-precision
// operands (hi.hi + hi.lo + lo.hi, fp32 accumulation); a normalised pixel is within +-2.7, scaled by 2^4 as K10's.
#include "common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int SIZE = 224, OUT = 112, C = 64, NTILES = 2;
constexpr int SR = 4, SC = 32;                     // output rows / columns per tile
constexpr int PH = 2 * SR + 5, PW = 2 * SC + 5;    // 13 x 69
constexpr int PLANE = PH * PW;
constexpr int TAPS = 147, KSTEPS = 10;             // 3 x 7 x 7, padded to 160
constexpr int YB = 7;                              // tiles (of 4 output rows) per workgroup: the 40 KB weight image is staged once for them
constexpr int TILES_X = (OUT + SC - 1) / SC, TILES_Y = OUT / SR;
constexpr int WF = KSTEPS * NTILES * 2 * 512;      // fp16 values of the weight fragments
constexpr float PIX_SCALE = 16.0f;

__global__ __launch_bounds__(256) void k_stem_rgb(const float* __restrict__ img, int H, int W, const int* __restrict__ rowidx,
                                                  const int* __restrict__ colidx, const _Float16* __restrict__ packed,
                                                  const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ y) {
    __shared__ float patch[3 * PLANE];
    __shared__ __attribute__((aligned(16))) _Float16 wf[WF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    constexpr int nby = TILES_Y / YB;
    int t = blockIdx.x;
    const int tx = t % TILES_X;
    t /= TILES_X;
    const int tyb = t % nby, n = t / nby;
    const int ox0 = tx * SC;
    const float* im = img + (size_t)n * 3 * H * W;
    for (int i = tid; i < WF / 8; i += 256) reinterpret_cast<f16x8*>(wf)[i] = reinterpret_cast<const f16x8*>(packed)[i];
    float sc[NTILES], sh[NTILES];
#pragma unroll
    for (int nt = 0; nt < NTILES; ++nt) { sc[nt] = scale[32 * nt + l31]; sh[nt] = shift[32 * nt + l31]; }
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
    // the convolution's channel c is the image's channel 2 - c (model.py:135), normalised with the c-th mean / std
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
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
            if (i < 3 * PLANE && iy >= 0 && iy < SIZE && ix >= 0 && ix < SIZE) {
                const float s = im[((size_t)(2 - c) * H + rowidx[iy]) * W + colidx[ix]];
                v = ((s / 255.0f - mean[c]) / stdv[c]) * PIX_SCALE;
            }
            nxt[j] = v;
        }
    };
    const int ty_end = (tyb + 1) * YB;
    request(tyb * YB);
    for (int ty = tyb * YB; ty < ty_end; ++ty) {
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
                const float v = acc[nt][r] * sc[nt] + sh[nt];  // a ReLU that keeps NaN (as K10)
                if (ox < OUT) y[(((size_t)n * OUT + oy) * OUT + ox) * C + co] = v < 0.f ? 0.f : v;
            }
        }
    }
}

// weight fragments: item (k-step ks, tile nt, lane): the 8 taps 16 ks + 8 (lane >> 5) + e of channel 32 nt + (lane & 31), times
// pack_scale[0], as a hi and a lo plane; the pad taps are zero
__global__ __launch_bounds__(256) void k_stem_rgb_pack(const float* __restrict__ w, const float* __restrict__ pack_scale,
                                                       _Float16* __restrict__ packed, const float* __restrict__ base_scale,
                                                       float* __restrict__ scale_vec) {
    const float wmul = pack_scale[0];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < KSTEPS * NTILES * 64; i += gridDim.x * 256) {
        const int ln = i & 63, nt = (i >> 6) % NTILES, ks = i / (64 * NTILES);
        const int co = 32 * nt + (ln & 31);
        f16x8 vh, vl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int tap = 16 * ks + 8 * (ln >> 5) + e;
            const float v = tap < TAPS ? w[co * TAPS + tap] * wmul : 0.f;
            const _Float16 hh = (_Float16)v;
            vh[e] = hh;
            vl[e] = (_Float16)(v - (float)hh);
        }
        _Float16* dst = packed + (size_t)((ks * NTILES + nt) * 2) * 512 + ln * 8;
        *reinterpret_cast<f16x8*>(dst) = vh;
        *reinterpret_cast<f16x8*>(dst + 512) = vl;
    }
    for (int co = blockIdx.x * 256 + threadIdx.x; co < C; co += gridDim.x * 256)
        scale_vec[co] = (base_scale ? base_scale[co] : 1.0f) * pack_scale[1];
}

// K26: max-pool 3x3 stride 2 pad 1, NHWC; four channels per thread; the padding takes no part (-inf), a NaN stays a NaN
__global__ __launch_bounds__(256) void k_maxpool3x3s2(const float* __restrict__ x, long total, int H, int W, int Ho, int Wo, int C4,
                                                      float* __restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    long u = i / C4;
    const int ox = (int)(u % Wo);
    u /= Wo;
    const int oy = (int)(u % Ho);
    const long n = u / Ho;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int iy = 2 * oy + dy;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int ix = 2 * ox + dx;
            if (ix < 0 || ix >= W) continue;
            const float4 v = reinterpret_cast<const float4*>(x)[(((size_t)n * H + iy) * W + ix) * C4 + c4];
            const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (a[k] > m[k] || a[k] != a[k]) m[k] = a[k];
        }
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(m[0], m[1], m[2], m[3]);
}

}  // namespace

extern "C" {

// Bytes of K25's packed weight image (the (64, 3, 7, 7) weight as split-fp16 fragments).
size_t far_stem_rgb_packed_bytes(void) { return (size_t)WF * sizeof(_Float16); }

// Packs w [64][3][7][7] (torch layout) times pack_scale[0] (far_weight_scale_f32's two device floats) and writes the epilogue scale
// vector scale_vec[co] = base_scale[co] (1 when NULL) * pack_scale[1].
int far_stem_rgb_pack_f32(const float* w, const float* pack_scale, void* packed, const float* base_scale, float* scale_vec,
                          hipStream_t stream) {
    far_clear_errors();
    if (!w || !pack_scale || !packed || !scale_vec) return FAR_EINVAL;
    hipLaunchKernelGGL(k_stem_rgb_pack, dim3(5), dim3(256), 0, stream, w, pack_scale, (_Float16*)packed, base_scale, scale_vec);
    return far_check_launch();
}

// y[n][oy][ox][co] = relu(scale[co] sum_{c, ky, kx} X[n][c][2 oy + ky - 3][2 ox + kx - 3] w[co][c][ky][kx] + shift[co]) with
// X[n][c][i][j] = (img[n][2 - c][rowidx[i]][colidx[j]] / 255 - mean[c]) / std[c] inside the 224 x 224 grid and 0 outside (mean, std: the
// ImageNet constants of model.py:136-137).  img [N][3][H][W] fp32 contiguous, values 0 .. 255, left as it is; rowidx / colidx [224]
// int32 on the device, every entry in [0, H) / [0, W) (the caller's: a wrong table reads out of bounds); y [N][112][112][64] NHWC;
// `scale` includes 2^-(w_exp + 4) (far_stem_rgb_pack_f32 writes it).
int far_stem_rgb_f16s(const float* img, long N, int H, int W, const int* rowidx, const int* colidx, const void* packed, const float* scale,
                      const float* shift, float* y, hipStream_t stream) {
    far_clear_errors();
    if (N == 0) return FAR_OK;
    if (!img || !rowidx || !colidx || !packed || !scale || !shift || !y || N < 0 || H <= 0 || W <= 0 ||
        (reinterpret_cast<uintptr_t>(packed) & 15))
        return FAR_EINVAL;
    const long nb = N * TILES_X * (TILES_Y / YB);
    if (nb > 0x7fffffffL) return FAR_EINVAL;
    hipLaunchKernelGGL(k_stem_rgb, dim3((unsigned)nb), dim3(256), 0, stream, img, H, W, rowidx, colidx, (const _Float16*)packed, scale, shift, y);
    return far_check_launch();
}

// y = max_pool2d(x, 3, stride 2, padding 1) for x [N][H][W][C] fp32 NHWC -> y [N][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C]; C % 4 == 0,
// 16-byte aligned tensors.  Exact; the padding counts as -inf.
int far_maxpool3x3s2_nhwc_f32(const float* x, long N, int H, int W, int Cc, float* y, hipStream_t stream) {
    far_clear_errors();
    if (N == 0) return FAR_OK;
    if (!x || !y || x == y || N < 0 || H <= 0 || W <= 0 || Cc <= 0 || (Cc & 3) || (reinterpret_cast<uintptr_t>(x) & 15) ||
        (reinterpret_cast<uintptr_t>(y) & 15))
        return FAR_EINVAL;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long total = N * Ho * Wo * (Cc / 4);
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) return FAR_EINVAL;
    hipLaunchKernelGGL(k_maxpool3x3s2, dim3((unsigned)blocks), dim3(256), 0, stream, x, total, H, W, Ho, Wo, Cc / 4, y);
    return far_check_launch();
}

}  // extern "C"
