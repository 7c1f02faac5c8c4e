// What K24's forward (conv_valid_f16s.hip) and its input gradient (conv_valid_bwd_f16s.hip) share: both are the same implicit GEMM of a
// 5 x 5 unpadded convolution on the f16 matrix cores with split-precision operands (hi.hi + hi.lo + lo.hi, fp32 accumulation) -- the
// dgrad is the forward on dy, shifted by four pixels, with the channels of the weight exchanged and its taps reversed.
//   KS .. STEPS, valid_shape   the geometry and the shapes K24 covers
//   conv_valid_tile.inc        the tile loop, a fragment both kernels include into their bodies (its head says why it is no function):
//                              one workgroup = 4 waves = an 8 MT-row x 8-column tile x 2 NTW 32-channel N-tiles.  Per 32-channel chunk
//                              of the reduction the (8 MT + 4) x 12 patch is scaled, split once into fp16 hi / lo planes in LDS (80 B
//                              per pixel and plane: the 16-byte fragment reads of eight neighbouring pixels fall into distinct banks)
//                              and the 25 taps walk over it: an A fragment is a shifted 16-byte read, no im2col.  The B fragments come
//                              pre-split from the packed image in 1 KB coalesced reads (every workgroup reads the same image: L2
//                              resident), requested one k-step ahead of their use.  The sum of an element runs over (chunk, tap,
//                              k-step) in that order whatever the launch: the same bits run to run and batch to batch
//   k_valid_pack, valid_pack   the packed image [chunk][tap][k-step][N-tile][plane][lane][8] of either direction
// The epilogues, and what a launch chooses for MT and NTW, stay with their kernels.  Each including file gets its own copy in its
// anonymous namespace.
#pragma once
#include "common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int KS = 5, TAPS = KS * KS;
constexpr int TW = 8, PW = TW + KS - 1;                 // tile width of a workgroup; patch width 12
constexpr int PSTR = 40;                                // fp16 per patch pixel and plane: 32 channels + 8 of padding
constexpr int NTHR = 256;
constexpr int STEPS = TAPS * 2;                         // k-steps of 16 channels per chunk

bool valid_shape(int Cin, int Cout, int ksize) {
    return ksize == KS && Cin > 0 && Cout > 0 && (Cin & 31) == 0 && (Cout & 31) == 0;
}

// The packed image of w [Cout][Cin][5][5]: item (chunk c, tap t, k-step s, N-tile nt, lane) holds, as a hi and a lo fp16 plane of 512
// values each, w times pack_scale[0] at the eight reduction channels 32 c + 16 s + 8 (lane >> 5) + e of the N-side channel
// 32 nt + (lane & 31).  Forward: the reduction runs over Cin, N is Cout, tap t; scale_vec[co] = base_scale[co] (1 when NULL) *
// pack_scale[1] is written as well.  DGRAD: the channels exchanged (reduction over Cout, N is Cin), tap 24 - t, no scale vector.
__host__ __device__ inline long valid_pack_items(int Cin, int Cout) { return (long)(Cin >> 5) * (Cout >> 5) * TAPS * 2 * 64; }

template <bool DGRAD>
__global__ __launch_bounds__(256) void k_valid_pack(const float* __restrict__ w, int Cin, int Cout, const float* __restrict__ pack_scale,
                                                    _Float16* __restrict__ packed, const float* __restrict__ base_scale,
                                                    float* __restrict__ scale_vec) {
    const int NT = (DGRAD ? Cin : Cout) >> 5;
    const long items = valid_pack_items(Cin, Cout);
    const float wmul = pack_scale[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int ln = (int)(i & 63);
        long u = i >> 6;
        const int nt = (int)(u % NT);
        u /= NT;
        const int s = (int)(u & 1);
        u >>= 1;
        const int t = (int)(u % TAPS), c = (int)(u / TAPS);
        const int cn = 32 * nt + (ln & 31);
        f16x8 vh, vl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ck = 32 * c + 16 * s + 8 * (ln >> 5) + e;
            const float v = (DGRAD ? w[((size_t)ck * Cin + cn) * TAPS + (TAPS - 1 - t)] : w[((size_t)cn * Cin + ck) * TAPS + t]) * wmul;
            const _Float16 hh = (_Float16)v;
            vh[e] = hh;
            vl[e] = (_Float16)(v - (float)hh);
        }
        _Float16* dst = packed + (size_t)(i >> 6) * 1024 + ln * 8;
        *reinterpret_cast<f16x8*>(dst) = vh;
        *reinterpret_cast<f16x8*>(dst + 512) = vl;
    }
    if (!DGRAD && scale_vec)
        for (int co = blockIdx.x * 256 + threadIdx.x; co < Cout; co += gridDim.x * 256)
            scale_vec[co] = (base_scale ? base_scale[co] : 1.0f) * pack_scale[1];
}

template <bool DGRAD>
void valid_pack(const float* w, int Cin, int Cout, const float* pack_scale, void* packed, const float* base_scale, float* scale_vec,
                hipStream_t stream) {
    long blocks = (valid_pack_items(Cin, Cout) + 255) / 256;
    blocks = blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL(k_valid_pack<DGRAD>, dim3((unsigned)blocks), dim3(256), 0, stream, w, Cin, Cout, pack_scale, (_Float16*)packed, base_scale,
                       scale_vec);
}

}  // namespace
