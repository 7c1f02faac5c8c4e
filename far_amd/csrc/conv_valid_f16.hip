// K24 on plain fp16 operands: the 5 x 5 unpadded ('valid') stride-1 convolution of conv_valid_f16s.hip, NHWC fp32 in and out, with ONE
// fp16 value per activation and per weight (fp32 accumulation) and the same epilogue: acc * scale + shift (+ residual), ReLU.
//
// The 16-bit-operand sibling of K24 for ViTEss.set_precision (narrower than the reference -- never the parity configuration).  The
// implicit GEMM, the workgroup tile (4 waves = an 8 MT-row x 8-column output tile x six 32-channel N-tiles; MT = 3 for large launches,
// MT = 1 below SMALL_GRID workgroups), the patch layout in LDS (PSTR = 40 fp16 per pixel: the 16-byte fragment reads of eight
// neighbouring pixels fall into distinct banks) and the order of an output's sum -- (chunk, tap, k-step) -- are the split kernel's
// (conv_valid_f16s.h describes the scheme).  What differs:
//   operands one patch plane in LDS (x 2^act_exp rounded to fp16 once per chunk), one weight plane in the packed image
//            [chunk][tap][k-step][N-tile][lane][8] (far_conv_valid_pack_f16: half of the split image), one accumulator set and ONE
//            MFMA per (tile, k-step) where the split kernel issues three.
//   loop     with half the accumulators the register file is not full: the tile loop is a plain __device__ function here, not the
//            included fragment conv_valid_tile.inc, whose text is tuned to the register allocation of the split k_conv_valid<3>.
// Forward only: the input gradient stays a split-fp16 kernel.  The same bits run to run, for an image alone or in a batch, and in
// both launch forms (an output's sum is the same sequence of MFMAs).
#include "conv_valid_f16s.h"

namespace {

constexpr int NTW = 3;                                  // 32-channel N-tiles per wave
constexpr int SMALL_GRID = 128;                         // fewer 24-row workgroups than this: the 8-row form (MT = 1) fills more CUs
constexpr int ACT_EXP_DEFAULT = 4;

struct ValidArgs {
    const float* x;
    const _Float16* w;
    const float* scale;
    const float* shift;
    const float* res;
    float* y;
    int H, W, Ho, Wo, Cin, Cout, tilesX, tilesY, act;
    float act_scale, out_mul;
    int* overflow;
};

// items of 64 lanes x 8 fp16 (one B fragment: 1 KB)
__host__ __device__ inline long pack16_items(int Cin, int Cout) { return (long)(Cin >> 5) * (Cout >> 5) * TAPS * 2 * 64; }

// The plain image: item (chunk c, tap t, k-step s, N-tile nt, lane) holds fp16(w pack_scale[0]) at the eight input channels
// 32 c + 16 s + 8 (lane >> 5) + e of output channel 32 nt + (lane & 31): the hi plane of the split image, contiguous.
__global__ __launch_bounds__(256) void k_valid_pack_f16(const float* __restrict__ w, int Cin, int Cout, const float* __restrict__ pack_scale,
                                                        _Float16* __restrict__ packed, const float* __restrict__ base_scale,
                                                        float* __restrict__ scale_vec) {
    const int NT = Cout >> 5;
    const long items = pack16_items(Cin, Cout);
    const float wmul = pack_scale[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const int ln = (int)(i & 63);
        long u = i >> 6;
        const int nt = (int)(u % NT);
        u /= NT;
        const int s = (int)(u & 1);
        u >>= 1;
        const int t = (int)(u % TAPS), c = (int)(u / TAPS);
        const int co = 32 * nt + (ln & 31);
        f16x8 vh;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ci = 32 * c + 16 * s + 8 * (ln >> 5) + e;
            vh[e] = (_Float16)(w[((size_t)co * Cin + ci) * TAPS + t] * wmul);
        }
        *reinterpret_cast<f16x8*>(packed + (size_t)i * 8) = vh;
    }
    if (scale_vec)
        for (int co = blockIdx.x * 256 + threadIdx.x; co < Cout; co += gridDim.x * 256)
            scale_vec[co] = (base_scale ? base_scale[co] : 1.0f) * pack_scale[1];
}

// The tile loop: the sums of this wave's MT x NTW tiles over every (chunk, tap, k-step), in that order.  Every thread of the
// workgroup stages its share of each chunk's (8 MT + 4) x 12 patch; a wave that is not `live` (its rows lie below the result, or it
// has no N-tile) does nothing else.  x: image n.  ntw: the wave's N-tiles that exist (<= NTW), in a scalar register -- see the kernel.
// FULL: every wave of the workgroup has ntw == NTW, the tap loop without a guard between its MFMAs (the workload's Cout = 192
// always; the guarded form's scalar branches between the MFMAs slow the launch: profiles/vit8pt_fp16_variants_ab.txt).
template <int MT, bool FULL>
__device__ __forceinline__ void conv_tiles(const ValidArgs& p, const float* __restrict__ x, _Float16* __restrict__ patch, int oy0, int ox0,
                                           int mh, int nt0, int ntw, bool live, f32x16 (&acc)[MT][NTW]) {
    constexpr int PH = 8 * MT + KS - 1;
    constexpr int NITEMS = PH * PW * 8;                 // float4 loads per chunk
    constexpr int ITEMS = (NITEMS + NTHR - 1) / NTHR;   // per thread
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int NT = p.Cout >> 5, nchunks = p.Cin >> 5;
    const int abase = ((4 * MT * mh + (l31 >> 3)) * PW + (l31 & 7)) * PSTR + 8 * h;
    const f32x2 s2 = {p.act_scale, p.act_scale};

    // the B fragments of k-step j (tap j / 2, channels 16 (j & 1) ..) of chunk c, requested one k-step ahead of their MFMAs
    f16x8 b[2][NTW];
    auto fetch = [&](int c, int j, int slot) {
        const _Float16* wt = p.w + ((size_t)(c * STEPS + j) * NT + nt0) * 512 + lane * 8;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
            if (FULL || nt < ntw) b[slot][nt] = *reinterpret_cast<const f16x8*>(wt + nt * 512);
    };
    auto step = [&](int off, int cur) {
        f16x8 a[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f16x8*>(patch + off + 4 * mt * PW * PSTR);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
            if (FULL || nt < ntw) {                                    // a scalar branch: a matrix instruction ignores the lane mask
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mt], b[cur][nt], acc[mt][nt], 0, 0, 0);
            }
    };

    for (int c = 0; c < nchunks; ++c) {
        if (live) fetch(c, 0, 0);                                  // in flight under the staging below
        __syncthreads();                                           // the previous chunk's plane is consumed
        {
            float4 v[ITEMS];
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int i = tid + NTHR * j, pix = i >> 3, q = i & 7;
                const int py = pix / PW, px = pix - py * PW;
                const int yy = oy0 + py, xx = ox0 + px;
                v[j] = (i < NITEMS && yy < p.H && xx < p.W) ? *reinterpret_cast<const float4*>(x + ((size_t)yy * p.W + xx) * p.Cin + 32 * c + 4 * q)
                                                             : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int i = tid + NTHR * j, pix = i >> 3, q = i & 7;
                const f16x2 h0 = __builtin_convertvector(f32x2{v[j].x, v[j].y} * s2, f16x2);
                const f16x2 h1 = __builtin_convertvector(f32x2{v[j].z, v[j].w} * s2, f16x2);
                if (i < NITEMS) *reinterpret_cast<f16x4*>(patch + pix * PSTR + 4 * q) = f16x4{h0.x, h0.y, h1.x, h1.y};
            }
        }
        __syncthreads();
        if (!live) continue;
#pragma unroll 1
        for (int dy = 0; dy < KS; ++dy) {
#pragma unroll 1
            for (int dx = 0; dx < KS; ++dx) {
                const int tap = dy * KS + dx, off = abase + (dy * PW + dx) * PSTR;
                fetch(c, 2 * tap + 1, 1);
                step(off, 0);                                      // channels 0 .. 15 of the chunk
                if (tap + 1 < TAPS) fetch(c, 2 * tap + 2, 0);
                step(off + 16, 1);                                 // channels 16 .. 31
            }
        }
    }
}

// MT: 4 x 8-pixel M-tiles per wave; the workgroup's tile is 8 MT output rows x 8 columns, as in k_conv_valid.
template <int MT>
__global__ __launch_bounds__(NTHR) void k_conv_valid_f16(const ValidArgs p) {
    constexpr int PH = 8 * MT + KS - 1;
    __shared__ __attribute__((aligned(16))) _Float16 patch[PH * PW * PSTR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;                       // this wave's half of the rows / of the workgroup's six N-tiles
    int t = blockIdx.x;
    const int tx = t % p.tilesX;
    t /= p.tilesX;
    const int ty = t % p.tilesY, n = t / p.tilesY;
    const int oy0 = ty * 8 * MT, ox0 = tx * TW;
    const int NT = p.Cout >> 5, nt0 = (blockIdx.y * 2 + nh) * NTW;
    // Wave-uniform values the compiler cannot see as such (they come from threadIdx): read into scalar registers, so that the guards
    // on them are scalar branches.  As a lane-mask guard hipcc predicates a short block instead of jumping over it, and a matrix
    // instruction ignores the lane mask: the MFMA of an N-tile that does not exist then runs on a B fragment that was never loaded.
    const int ntw = __builtin_amdgcn_readfirstlane(NT - nt0 < NTW ? NT - nt0 : NTW);
    const bool live = __builtin_amdgcn_readfirstlane(oy0 + 4 * MT * mh < p.Ho && ntw > 0) != 0;

    f32x16 acc[MT][NTW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
    const float* const xn = p.x + (size_t)n * p.H * p.W * p.Cin;
    // Workgroup-uniform (block index and arguments only): all six N-tiles of this workgroup exist, so both of its wave pairs take the
    // unguarded loop; every wave of a workgroup reaches the same __syncthreads() call sites.
    const bool full = ((int)blockIdx.y * 2 + 2) * NTW <= NT;
    if (full) conv_tiles<MT, true>(p, xn, patch, oy0, ox0, mh, nt0, ntw, live, acc);
    else conv_tiles<MT, false>(p, xn, patch, oy0, ox0, mh, nt0, ntw, live, acc);
    if (!live) return;

    // Range guard (as K24): an input beyond fp16's range (|a| 2^act_exp > 65504) or a non-finite one reaches the accumulators as inf /
    // NaN, and the sum of a wave's accumulators is not finite exactly then; one integer atomic per wave that saw it, none otherwise.
    if (p.overflow) {
        float chk = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) chk += acc[mt][nt][r];            // (the tiles that do not exist stayed zero)
        if (__any(!(fabsf(chk) <= FLT_MAX)) && lane == 0) atomicOr(p.overflow, 1);
    }

#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        if (nt >= ntw) continue;
        const int co = 32 * (nt0 + nt) + l31;
        const float sc = p.scale[co] * p.out_mul, sh = p.shift ? p.shift[co] : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mfma32_row(r, h);
                const int oy = oy0 + 4 * MT * mh + 4 * mt + (m >> 3), ox = ox0 + (m & 7);
                if (oy < p.Ho && ox < p.Wo) {
                    const size_t o = (((size_t)n * p.Ho + oy) * p.Wo + ox) * p.Cout + co;
                    float v = acc[mt][nt][r] * sc + sh;
                    if (p.res) v += p.res[o];
                    if (p.act == 1) v = v < 0.f ? 0.f : v;          // a ReLU that keeps NaN (as K24)
                    p.y[o] = v;
                }
            }
        }
    }
}

}  // namespace

extern "C" {

// Bytes of the packed plain-fp16 image of a (Cout, Cin, 5, 5) weight: half of far_conv_valid_packed_bytes; 0 for a shape K24 does not
// cover (ksize != 5, Cin or Cout not a multiple of 32).
size_t far_conv_valid_f16_packed_bytes(int Cin, int Cout, int ksize) {
    if (!valid_shape(Cin, Cout, ksize)) return 0;
    return (size_t)Cin * Cout * TAPS * sizeof(_Float16);
}

// far_conv_valid_pack_f32 for the plain image: fp16(w pack_scale[0]) only, and the same epilogue scale vector.
int far_conv_valid_pack_f16(const float* w, int Cin, int Cout, int ksize, const float* pack_scale, void* packed, const float* base_scale,
                            float* scale_vec, hipStream_t stream) {
    far_clear_errors();
    if (!w || !pack_scale || !packed || !scale_vec || !valid_shape(Cin, Cout, ksize)) return FAR_EINVAL;
    long blocks = (pack16_items(Cin, Cout) + 255) / 256;
    blocks = blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL(k_valid_pack_f16, dim3((unsigned)blocks), dim3(256), 0, stream, w, Cin, Cout, pack_scale, (_Float16*)packed, base_scale,
                       scale_vec);
    return far_check_launch();
}

// far_conv_valid_f16s on plain fp16 operands: the same arguments, shapes, checks and return codes; `packed` is
// far_conv_valid_pack_f16's image.  Narrower than the reference; forward only.
int far_conv_valid_f16(const float* x, const void* packed, const float* scale, const float* shift, const float* res, float* y, long N,
                       int H, int W, int Cin, int Cout, int ksize, int act, int act_exp, int* overflow, hipStream_t stream) {
    far_clear_errors();
    if (act_exp < -24 || act_exp > 8 || act < 0 || act > 1 || N < 0) return FAR_EINVAL;
    if (!valid_shape(Cin, Cout, ksize) || H < KS || W < KS) return FAR_EINVAL;
    if (N == 0) return FAR_OK;
    if (!x || !packed || !scale || !y || x == y || (res && res == y) || (reinterpret_cast<uintptr_t>(x) & 15)) return FAR_EINVAL;
    ValidArgs a;
    a.x = x; a.w = (const _Float16*)packed; a.scale = scale; a.shift = shift; a.res = res; a.y = y;
    a.H = H; a.W = W; a.Ho = H - KS + 1; a.Wo = W - KS + 1; a.Cin = Cin; a.Cout = Cout;
    a.tilesX = (a.Wo + TW - 1) / TW; a.tilesY = (a.Ho + 23) / 24; a.act = act;
    a.act_scale = ldexpf(1.0f, act_exp); a.out_mul = ldexpf(1.0f, ACT_EXP_DEFAULT - act_exp); a.overflow = overflow;
    long nbx = N * a.tilesX * a.tilesY;
    const bool small = nbx < SMALL_GRID;
    if (small) { a.tilesY = (a.Ho + 7) / 8; nbx = N * a.tilesX * a.tilesY; }
    const int nby = ((Cout >> 5) + 2 * NTW - 1) / (2 * NTW);
    if (nbx > 0x7fffffffL || nby > 65535) return FAR_EINVAL;
    if (small) hipLaunchKernelGGL(k_conv_valid_f16<1>, dim3((unsigned)nbx, (unsigned)nby), dim3(NTHR), 0, stream, a);
    else hipLaunchKernelGGL(k_conv_valid_f16<3>, dim3((unsigned)nbx, (unsigned)nby), dim3(NTHR), 0, stream, a);
    return far_check_launch();
}

}  // extern "C"
