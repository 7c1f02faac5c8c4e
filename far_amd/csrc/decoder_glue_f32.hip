// K28: the glue of the Map-free regressor's ResUNet decoder, exact fp32, NHWC.
//
// Replaces mapfree_6dreg/lib/models/regression/encoder/resunet.py:37-39 (F.interpolate(scale_factor=2, bilinear, align_corners=True) in
// front of an upconv's convolution), :90-95 (skipconnect: F.pad of the skip map to the upsampled size, diff // 2 before and the rest
// after) and :26 (F.elu behind the decoder's convolutions).
//   k_upsample2x_pad: ONE launch writes both inputs of the convolution that follows a skip connection -- the upsampled map and the
//     zero-padded skip map -- as two tensors K9 reads in place as cat([up, skip]) (x, x2); either half may be absent.
//   k_elu: y = x > 0 ? x : expm1(x), elementwise, in place or not.
// Four channels per thread.  The interpolation weights are exact: the source coordinate Y (h - 1) / (2 h - 1) is split into its integer
// part and remainder in integer arithmetic, and the remainder is divided once (torch forms the coordinate in fp32 and loses the low
// bits of the fraction at large Y).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void k_upsample2x_pad(const float4* __restrict__ lo, int h, int w, int cvec, long n_up,
                                                        float4* __restrict__ up, const float4* __restrict__ skip, int hs, int ws,
                                                        int svec, int top, int left, long n_total, float4* __restrict__ skip_out) {
    const int H = 2 * h, W = 2 * w;
    const float inv_y = 1.0f / (float)(H - 1), inv_x = 1.0f / (float)(W - 1);
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_total; i += stride) {
        if (i < n_up) {
            const int c4 = (int)(i % cvec);
            long p = i / cvec;
            const int X = (int)(p % W); p /= W;
            const int Y = (int)(p % H);
            const long n = p / H;
            const int ny = Y * (h - 1), nx = X * (w - 1);
            const int y0 = ny / (H - 1), x0 = nx / (W - 1);
            const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
            const float ly = (float)(ny - y0 * (H - 1)) * inv_y, lx = (float)(nx - x0 * (W - 1)) * inv_x;
            const float hy = 1.f - ly, hx = 1.f - lx;
            const float4* base = lo + n * h * w * cvec + c4;
            const float4 a = base[((long)y0 * w + x0) * cvec], b = base[((long)y0 * w + x1) * cvec];
            const float4 c = base[((long)y1 * w + x0) * cvec], d = base[((long)y1 * w + x1) * cvec];
            float4 v;
            // torch: hy * (hx * a + lx * b) + ly * (hx * c + lx * d)
            v.x = hy * (hx * a.x + lx * b.x) + ly * (hx * c.x + lx * d.x);
            v.y = hy * (hx * a.y + lx * b.y) + ly * (hx * c.y + lx * d.y);
            v.z = hy * (hx * a.z + lx * b.z) + ly * (hx * c.z + lx * d.z);
            v.w = hy * (hx * a.w + lx * b.w) + ly * (hx * c.w + lx * d.w);
            up[i] = v;
        } else {
            const long k = i - n_up;
            const int c4 = (int)(k % svec);
            long p = k / svec;
            const int X = (int)(p % W); p /= W;
            const int Y = (int)(p % H);
            const long n = p / H;
            const int ys = Y - top, xs = X - left;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ys >= 0 && ys < hs && xs >= 0 && xs < ws) v = skip[((n * hs + ys) * ws + xs) * svec + c4];
            skip_out[k] = v;
        }
    }
}

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }      // a NaN stays a NaN (expm1f(NaN))

__global__ __launch_bounds__(256) void k_elu(const float* __restrict__ x, long n, float* __restrict__ y, int vec) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec) {
        const long nv = n / 4;
        for (long i = i0; i < nv; i += stride) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            reinterpret_cast<float4*>(y)[i] = make_float4(elu1(v.x), elu1(v.y), elu1(v.z), elu1(v.w));
        }
        for (long i = 4 * nv + i0; i < n; i += stride) y[i] = elu1(x[i]);
    } else {
        for (long i = i0; i < n; i += stride) y[i] = elu1(x[i]);
    }
}

inline unsigned glue_grid(long items) {
    const long b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

extern "C" {

// up[n][Y][X][c] = bilinear(lo)[n][Y][X][c] on the (2 h) x (2 w) grid, align_corners = True (source coordinate Y (h - 1) / (2 h - 1));
// skip_out[n][Y][X][c] = skip[n][Y - top][X - left][c] inside the skip map and 0 outside, top = (2 h - hs) / 2, left = (2 w - ws) / 2
// (F.pad(skip, (left, 2 w - ws - left, top, 2 h - hs - top))).  lo [N][h][w][C], up [N][2h][2w][C], skip [N][hs][ws][Cs], skip_out
// [N][2h][2w][Cs]: fp32 NHWC, 16-byte aligned, C % 4 == 0, Cs % 4 == 0, hs <= 2 h, ws <= 2 w.  lo / up NULL: the pad alone; skip /
// skip_out NULL: the upsampling alone.  Outputs alias no input.
int far_upsample2x_pad_f32(const float* lo, long N, int h, int w, int C, float* up, const float* skip, int hs, int ws, int Cs,
                           float* skip_out, hipStream_t stream) {
    far_clear_errors();
    if (N == 0) return FAR_OK;
    const bool do_up = lo || up, do_pad = skip || skip_out;
    auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    if (N < 0 || h <= 0 || w <= 0 || h > (1 << 14) || w > (1 << 14) || (!do_up && !do_pad)) return FAR_EINVAL;
    if (do_up && (!lo || !up || lo == up || C <= 0 || (C & 3) || misaligned(lo) || misaligned(up))) return FAR_EINVAL;
    if (do_pad && (!skip || !skip_out || skip == skip_out || Cs <= 0 || (Cs & 3) || hs <= 0 || ws <= 0 || hs > 2 * h || ws > 2 * w ||
                   misaligned(skip) || misaligned(skip_out) || skip_out == up || skip_out == lo || up == skip))
        return FAR_EINVAL;
    const long pix = N * (2L * h) * (2L * w);
    const long n_up = do_up ? pix * (C / 4) : 0, n_pad = do_pad ? pix * (Cs / 4) : 0;
    hipLaunchKernelGGL(k_upsample2x_pad, dim3(glue_grid(n_up + n_pad)), dim3(256), 0, stream, (const float4*)lo, h, w, do_up ? C / 4 : 1, n_up,
                       (float4*)up, (const float4*)skip, hs, ws, do_pad ? Cs / 4 : 1, do_pad ? (2 * h - hs) / 2 : 0,
                       do_pad ? (2 * w - ws) / 2 : 0, n_up + n_pad, (float4*)skip_out);
    return far_check_launch();
}

// y[i] = x[i] > 0 ? x[i] : exp(x[i]) - 1 (F.elu, alpha 1) for n fp32 values; y may be x.
int far_elu_f32(const float* x, long n, float* y, hipStream_t stream) {
    far_clear_errors();
    if (n == 0) return FAR_OK;
    if (!x || !y || n < 0) return FAR_EINVAL;
    const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    hipLaunchKernelGGL(k_elu, dim3(glue_grid(vec ? (n + 3) / 4 : n)), dim3(256), 0, stream, x, n, y, vec);
    return far_check_launch();
}

}  // extern "C"
