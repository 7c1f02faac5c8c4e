// K20: AdamW for all parameters of a model in ONE launch (training step of BASELINE configs[2]).
//
// Replaces the multi-tensor kernels of torch.optim.AdamW (mp3d_loftr/src/optimizers/__init__.py:5-16 builds it; ~30 launches per
// step for the 189 parameter tensors) with the same arithmetic in the same order, element by element:
//     p   *= 1 - lr wd
//     m    = m + (1 - beta1) (g - m)                               (torch's lerp)
//     v    = beta2 v + (1 - beta2) g g
//     p   -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)             bc_i = 1 - beta_i^step
// A device table holds one row per tensor {p, g, m, v, n} and one {tensor, chunk} pair per workgroup (4096 elements each); the
// gradient pointers are refreshed every step (autograd re-allocates them), the rest is built once.
//
// The same table serves the rest of the reference's optimizer step: gradient clipping by the global norm (every training run of the
// reference passes gradient_clip_val = 0.5 to its trainer) as a deterministic two-launch reduction whose coefficient stays on the
// device and is applied inside the update (k_adamw<CLIP = true>: no pass that rescales the gradients), torch.optim.Adam's coupled
// decay (COUPLED), and a device-side "skip the update when the norm is not finite".
#include "common.h"

namespace {

struct AdamRow {
    float* p;
    const float* g;
    float* m;
    float* v;
    long n;
};

constexpr int ADAM_CHUNK = 4096;

// What the finalize kernel leaves for the update and scale kernels (the head of the clipping workspace; the float64 partials follow
// at byte CLIP_HEAD_BYTES).  skipped is the only word that outlives a step: the workspace arrives zeroed.
struct ClipResult {
    float norm;        // the global gradient norm, rounded to fp32 once
    float coef;        // min(max_norm / (norm + 1e-6), 1) with torch's NaN semantics: a NaN norm gives a NaN coefficient
    int nonfinite;     // norm is NaN or inf
    int skipped;       // steps counted as skipped so far (count_skipped launches that saw nonfinite)
};
constexpr long CLIP_HEAD_BYTES = 64;

// CLIP: the gradient is scaled by the device-side coefficient on its way in (gc = g coef, rounded to fp32 as an operation of its own:
// the same bits as k_grad_scale followed by the plain kernel); with skip != 0 a non-finite norm leaves p, m, v alone.
// COUPLED: torch.optim.Adam -- L2 decay added to the gradient (gc += wd p) instead of p *= 1 - lr wd.
// k_adamw<false, false> is the kernel of far_adamw_step_f32 (wd, clip, skip unused).
template <bool CLIP, bool COUPLED>
__global__ __launch_bounds__(256) void k_adamw(const AdamRow* __restrict__ rows, const int2* __restrict__ blocks, float decay, float w1,
                                               float beta2, float w2, float step, float bc2_sqrt, float eps, float wd,
                                               const ClipResult* __restrict__ clip, int skip) {
    const int2 b = blocks[blockIdx.x];
    const AdamRow r = rows[b.x];
    if (!r.g) return;                                   // a parameter without a gradient this step is left alone (as torch does)
    float coef = 1.0f;
    if (CLIP) {
        if (skip && clip->nonfinite) return;
        coef = clip->coef;
    }
    const long base = (long)b.y * ADAM_CHUNK;
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
        const long i = base + k * 256 + threadIdx.x;
        if (i >= r.n) break;
        float g = r.g[i];
        if (CLIP) g = __fmul_rn(g, coef);               // never contracted into g - m below
        float p = r.p[i];
        if (COUPLED) {
            if (wd != 0.0f) g = fmaf(wd, p, g);          // grad.add(param, alpha = wd): one rounding, as ATen's a + alpha * b compiles (fma)
        } else {
            p = p * decay;
        }
        float m = r.m[i];
        m = m + w1 * (g - m);
        float v = r.v[i] * beta2;
        v = v + (w2 * g) * g;                           // addcmul: value * tensor1 * tensor2, left to right
        const float denom = __builtin_sqrtf(v) / bc2_sqrt + eps;
        p = p - step * (m / denom);
        r.p[i] = p; r.m[i] = m; r.v[i] = v;
    }
}

// ---- the global gradient norm: deterministic (fixed-order trees, no atomics), float64 accumulation of exact squares.
// INF = false: sum; INF = true: max with NaN kept (fmax would drop it).
template <bool INF>
__device__ __forceinline__ double norm_combine(double a, double b) {
    if (!INF) return a + b;
    return (a != a) ? a : ((b != b) ? b : (a > b ? a : b));
}

// The workgroup's NW waves -> one value, the same in every thread: an xor tree inside each wave, then the waves in index order.
template <bool INF, int NW>
__device__ __forceinline__ double norm_block_reduce(double x, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = norm_combine<INF>(x, __shfl_xor(x, o, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = lds[0];
    for (int w = 1; w < NW; ++w) t = norm_combine<INF>(t, lds[w]);
    return t;
}

// One workgroup per {tensor, chunk} pair (k_adamw's grid): partials[blockIdx.x] = sum g^2 (or max |g|) of the chunk; 0 for a row
// without a gradient.  One dword per lane, coalesced, as k_adamw reads them (a gradient is only known to be 4-byte aligned).
template <bool INF>
__global__ __launch_bounds__(256) void k_grad_norm_partial(const AdamRow* __restrict__ rows, const int2* __restrict__ blocks,
                                                           double* __restrict__ partials) {
    __shared__ double lds[4];
    const int2 b = blocks[blockIdx.x];
    const AdamRow r = rows[b.x];
    double acc = 0.0;
    if (r.g) {                                          // uniform over the workgroup
        const long base = (long)b.y * ADAM_CHUNK;
        float mx = 0.0f;
        bool nan = false;
        // all loads of the chunk first, then the arithmetic: an element past the end reads as 0, which changes neither a sum nor a max
        float x[ADAM_CHUNK / 256];
        if (base + ADAM_CHUNK <= r.n) {
#pragma unroll
            for (int k = 0; k < ADAM_CHUNK / 256; ++k) x[k] = r.g[base + k * 256 + threadIdx.x];
        } else {
#pragma unroll
            for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
                const long i = base + k * 256 + threadIdx.x;
                x[k] = i < r.n ? r.g[i] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
            if (INF) {
                const float a = __builtin_fabsf(x[k]);
                nan = nan || (a != a);
                mx = a > mx ? a : mx;
            } else {
                const double d = (double)x[k];
                acc = acc + d * d;                      // the square of an fp32 value is exact in float64
            }
        }
        if (INF) acc = nan ? (double)__builtin_nanf("") : (double)mx;
    }
    const double t = norm_block_reduce<INF, 4>(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// One workgroup of 1024: every lane strides over the partials in index order, then the same fixed tree.
template <bool INF>
__global__ __launch_bounds__(1024) void k_grad_norm_finalize(const double* __restrict__ partials, long total, float max_norm,
                                                             int count_skipped, ClipResult* __restrict__ res) {
    __shared__ double lds[16];
    double acc = 0.0;
    for (long i = threadIdx.x; i < total; i += 1024) acc = norm_combine<INF>(acc, partials[i]);
    const double t = norm_block_reduce<INF, 16>(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = INF ? (float)t : (float)__builtin_sqrt(t);
        // torch: clip_coef = max_norm / (total_norm + 1e-6) is Tensor.__rtruediv__ = reciprocal() * max_norm, in fp32; then
        // clamp(max = 1), which keeps a NaN (fminf would return 1)
        float coef = __fmul_rn(1.0f / (norm + 1e-6f), max_norm);
        coef = coef > 1.0f ? 1.0f : coef;
        const int bad = !(__builtin_fabsf(norm) <= FLT_MAX);       // NaN or inf
        res->norm = norm;
        res->coef = coef;
        res->nonfinite = bad;
        if (count_skipped && bad) res->skipped = res->skipped + 1;
    }
}

// g *= coef in place over the table (the stand-alone clip_grad_norm_).
__global__ __launch_bounds__(256) void k_grad_scale(const AdamRow* __restrict__ rows, const int2* __restrict__ blocks,
                                                    const ClipResult* __restrict__ clip) {
    const int2 b = blocks[blockIdx.x];
    const AdamRow r = rows[b.x];
    if (!r.g) return;
    const float coef = clip->coef;
    float* g = const_cast<float*>(r.g);
    const long base = (long)b.y * ADAM_CHUNK;
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
        const long i = base + k * 256 + threadIdx.x;
        if (i >= r.n) break;
        g[i] = __fmul_rn(g[i], coef);
    }
}

inline bool table_args_ok(const void* table, int n, long nblocks) { return table && n > 0 && nblocks > 0 && nblocks <= 0x7fffffffL; }

}  // namespace

extern "C" {

// Bytes of the device table for n tensors with `nblocks` = sum over tensors of ceil(numel / 4096) workgroups.
long far_adamw_table_bytes(int n, long nblocks) {
    if (n <= 0 || nblocks <= 0) return 0;
    return (long)n * (long)sizeof(AdamRow) + nblocks * (long)sizeof(int2);
}

// One AdamW step over the table: rows = table, blocks = table + n rows.  bc1 = 1 - beta1^step, bc2_sqrt = sqrt(1 - beta2^step).
// Hyper-parameters in double: the derived scalars (1 - lr wd, 1 - beta, lr / bc1) are formed in double and rounded once, as torch does.
int far_adamw_step_f32(const void* table, int n, long nblocks, double lr, double beta1, double beta2, double eps, double wd, double bc1,
                       double bc2_sqrt, hipStream_t stream) {
    far_clear_errors();
    if (!table || n <= 0 || nblocks <= 0 || nblocks > 0x7fffffffL || !(bc1 > 0.0) || !(bc2_sqrt > 0.0)) return FAR_EINVAL;
    const AdamRow* rows = reinterpret_cast<const AdamRow*>(table);
    const int2* blocks = reinterpret_cast<const int2*>(rows + n);
    // the derived scalars in double, rounded once, as torch passes them to its kernels
    hipLaunchKernelGGL((k_adamw<false, false>), dim3((unsigned)nblocks), dim3(256), 0, stream, rows, blocks, (float)(1.0 - lr * wd),
                       (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1), (float)bc2_sqrt, (float)eps, 0.0f,
                       (const ClipResult*)nullptr, 0);
    return far_check_launch();
}

// Bytes of the clipping workspace for `nblocks` partials: the result block { float norm; float coef; int nonfinite; int skipped; }
// at byte 0, the float64 partials from byte 64.  The caller zeroes it once (the skipped counter lives in it).
size_t far_grad_norm_workspace_bytes(long nblocks) {
    if (nblocks <= 0) return 0;
    return (size_t)CLIP_HEAD_BYTES + (size_t)nblocks * sizeof(double);
}

// The global gradient norm of a table (norm_type 2 or +inf) in two launches: one float64 partial per workgroup into
// partials[first .. first + nblocks), then -- when total > 0 -- one workgroup that combines partials[0 .. total) in a fixed order and
// writes the result block.  Several tables (parameter groups) share one norm: each passes its `first`, the last one `total`.
int far_grad_norm_f32(const void* table, int n, long nblocks, long first, long total, double norm_type, double max_norm,
                      int count_skipped, void* workspace, hipStream_t stream) {
    far_clear_errors();
    const bool inf = norm_type > DBL_MAX;
    if (!table_args_ok(table, n, nblocks) || !workspace || first < 0 || total < 0 || (total > 0 && total < first + nblocks) ||
        !(inf || norm_type == 2.0) || !(max_norm > 0.0))
        return FAR_EINVAL;
    const AdamRow* rows = reinterpret_cast<const AdamRow*>(table);
    const int2* blocks = reinterpret_cast<const int2*>(rows + n);
    ClipResult* res = reinterpret_cast<ClipResult*>(workspace);
    double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + CLIP_HEAD_BYTES);
    if (inf) hipLaunchKernelGGL(k_grad_norm_partial<true>, dim3((unsigned)nblocks), dim3(256), 0, stream, rows, blocks, partials + first);
    else hipLaunchKernelGGL(k_grad_norm_partial<false>, dim3((unsigned)nblocks), dim3(256), 0, stream, rows, blocks, partials + first);
    if (total > 0) {
        const float mn = (float)max_norm;
        if (inf) hipLaunchKernelGGL(k_grad_norm_finalize<true>, dim3(1), dim3(1024), 0, stream, partials, total, mn, count_skipped, res);
        else hipLaunchKernelGGL(k_grad_norm_finalize<false>, dim3(1), dim3(1024), 0, stream, partials, total, mn, count_skipped, res);
    }
    return far_check_launch();
}

// g *= coef in place for every row with a gradient; coef from the workspace far_grad_norm_f32 filled.
int far_grad_clip_scale_f32(const void* table, int n, long nblocks, const void* workspace, hipStream_t stream) {
    far_clear_errors();
    if (!table_args_ok(table, n, nblocks) || !workspace) return FAR_EINVAL;
    const AdamRow* rows = reinterpret_cast<const AdamRow*>(table);
    const int2* blocks = reinterpret_cast<const int2*>(rows + n);
    hipLaunchKernelGGL(k_grad_scale, dim3((unsigned)nblocks), dim3(256), 0, stream, rows, blocks, reinterpret_cast<const ClipResult*>(workspace));
    return far_check_launch();
}

// far_adamw_step_f32 with two switches: coupled != 0 is torch.optim.Adam (L2 decay added to the gradient); clip_workspace != NULL
// scales every gradient by the workspace's coefficient on its way in and, with skip_nonfinite != 0, leaves p, m, v untouched when the
// norm was NaN or inf.  coupled = 0 and clip_workspace = NULL is far_adamw_step_f32.
int far_adam_step_f32(const void* table, int n, long nblocks, double lr, double beta1, double beta2, double eps, double wd, double bc1,
                      double bc2_sqrt, int coupled, const void* clip_workspace, int skip_nonfinite, hipStream_t stream) {
    far_clear_errors();
    if (!table_args_ok(table, n, nblocks) || !(bc1 > 0.0) || !(bc2_sqrt > 0.0) || (skip_nonfinite && !clip_workspace)) return FAR_EINVAL;
    const AdamRow* rows = reinterpret_cast<const AdamRow*>(table);
    const int2* blocks = reinterpret_cast<const int2*>(rows + n);
    const ClipResult* clip = reinterpret_cast<const ClipResult*>(clip_workspace);
    const dim3 grid((unsigned)nblocks), block(256);
    const float decay = (float)(1.0 - lr * wd), w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2),
                step = (float)(lr / bc1), bs = (float)bc2_sqrt, e = (float)eps, wdf = (float)wd;
#define FAR_ADAM_LAUNCH(CLIP, COUPLED) \
    hipLaunchKernelGGL((k_adamw<CLIP, COUPLED>), grid, block, 0, stream, rows, blocks, decay, w1, b2, w2, step, bs, e, wdf, clip, skip_nonfinite)
    if (clip && coupled) FAR_ADAM_LAUNCH(true, true);
    else if (clip) FAR_ADAM_LAUNCH(true, false);
    else if (coupled) FAR_ADAM_LAUNCH(false, true);
    else FAR_ADAM_LAUNCH(false, false);
#undef FAR_ADAM_LAUNCH
    return far_check_launch();
}

}  // extern "C"
