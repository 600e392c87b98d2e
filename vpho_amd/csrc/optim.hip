// Optimiser tail of the training step (lib/engine/train_diff_hand_obj.py:49-54,182-185): the global gradient norm of
// accel.clip_grad_norm_ as ONE fixed-order fp64 reduction that stays on the device, and the Adam / AdamW update of every tensor as ONE
// launch that forms the clip coefficient itself -- the gradient buffer is read twice and never written, nothing comes back to the host.
// Both kernels are HBM-bound: 4 B per element for the norm, 28 B per element for the update.
#include "common.h"
#include "../../include/vpho_hip.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

// ---- sum of squares ------------------------------------------------------------------------------------------------------------------
// The buffer is split into a scalar head (up to the first 16-byte boundary), nv float4 vectors and a scalar tail.  The grid depends on n
// alone: min(SQN_MAX_BLOCKS, ceil(nv / SQN_THREADS)) workgroups, workgroup b owns the contiguous vectors [b * per, (b + 1) * per), a
// thread walks them in rounds of SQN_THREADS vectors.  Thread 0 of workgroup 0 starts from the head and tail elements.  Lanes are folded
// by a butterfly, waves in ascending order, the partials by one thread in ascending index: no atomics, the same bits on every run.
constexpr int SQN_THREADS = 256;
constexpr int SQN_MAX_BLOCKS = 1024;

struct SqnPlan { int head; long long nv; int tail; int blocks; long long per; };

inline SqnPlan sqn_plan(const float* g, long long n) {
    SqnPlan p;
    p.head = (int)std::min<long long>(n, (long long)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) / 4));
    p.nv = (n - p.head) / 4;
    p.tail = (int)(n - p.head - 4 * p.nv);
    p.blocks = (int)std::max<long long>(1, std::min<long long>(SQN_MAX_BLOCKS, (p.nv + SQN_THREADS - 1) / SQN_THREADS));
    p.per = (p.nv + p.blocks - 1) / p.blocks;
    return p;
}

__device__ inline double sq4(double acc, const float4 t) {
    // a float squared is exact in fp64, so each line rounds once (the addition)
    acc += (double)t.x * (double)t.x;
    acc += (double)t.y * (double)t.y;
    acc += (double)t.z * (double)t.z;
    acc += (double)t.w * (double)t.w;
    return acc;
}

__global__ __launch_bounds__(SQN_THREADS) void grad_sqnorm_kernel(const float* __restrict__ g, int head, long long nv, int tail, long long per,
                                                                  double* __restrict__ partial) {
    __shared__ double wave_sum[SQN_THREADS / 64];
    const float4* __restrict__ gv = reinterpret_cast<const float4*>(g + head);
    const long long lo = (long long)blockIdx.x * per, hi = lo + per < nv ? lo + per : nv;
    double acc = 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int i = 0; i < head; ++i) acc += (double)g[i] * (double)g[i];
        const float* t = g + head + 4 * nv;
        for (int i = 0; i < tail; ++i) acc += (double)t[i] * (double)t[i];
    }
    long long i = lo + threadIdx.x;
    for (; i + 3 * SQN_THREADS < hi; i += 4 * SQN_THREADS) {         // four loads in flight per thread
        const float4 a = gv[i], b = gv[i + SQN_THREADS], c = gv[i + 2 * SQN_THREADS], d = gv[i + 3 * SQN_THREADS];
        acc = sq4(sq4(sq4(sq4(acc, a), b), c), d);
    }
    for (; i < hi; i += SQN_THREADS) acc = sq4(acc, gv[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
#pragma unroll
        for (int w = 1; w < SQN_THREADS / 64; ++w) s += wave_sum[w];
        partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(SQN_THREADS) void grad_sqnorm_finish_kernel(const double* __restrict__ partial, int n, double* __restrict__ out) {
    __shared__ double p[SQN_MAX_BLOCKS];
    for (int i = threadIdx.x; i < n; i += SQN_THREADS) p[i] = partial[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += p[i];
        *out = s;
    }
}

// ---- the update ----------------------------------------------------------------------------------------------------------------------
// Segment table and block ownership of adamw_multi_kernel (train_score.hip): a block updates 1024 consecutive elements of one tensor.
// kind 0: torch.optim.AdamW, the expressions of adamw_multi_kernel one by one.  kind 1: torch.optim.Adam with L2 decay (g += wd * p).
// CLIP: every thread forms the coefficient of torch.nn.utils.clip_grad_norm_ from the device-resident sum of squares (fp64, rounded
// once); a coefficient of 1.0f multiplies exactly, so an unclipped step has the bits of a step without a norm.
// The segments of the flat gradient start at arbitrary 4-byte offsets: a block whose four base pointers are 16-byte aligned and which
// owns 1024 whole elements moves float4s, every other block takes the scalar path.
struct OptimSeg { float* p; const float* g; float* m; float* v; long long n; long long blk0; };

struct OptimArgs { float lr, beta1, beta2, eps, wd, step_size, sqrt_bc2, grad_scale; const double* sqnorm; float max_norm; };

template <int KIND, bool CLIP>
__device__ inline void optim_one(float& p, const float g, float& m, float& v, const OptimArgs& a, const float coef) {
    float gr = g * a.grad_scale;
    if constexpr (CLIP) gr = gr * coef;
    float w;
    if constexpr (KIND == 0) {
        w = p * (1.f - a.lr * a.wd);
    } else {
        w = p;
        gr = gr + a.wd * p;
    }
    const float mi = a.beta1 * m + (1.f - a.beta1) * gr;
    const float vi = a.beta2 * v + (1.f - a.beta2) * gr * gr;
    m = mi; v = vi;
    const float denom = sqrtf(vi) / a.sqrt_bc2 + a.eps;
    p = w - a.step_size * (mi / denom);
}

template <int KIND, bool CLIP>
__global__ __launch_bounds__(256) void optim_multi_kernel(const OptimSeg* __restrict__ segs, int nseg, const OptimArgs a) {
    int lo = 0, hi = nseg - 1;
    const long long b = blockIdx.x;
    while (lo < hi) {                                   // last segment with blk0 <= b
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    const OptimSeg sg = segs[lo];
    const long long base = (b - sg.blk0) * 1024;
    float coef = 1.f;
    if constexpr (CLIP) {
        // clip_coef = max_norm / (total_norm + 1e-6), clamped to 1 (a NaN stays a NaN, as torch.clamp keeps it)
        const double norm = (double)a.grad_scale * sqrt(*a.sqnorm);
        const double c = (double)a.max_norm / (norm + 1e-6);
        coef = (float)(c > 1.0 ? 1.0 : c);
    }
    const uintptr_t bits = reinterpret_cast<uintptr_t>(sg.p) | reinterpret_cast<uintptr_t>(sg.g) | reinterpret_cast<uintptr_t>(sg.m) |
                           reinterpret_cast<uintptr_t>(sg.v);
    if ((bits & 15) == 0 && base + 1024 <= sg.n) {
        const long long i = base + 4 * threadIdx.x;
        float4 p = *reinterpret_cast<const float4*>(sg.p + i), m = *reinterpret_cast<const float4*>(sg.m + i), v = *reinterpret_cast<const float4*>(sg.v + i);
        const float4 g = *reinterpret_cast<const float4*>(sg.g + i);
        optim_one<KIND, CLIP>(p.x, g.x, m.x, v.x, a, coef);
        optim_one<KIND, CLIP>(p.y, g.y, m.y, v.y, a, coef);
        optim_one<KIND, CLIP>(p.z, g.z, m.z, v.z, a, coef);
        optim_one<KIND, CLIP>(p.w, g.w, m.w, v.w, a, coef);
        *reinterpret_cast<float4*>(sg.m + i) = m;
        *reinterpret_cast<float4*>(sg.v + i) = v;
        *reinterpret_cast<float4*>(sg.p + i) = p;
        return;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long i = base + u * 256 + threadIdx.x;
        if (i >= sg.n) continue;
        float p = sg.p[i], m = sg.m[i], v = sg.v[i];
        optim_one<KIND, CLIP>(p, sg.g[i], m, v, a, coef);
        sg.m[i] = m; sg.v[i] = v; sg.p[i] = p;
    }
}

}  // namespace

extern "C" long long vpho_grad_sqnorm_workspace_bytes(long long n) {
    if (n <= 0) return -1;
    return (long long)sizeof(double) * std::min<long long>(SQN_MAX_BLOCKS, (n / 4 + SQN_THREADS - 1) / SQN_THREADS + 1);
}

extern "C" int vpho_grad_sqnorm_f64(const float* grad, long long n, double* out, void* workspace, void* stream) {
    VPHO_REQUIRE(grad && out && workspace && n > 0 && (reinterpret_cast<uintptr_t>(grad) & 3) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                 "vpho_grad_sqnorm_f64: bad argument");
    const SqnPlan p = sqn_plan(grad, n);
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(p.blocks), dim3(SQN_THREADS), 0, (hipStream_t)stream, grad, p.head, p.nv, p.tail, p.per, (double*)workspace);
    hipLaunchKernelGGL(grad_sqnorm_finish_kernel, dim3(1), dim3(SQN_THREADS), 0, (hipStream_t)stream, (const double*)workspace, p.blocks, out);
    return vpho::check_launch("grad_sqnorm kernels");
}

extern "C" int vpho_optim_multi_f32(const void* segments, int n_segments, long long total_blocks, int kind, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, int step, float grad_scale, const double* sqnorm, float max_norm, void* stream) {
    VPHO_REQUIRE(segments && n_segments > 0 && total_blocks > 0 && total_blocks < (1ll << 31) && step >= 1 && (kind == 0 || kind == 1) &&
                 (!sqnorm || max_norm > 0.f), "vpho_optim_multi_f32: bad argument");
    static_assert(sizeof(OptimSeg) == 48, "segment record = 4 pointers + 2 int64");
    // bias corrections in double on the host, as torch.optim computes them (python floats)
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const OptimArgs a{lr, beta1, beta2, eps, weight_decay, (float)((double)lr / bc1), (float)std::sqrt(bc2), grad_scale, sqnorm, max_norm};
    const dim3 grid((unsigned)total_blocks), block(256);
    const OptimSeg* segs = (const OptimSeg*)segments;
    hipStream_t s = (hipStream_t)stream;
    if (kind == 0 && !sqnorm) hipLaunchKernelGGL((optim_multi_kernel<0, false>), grid, block, 0, s, segs, n_segments, a);
    else if (kind == 0) hipLaunchKernelGGL((optim_multi_kernel<0, true>), grid, block, 0, s, segs, n_segments, a);
    else if (!sqnorm) hipLaunchKernelGGL((optim_multi_kernel<1, false>), grid, block, 0, s, segs, n_segments, a);
    else hipLaunchKernelGGL((optim_multi_kernel<1, true>), grid, block, 0, s, segs, n_segments, a);
    return vpho::check_launch("optim_multi_kernel");
}
