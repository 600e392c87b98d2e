// Exponential moving average of the trained weights (lib/model/ema.py:25-44, ExponentialMovingAverage.update): every shadow tensor of
// the training step moves towards its parameter in ONE launch, next to the optimiser tail (optim.hip).  HBM-bound: 12 B per element
// (parameter read, shadow read and written).
#include "common.h"
#include "../../include/vpho_hip.h"
#include <cstdint>

namespace {

// Segment table and block ownership of optim_multi_kernel (optim.hip): a block updates 1024 consecutive elements of one tensor.
struct EmaSeg { const float* p; float* s; long long n; long long blk0; };

// s.sub_(one_minus_decay * (s - p)) as torch runs it: three fp32 operations, each rounded once.  A contracted multiply-subtract
// (fma(-omd, d, s)) rounds once less and differs in the last bit on about one element in 700, so contraction is switched off HERE,
// whatever the translation unit is compiled with: the pragma covers the front end and -ffp-contract=fast-honor-pragmas (hipcc's
// default), the empty asm makes the rounded product opaque to a back end that fuses across statements under -ffp-contract=fast.
// NaN and infinities propagate as IEEE gives them.
__device__ __forceinline__ float ema_one(const float s, const float p, const float omd) {
#pragma clang fp contract(off)
    const float d = s - p;
    float t = omd * d;
    asm volatile("" : "+v"(t));
    return s - t;
}

__global__ __launch_bounds__(256) void ema_multi_kernel(const EmaSeg* __restrict__ segs, int nseg, const float omd) {
    int lo = 0, hi = nseg - 1;
    const long long b = blockIdx.x;
    while (lo < hi) {                                   // last segment with blk0 <= b
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    const EmaSeg sg = segs[lo];
    const long long base = (b - sg.blk0) * 1024;
    // the tensors start at arbitrary 4-byte offsets: a block whose two base pointers are 16-byte aligned and which owns 1024 whole
    // elements moves float4s, every other block takes the scalar path
    const uintptr_t bits = reinterpret_cast<uintptr_t>(sg.p) | reinterpret_cast<uintptr_t>(sg.s);
    if ((bits & 15) == 0 && base + 1024 <= sg.n) {
        const long long i = base + 4 * threadIdx.x;
        const float4 p = *reinterpret_cast<const float4*>(sg.p + i);
        float4 s = *reinterpret_cast<const float4*>(sg.s + i);
        s.x = ema_one(s.x, p.x, omd);
        s.y = ema_one(s.y, p.y, omd);
        s.z = ema_one(s.z, p.z, omd);
        s.w = ema_one(s.w, p.w, omd);
        *reinterpret_cast<float4*>(sg.s + i) = s;
        return;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long i = base + u * 256 + threadIdx.x;
        if (i < 0 || i >= sg.n) continue;
        sg.s[i] = ema_one(sg.s[i], sg.p[i], omd);
    }
}

}  // namespace

extern "C" int vpho_ema_multi_f32(const void* table, int n_tensors, long long blocks, float one_minus_decay, void* stream) {
    VPHO_REQUIRE(n_tensors >= 0 && blocks >= 0 && blocks < (1ll << 31) && (table || n_tensors == 0), "vpho_ema_multi_f32: bad argument");
    static_assert(sizeof(EmaSeg) == 32, "segment record = 2 pointers + 2 int64");
    if (n_tensors == 0 || blocks == 0) return 0;        // nothing to average: no launch
    hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const EmaSeg*)table, n_tensors, one_minus_decay);
    return vpho::check_launch("ema_multi_kernel");
}
