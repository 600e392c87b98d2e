// Symmetry-aware object pose errors for every sampled hypothesis (--eval_symmetric): SMCE, the symmetric mean corner
// error of TesterObject.criterion_SMCE (lib/engine/test.py:377-398, whose call at :258 is commented out as "very slow"), over the padded
// symmetry table of TesterObject.__init__ (:204-226, get_symmetry_transformations :103-150), and MSSD, the BOP toolkit's maximum
// symmetry-aware surface distance over the same table and the sampled vertices of criterion_ADD_REP (:425-458).
//   per (hypothesis, k):  D_k = P - G S_k  (one 3x4 affine map),  SMCE = min_k mean_c |D_k c|,  MSSD = min_k max_v |D_k v|
// One 256-thread workgroup per (image, hypothesis).  The vertices are staged in LDS once (2048 points = 48 KB of fp64; every lane reads
// the same vertex: a broadcast); lane l owns the symmetries l, l + 256, ... and keeps its running maximum of the SQUARED distance, one
// square root is taken at the very end.  Pruning is exact: a lane abandons symmetry k once its running maximum has reached the smallest
// COMPLETED maximum of an earlier round of 256 (reduced by wave shuffles and LDS between the rounds): the abandoned k's full maximum is
// no smaller than that bound, so it cannot be the minimum, and what the lane hands on for it (the partial maximum) is no smaller
// either.  No float atomics, nothing depends on workgroup order; prune = 0 runs every pair in full and returns the same bits.
#include "common.h"
#include "../../include/vpho_hip.h"

#include <cfloat>

namespace {

constexpr int OS_LDS_PTS = 2048;                   // vertices kept in LDS; the rest of a longer table is read from memory
constexpr int OS_MAX_K = 4096;                     // symmetries per object
constexpr int OS_STEP = 8;                         // vertices between two looks at the pruning bound

__device__ inline double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

// minimum over the 256 threads, every thread gets the same bits (no NaN reaches it: non-finite poses leave before)
__device__ inline double block_min(double v, double* red) {
    v = wave_min(v);
    __syncthreads();                               // the previous round's reads of red are over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
}

__device__ inline bool finite64(double x) { return fabs(x) <= DBL_MAX; }

// squared length of a x + b for the 3x4 map (a | b), products contracted in a fixed order
__device__ inline double dist2(const double (&a)[9], const double (&b)[3], double x, double y, double z) {
    const double dx = fma(a[0], x, fma(a[1], y, fma(a[2], z, b[0])));
    const double dy = fma(a[3], x, fma(a[4], y, fma(a[5], z, b[1])));
    const double dz = fma(a[6], x, fma(a[7], y, fma(a[8], z, b[2])));
    return fma(dx, dx, fma(dy, dy, dz * dz));
}

__global__ __launch_bounds__(256) void obj_symmetry_multi_kernel(const vpho_obj_symmetry_tables t, const double* __restrict__ pd_rt,
                                                                 const double* __restrict__ gt_rt, const int* __restrict__ obj_id, int S,
                                                                 int prune, double* __restrict__ per) {
    __shared__ double pts[OS_LDS_PTS * 3];
    __shared__ double corner[24];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const long long bs = blockIdx.x;
    const int b = (int)(bs / S);
    double* out = per + bs * 3;
    const int id = obj_id[b];
    double p[12], g[12];
    bool ok = id >= 0 && id < t.n_obj;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        p[i] = pd_rt[bs * 12 + i];
        g[i] = gt_rt[(long long)b * 12 + i];
        ok = ok && finite64(p[i]) && finite64(g[i]);
    }
    if (!ok) {                                     // the same for every thread: nobody is left waiting at a barrier
        if (tid == 0) {
            out[0] = out[1] = __longlong_as_double(0x7ff8000000000000LL);
            out[2] = 0.0;
        }
        return;
    }
    const int nv = t.n_sampled;
    const int nl = nv < OS_LDS_PTS ? nv : OS_LDS_PTS;
    const int nl8 = (nl + OS_STEP - 1) / OS_STEP * OS_STEP;          // <= OS_LDS_PTS; the tail repeats vertex 0, which changes no maximum
    const double* vs = t.verts_sampled + (long long)id * nv * 3;
    for (int i = tid; i < nl8 * 3; i += 256) pts[i] = vs[i < nl * 3 ? i : i % 3];
    if (tid < 24) corner[tid] = t.bbox3d[(long long)id * 24 + tid];
    __syncthreads();

    const int K = t.K;
    const double* sR = t.sym_R + (long long)id * K * 9;
    const double* sT = t.sym_t + (long long)id * K * 3;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double bound = inf, lane_mssd = inf, lane_smce = inf;
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + tid;
        if (k < K) {
            double r[9], a[9], c[3];
#pragma unroll
            for (int i = 0; i < 9; ++i) r[i] = sR[(long long)k * 9 + i];
            const double t0 = sT[(long long)k * 3], t1 = sT[(long long)k * 3 + 1], t2 = sT[(long long)k * 3 + 2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    a[i * 3 + j] = p[i * 4 + j] - fma(g[i * 4], r[j], fma(g[i * 4 + 1], r[3 + j], g[i * 4 + 2] * r[6 + j]));
                c[i] = p[i * 4 + 3] - fma(g[i * 4], t0, fma(g[i * 4 + 1], t1, fma(g[i * 4 + 2], t2, g[i * 4 + 3])));
            }
            double sum = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) sum += sqrt(dist2(a, c, corner[q * 3], corner[q * 3 + 1], corner[q * 3 + 2]));
            lane_smce = fmin(lane_smce, sum * 0.125);
            double m = 0.0;
            int v = 0;
            for (; v < nl8; v += OS_STEP) {
#pragma unroll
                for (int u = 0; u < OS_STEP; ++u) m = fmax(m, dist2(a, c, pts[(v + u) * 3], pts[(v + u) * 3 + 1], pts[(v + u) * 3 + 2]));
                if (m >= bound) break;
            }
            if (v >= nl8)
                for (v = OS_LDS_PTS; v < nv && m < bound; ++v) m = fmax(m, dist2(a, c, vs[(long long)v * 3], vs[(long long)v * 3 + 1], vs[(long long)v * 3 + 2]));
            lane_mssd = fmin(lane_mssd, m);
        }
        if (k0 + 256 < K) {                        // uniform: K and k0 are
            const double done = block_min(lane_mssd, red);
            if (prune) bound = done;
        }
    }
    const double mssd = sqrt(block_min(lane_mssd, red));
    const double smce = block_min(lane_smce, red);
    if (tid == 0) {
        out[0] = smce;
        out[1] = mssd;
        out[2] = mssd < 0.1 * t.diameter[id] ? 1.0 : 0.0;
    }
}

// per image and value, in hypothesis order: hypothesis 0, best-of-S (TesterObject.postprocess: min of SMCE and MSSD, max of the hit) and
// mean-of-S (fp64 sum in ascending s); the comparisons are those of obj_multi_reduce_kernel, so a NaN hypothesis behaves as it does there
__global__ void obj_symmetry_table_kernel(const double* __restrict__ per, int n_img, int S, double* __restrict__ one, double* __restrict__ best,
                                          double* __restrict__ mean) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img * 3) return;
    const int b = i / 3, c = i % 3;
    const double* p = per + (long long)b * S * 3 + c;
    double bv = p[0], sv = p[0];
    for (int s = 1; s < S; ++s) {
        const double v = p[(long long)s * 3];
        bv = c == 2 ? (v > bv ? v : bv) : (v < bv ? v : bv);
        sv += v;
    }
    one[i] = p[0];
    best[i] = bv;
    mean[i] = sv / S;
}

}  // namespace

extern "C" int vpho_obj_symmetry_multi_f64(const vpho_obj_symmetry_tables* t, const double* pd_rt, const double* gt_rt, const int* obj_id,
                                           int n_img, int n_hyp, int prune, double* per, void* stream) {
    VPHO_REQUIRE(t && t->sym_R && t->sym_t && t->bbox3d && t->verts_sampled && t->diameter && t->n_obj > 0 && t->n_sampled > 0,
                 "vpho_obj_symmetry_multi_f64: bad tables");
    VPHO_REQUIRE(t->K >= 1 && t->K <= OS_MAX_K, "vpho_obj_symmetry_multi_f64: %d symmetry transforms per object, the kernel takes 1 .. %d", t->K,
                 OS_MAX_K);
    VPHO_REQUIRE(pd_rt && gt_rt && obj_id && per && n_img > 0 && n_hyp > 0, "vpho_obj_symmetry_multi_f64: bad argument");
    VPHO_REQUIRE((long long)n_img * n_hyp <= 0x7fffffffLL, "vpho_obj_symmetry_multi_f64: %d x %d pairs, at most 2^31 - 1 in one call", n_img, n_hyp);
    hipLaunchKernelGGL(obj_symmetry_multi_kernel, dim3(n_img * n_hyp), dim3(256), 0, (hipStream_t)stream, *t, pd_rt, gt_rt, obj_id, n_hyp,
                       prune != 0, per);
    return vpho::check_launch("obj_symmetry_multi_kernel");
}

extern "C" int vpho_obj_symmetry_table_f64(const double* per, int n_img, int n_hyp, double* one, double* best, double* mean, void* stream) {
    VPHO_REQUIRE(per && one && best && mean && n_img > 0 && n_hyp > 0 && (long long)n_img * 3 <= 0x7fffffffLL,
                 "vpho_obj_symmetry_table_f64: bad argument");
    hipLaunchKernelGGL(obj_symmetry_table_kernel, dim3((n_img * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, per, n_img, n_hyp, one, best,
                       mean);
    return vpho::check_launch("obj_symmetry_table_kernel");
}
