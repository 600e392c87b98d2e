// Hand benchmark metrics of the HO3D / FreiHAND leaderboards for every sampled hypothesis (nothing in the reference:
// the definitions are those of the leaderboards' eval.py): the AUC of the PCK curve over a threshold table and the F-score at two
// distances, each raw and after the similarity alignment of rigid_align_AtoB (lib/utils/transform_fn.py:43-66), per (hand, ground truth)
// pair.  One workgroup per pair: the points stay in LDS, the nearest-neighbour distances in registers, nothing but the 6 values (and on
// request 10 integer counts) goes to HBM.
#include "common.h"
#include "procrustes.h"
#include "../../include/vpho_hip.h"

namespace {

constexpr int HB_MAX_PTS = 1024;                   // points per set: three sets of x | y | z planes in LDS, 36 KB
constexpr int HB_MAX_THRESH = 256;                 // AUC table entries

// sums of N doubles over the 256 threads of a workgroup, every thread gets the same bits: xor butterfly inside a wave (vpho::wave_sum),
// then the four waves in ascending order
template <int N>
__device__ inline void block_sums(double (&v)[N], double (*red)[N]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = vpho::wave_sum(v[k]);
    __syncthreads();                               // the previous round's reads of red are over
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

__device__ inline int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// c = #{j : e <= t_j} of an ascending table = n_t - (index of the first entry >= e)
__device__ inline int pck_count(double e, const double* t, int n_t) {
    int lo = 0, hi = n_t;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] >= e) hi = mid; else lo = mid + 1;
    }
    return n_t - lo;
}

struct alignas(16) Planes { float x[HB_MAX_PTS], y[HB_MAX_PTS], z[HB_MAX_PTS]; };

// squared distance of q to the nearest of the m4 (a multiple of 4) points of a plane set; every lane reads the same addresses
__device__ inline float nearest_d2(const Planes& T, int m4, float qx, float qy, float qz) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    float best = INFINITY;
    const f32x2 vx = {qx, qx}, vy = {qy, qy}, vz = {qz, qz};
    for (int j = 0; j < m4; j += 4) {
#pragma clang fp contract(fast)
        const float4 tx = *reinterpret_cast<const float4*>(T.x + j), ty = *reinterpret_cast<const float4*>(T.y + j),
                     tz = *reinterpret_cast<const float4*>(T.z + j);
        const f32x2 ax = vx - f32x2{tx.x, tx.y}, ay = vy - f32x2{ty.x, ty.y}, az = vz - f32x2{tz.x, tz.y};
        const f32x2 bx = vx - f32x2{tx.z, tx.w}, by = vy - f32x2{ty.z, ty.w}, bz = vz - f32x2{tz.z, tz.w};
        const f32x2 da = az * az + (ay * ay + ax * ax), db = bz * bz + (by * by + bx * bx);
        best = fminf(best, fminf(da.x, da.y));
        best = fminf(best, fminf(db.x, db.y));
    }
    return best;
}

// One 256-thread workgroup per (image, hypothesis).  A = the hypothesis after the reference's postprocess (x un-flipped for left hands,
// root added, both in fp32: the bits hand_metrics_multi_kernel forms), B = the ground truth.  Errors, the alignment and the AUC counts
// in fp64 on those bits; for the F-scores A, the aligned A (fp64, rounded once) and B are centred on B's centroid before they are
// rounded to fp32, and the 4 P queries (raw | aligned) x (B -> X | X -> B) are dealt round-robin to the threads.
__global__ __launch_bounds__(256) void hand_bench_multi_kernel(const float* __restrict__ pd, const float* __restrict__ gt,
                                                               const float* __restrict__ root, const unsigned char* __restrict__ is_right,
                                                               int S, int n, double th_lo, double th_hi, const double* __restrict__ auc_t,
                                                               const double* __restrict__ auc_g, int n_t, int with_fscore,
                                                               double* __restrict__ values, int* __restrict__ counts) {
    __shared__ Planes sA, sH, sB;                                         // raw, aligned, ground truth
    __shared__ double s_t[HB_MAX_THRESH], s_g[HB_MAX_THRESH + 1];
    __shared__ double red[4][12];
    __shared__ int redi[4][10];
    const long long bs = blockIdx.x;
    const int b = (int)(bs / S), tid = threadIdx.x;
    const float* A = pd + bs * n * 3;
    const float* B = gt + (long long)b * n * 3;
    const float sg = is_right[b] ? 1.f : -1.f, r0 = root[b * 3], r1 = root[b * 3 + 1], r2 = root[b * 3 + 2];
    double* out = values + bs * 6;
    for (int j = tid; j < n_t; j += 256) s_t[j] = auc_t[j];
    for (int j = tid; j <= n_t; j += 256) s_g[j] = auc_g[j];
    // stage the exact fp32 points; a non-finite coordinate anywhere makes the whole row NaN
    int bad = 0;
    for (int i = tid; i < n; i += 256) {
        const float ax = A[i * 3] * sg + r0, ay = A[i * 3 + 1] + r1, az = A[i * 3 + 2] + r2;
        const float bx = B[i * 3], by = B[i * 3 + 1], bz = B[i * 3 + 2];
        sA.x[i] = ax; sA.y[i] = ay; sA.z[i] = az;
        sB.x[i] = bx; sB.y[i] = by; sB.z[i] = bz;
        bad |= !(isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(bx) && isfinite(by) && isfinite(bz));
    }
    if (__syncthreads_or(bad)) {                   // uniform over the workgroup
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        if (tid < 6) out[tid] = nan;
        if (counts && tid < 10) counts[bs * 10 + tid] = 0;
        return;
    }
    // every thread reads back only the points it staged itself (i = tid + 256 k) until the query stage
    double c6[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += 256) {
        c6[0] += (double)sA.x[i]; c6[1] += (double)sA.y[i]; c6[2] += (double)sA.z[i];
        c6[3] += (double)sB.x[i]; c6[4] += (double)sB.y[i]; c6[5] += (double)sB.z[i];
    }
    block_sums<6>(c6, reinterpret_cast<double(*)[6]>(&red[0][0]));
    double cA[3], cB[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { cA[c] = c6[c] / n; cB[c] = c6[3 + c] / n; }
    double h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                   // cross-covariance (9) and the variance of A
    for (int i = tid; i < n; i += 256) {
        const double a[3] = {(double)sA.x[i] - cA[0], (double)sA.y[i] - cA[1], (double)sA.z[i] - cA[2]};
        const double bb[3] = {(double)sB.x[i] - cB[0], (double)sB.y[i] - cB[1], (double)sB.z[i] - cB[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            h[9] += a[r] * a[r];
#pragma unroll
            for (int c = 0; c < 3; ++c) h[r * 3 + c] += a[r] * bb[c];
        }
    }
    block_sums<10>(h, reinterpret_cast<double(*)[10]>(&red[0][0]));
    double H[3][3], T[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k / 3][k % 3] = h[k] / n;
    vpho::similarity_from_cov(H, cA, cB, h[9] / n, T);             // every thread solves the same 3x3: identical bits, no broadcast
    // per-point errors and AUC counts in fp64; then the three centred fp32 sets for the queries
    double gs[2] = {0, 0};
    int cnt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += 256) {
        const double a[3] = {(double)sA.x[i], (double)sA.y[i], (double)sA.z[i]};
        const double bb[3] = {(double)sB.x[i], (double)sB.y[i], (double)sB.z[i]};
        double al[3], e0 = 0, e1 = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            al[r] = T[r * 3] * a[0] + T[r * 3 + 1] * a[1] + T[r * 3 + 2] * a[2] + T[9 + r];
            const double d0 = a[r] - bb[r], d1 = al[r] - bb[r];
            e0 += d0 * d0; e1 += d1 * d1;
        }
        const int k0 = pck_count(sqrt(e0), s_t, n_t), k1 = pck_count(sqrt(e1), s_t, n_t);
        gs[0] += s_g[k0]; gs[1] += s_g[k1];
        cnt[8] += k0; cnt[9] += k1;
        sA.x[i] = (float)(a[0] - cB[0]); sA.y[i] = (float)(a[1] - cB[1]); sA.z[i] = (float)(a[2] - cB[2]);
        sH.x[i] = (float)(al[0] - cB[0]); sH.y[i] = (float)(al[1] - cB[1]); sH.z[i] = (float)(al[2] - cB[2]);
        sB.x[i] = (float)(bb[0] - cB[0]); sB.y[i] = (float)(bb[1] - cB[1]); sB.z[i] = (float)(bb[2] - cB[2]);
    }
    __syncthreads();
    if (with_fscore) {
        const int m4 = (n + 3) & ~3;               // the last point repeated up to a multiple of 4: the target walk needs no tail
        if (tid < m4 - n) {
            const int i = n + tid;
            sA.x[i] = sA.x[n - 1]; sA.y[i] = sA.y[n - 1]; sA.z[i] = sA.z[n - 1];
            sH.x[i] = sH.x[n - 1]; sH.y[i] = sH.y[n - 1]; sH.z[i] = sH.z[n - 1];
            sB.x[i] = sB.x[n - 1]; sB.y[i] = sB.y[n - 1]; sB.z[i] = sB.z[n - 1];
        }
        __syncthreads();
        // task k: job = k / n in {0: B -> A (d1 raw), 1: A -> B (d2 raw), 2: B -> aligned (d1 PA), 3: aligned -> B (d2 PA)}, point k % n
        for (int k = tid; k < 4 * n; k += 256) {
            const int job = k / n, p = k - job * n;
            const Planes& X = job < 2 ? sA : sH;
            const Planes& Q = (job & 1) ? X : sB;
            const Planes& Tg = (job & 1) ? sB : X;
            const double d = sqrt((double)nearest_d2(Tg, m4, Q.x[p], Q.y[p], Q.z[p]));
            const int lo = d < th_lo, hi = d < th_hi;
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) { cnt[jb * 2] += jb == job ? lo : 0; cnt[jb * 2 + 1] += jb == job ? hi : 0; }   // constant indices: registers
        }
    }
    block_sums<2>(gs, reinterpret_cast<double(*)[2]>(&red[0][0]));
#pragma unroll
    for (int k = 0; k < 10; ++k) cnt[k] = wave_sum_i(cnt[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 10; ++k) redi[tid >> 6][k] = cnt[k];
    }
    __syncthreads();
    if (tid == 0) {
        int tot[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) tot[k] = redi[0][k] + redi[1][k] + redi[2][k] + redi[3][k];
        out[0] = gs[0] / n;
        out[1] = gs[1] / n;
#pragma unroll
        for (int set = 0; set < 2; ++set)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                double f = __longlong_as_double(0x7ff8000000000000LL);          // not computed without with_fscore
                if (with_fscore) {
                    const double prec = (double)tot[set * 4 + t] / n, rec = (double)tot[set * 4 + 2 + t] / n;
                    f = prec + rec > 0 ? 2.0 * prec * rec / (prec + rec) : 0.0;
                }
                out[2 + set * 2 + t] = f;
            }
        if (counts) {
            // {raw, PA} x {d1, d2} x {lo, hi}, then the two sums of the AUC counts
#pragma unroll
            for (int k = 0; k < 10; ++k) counts[bs * 10 + k] = tot[k];
        }
    }
}

// per image and value, in hypothesis order: hypothesis 0, best-of-S (the MAXIMUM: all eight values are scores) and mean-of-S (fp64 sum
// in ascending s); a NaN hypothesis makes best and mean NaN
__global__ void hand_bench_table_kernel(const double* __restrict__ per, int n_img, int S, double* __restrict__ one, double* __restrict__ best,
                                        double* __restrict__ mean) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img * 8) return;
    const int b = i / 8, c = i % 8;
    const double* p = per + (long long)b * S * 8 + c;
    double bv = p[0], sv = p[0];
    for (int s = 1; s < S; ++s) {
        const double v = p[(long long)s * 8];
        bv = (v > bv || v != v) ? v : bv;
        sv += v;
    }
    one[i] = p[0];
    best[i] = bv;
    mean[i] = sv / S;
}

}  // namespace

extern "C" int vpho_hand_bench_multi_f32(const float* pd, const float* gt, const float* root_joint, const unsigned char* is_right, int n_img,
                                         int n_hyp, int n_pts, double f_thresh_lo, double f_thresh_hi, const double* auc_thresh,
                                         const double* auc_g, int n_thresh, int with_fscore, double* values, int* counts, void* stream) {
    VPHO_REQUIRE(pd && gt && root_joint && is_right && auc_thresh && auc_g && values && n_img > 0 && n_hyp > 0,
                 "vpho_hand_bench_multi_f32: bad argument");
    VPHO_REQUIRE(n_pts >= 3 && n_pts <= HB_MAX_PTS, "vpho_hand_bench_multi_f32: %d points per hand, the kernel takes 3 .. %d", n_pts, HB_MAX_PTS);
    VPHO_REQUIRE((long long)n_img * n_hyp <= 0x7fffffffLL, "vpho_hand_bench_multi_f32: %d x %d pairs, at most 2^31 - 1 in one call", n_img, n_hyp);
    VPHO_REQUIRE(n_thresh >= 2 && n_thresh <= HB_MAX_THRESH, "vpho_hand_bench_multi_f32: %d AUC thresholds, the kernel takes 2 .. %d", n_thresh,
                 HB_MAX_THRESH);
    VPHO_REQUIRE(f_thresh_lo > 0 && f_thresh_hi > 0, "vpho_hand_bench_multi_f32: the F-score distances must be positive");
    hipLaunchKernelGGL(hand_bench_multi_kernel, dim3(n_img * n_hyp), dim3(256), 0, (hipStream_t)stream, pd, gt, root_joint, is_right, n_hyp,
                       n_pts, f_thresh_lo, f_thresh_hi, auc_thresh, auc_g, n_thresh, with_fscore, values, counts);
    return vpho::check_launch("hand_bench_multi_kernel");
}

extern "C" int vpho_hand_bench_table_f64(const double* per, int n_img, int n_hyp, double* one, double* best, double* mean, void* stream) {
    VPHO_REQUIRE(per && one && best && mean && n_img > 0 && n_hyp > 0 && (long long)n_img * 8 <= 0x7fffffffLL,
                 "vpho_hand_bench_table_f64: bad argument");
    hipLaunchKernelGGL(hand_bench_table_kernel, dim3((n_img * 8 + 255) / 256), dim3(256), 0, (hipStream_t)stream, per, n_img, n_hyp, one, best,
                       mean);
    return vpho::check_launch("hand_bench_table_kernel");
}
