// Device-side hand metrics: MJE / PA-MJE / MVE / PA-MVE of TesterHand.criterion_MJE_PAMJE
// (lib/engine/test.py:657-680) with the Procrustes alignment of transform_fn.rigid_transform_3D_AtoB (:43-58), so that the
// evaluation loop ships 8 floats per image to the all-gather instead of copying (bs,S,778,3) candidates to the host.
// One block per image; reductions and the 3x3 SVD (Jacobi on H^T H) in fp64.  HBM-bound: 24 B read per point.
#include <type_traits>
#include "common.h"
#include "rot.h"
#include "procrustes.h"
#include <algorithm>
#include "../../include/vpho_hip.h"

namespace {

using vpho::wave_sum;
using vpho::similarity_from_cov;

__device__ inline double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void hand_metrics_kernel(const float* __restrict__ pd, const float* __restrict__ gt, int n,
                                                           float* __restrict__ mean_err, float* __restrict__ pa_mean_err,
                                                           float* __restrict__ per_point) {
    __shared__ double red[256];
    __shared__ double T[12];            // c*R (9) and t (3)
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* A = pd + (long long)b * n * 3;
    const float* B = gt + (long long)b * n * 3;
    double sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0}, se = 0;
    for (int i = tid; i < n; i += 256) {
        double d2 = 0;
        for (int c = 0; c < 3; ++c) { sa[c] += A[i * 3 + c]; sb[c] += B[i * 3 + c]; const double d = (double)B[i * 3 + c] - A[i * 3 + c]; d2 += d * d; }
        const double e = sqrt(d2);
        se += e;
        if (per_point) per_point[(long long)b * n + i] = (float)e;
    }
    double cA[3], cB[3];
    for (int c = 0; c < 3; ++c) { cA[c] = block_sum(sa[c], red) / n; cB[c] = block_sum(sb[c], red) / n; }
    const double me = block_sum(se, red) / n;
    double h[9] = {0}, va = 0;
    for (int i = tid; i < n; i += 256) {
        double a[3], bb[3];
        for (int c = 0; c < 3; ++c) { a[c] = A[i * 3 + c] - cA[c]; bb[c] = B[i * 3 + c] - cB[c]; va += a[c] * a[c]; }
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) h[r * 3 + c] += a[r] * bb[c];
    }
    double H[3][3];
    for (int k = 0; k < 9; ++k) H[k / 3][k % 3] = block_sum(h[k], red) / n;
    const double varA = block_sum(va, red) / n;
    if (tid == 0) {   // the one solve of procrustes.h, as in the multi-hypothesis and the benchmark kernels
        double Tl[12];
        similarity_from_cov(H, cA, cB, varA, Tl);
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = Tl[k];
    }
    __syncthreads();
    double sp = 0;
    for (int i = tid; i < n; i += 256) {
        double d2 = 0;
        for (int r = 0; r < 3; ++r) {
            const double al = T[r * 3] * A[i * 3] + T[r * 3 + 1] * A[i * 3 + 1] + T[r * 3 + 2] * A[i * 3 + 2] + T[9 + r];
            const double d = (double)B[i * 3 + r] - al;
            d2 += d * d;
        }
        sp += sqrt(d2);
    }
    const double pa = block_sum(sp, red) / n;
    if (tid == 0) { mean_err[b] = (float)me; pa_mean_err[b] = (float)pa; }
}

// obj_9D_to_mat (lib/utils/transform_fn.py:85-90) + root joint (train_diff_hand_obj.py:594-597): [rot6d | t] -> [R | t + root]
__global__ void obj_9d_to_rt_kernel(const double* __restrict__ pose9, const float* __restrict__ root, int n, double* __restrict__ rt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    vpho::obj_9d_to_rt(pose9 + (long long)i * 9, root + (long long)i * 3, rt + (long long)i * 12);
}

// ------------------------------------------------------------------------------------------------ object metrics
// TesterObject (lib/engine/test.py:240-503) per image and single hypothesis: MCE / OCE on the 8 model-box corners (fp64,
// :354-374), MCE2 on the axis-aligned boxes of the transformed sampled vertices (:155-193,398-414), ADD / ADD-S / REP
// (:425-458), their 0.1-diameter and 5-pixel hits (:505-519), Chamfer-L2 and F-score at six thresholds on the full vertex
// set (:460-503).  Transforms are fp64 on the fp64 tables and rounded to fp32 where the reference calls .float(); the two
// nearest-neighbour searches are exact fp32 brute force through LDS tiles (the reference's torch.cdist uses the matmul
// expansion, which is only accurate to ~1e-7 in d^2 at camera-space magnitudes).  HBM/L2-bound: 24 B per table point.
struct ObjWs { float *pd_s, *gt_s, *pd_f, *gt_f, *d_s, *d_p2g, *d_g2p; long long bytes; };

__host__ __device__ inline long long ows_align(long long v) { return (v + 255) / 256 * 256; }

inline ObjWs obj_carve(int n_img, int ns, int vmax, char* base) {
    long long off = 0;
    ObjWs w;
    auto take = [&](long long b) { char* p = base ? base + off : nullptr; off += ows_align(b); return (float*)p; };
    w.pd_s = take((long long)n_img * ns * 12); w.gt_s = take((long long)n_img * ns * 12);
    w.pd_f = take((long long)n_img * vmax * 12); w.gt_f = take((long long)n_img * vmax * 12);
    w.d_s = take((long long)n_img * ns * 4); w.d_p2g = take((long long)n_img * vmax * 4); w.d_g2p = take((long long)n_img * vmax * 4);
    w.bytes = off;
    return w;
}

__device__ inline void rt_apply(const double* rt, const double* v, double* o) {
    for (int r = 0; r < 3; ++r) o[r] = v[0] * rt[r * 4 + 0] + v[1] * rt[r * 4 + 1] + v[2] * rt[r * 4 + 2] + rt[r * 4 + 3];
}

__global__ __launch_bounds__(256) void obj_transform_kernel(const vpho_obj_metric_tables t, const double* __restrict__ pd_rt,
                                                            const double* __restrict__ gt_rt, const int* __restrict__ obj_id,
                                                            int vmax, ObjWs w) {
    const int b = blockIdx.x, o = obj_id[b];
    const int nf = t.vert_offset[o + 1] - t.vert_offset[o];
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i >= t.n_sampled + nf) return;
    const bool full = i >= t.n_sampled;
    const int k = full ? i - t.n_sampled : i;
    const double* v = full ? t.verts + ((long long)t.vert_offset[o] + k) * 3 : t.verts_sampled + ((long long)o * t.n_sampled + k) * 3;
    double p[3], g[3];
    rt_apply(pd_rt + (long long)b * 12, v, p);
    rt_apply(gt_rt + (long long)b * 12, v, g);
    float* po = full ? w.pd_f + ((long long)b * vmax + k) * 3 : w.pd_s + ((long long)b * t.n_sampled + k) * 3;
    float* go = full ? w.gt_f + ((long long)b * vmax + k) * 3 : w.gt_s + ((long long)b * t.n_sampled + k) * 3;
    for (int c = 0; c < 3; ++c) { po[c] = (float)p[c]; go[c] = (float)g[c]; }
}

// grid (image, job, chunk of 256 source points): job 0 sampled pd->gt, 1 full pd->gt, 2 full gt->pd
__global__ __launch_bounds__(256) void obj_nn_kernel(const vpho_obj_metric_tables t, const int* __restrict__ obj_id, int vmax, ObjWs w) {
    __shared__ float tile[256 * 3];
    const int b = blockIdx.x, job = blockIdx.y, o = obj_id[b];
    const int n = job == 0 ? t.n_sampled : t.vert_offset[o + 1] - t.vert_offset[o];
    const int ld = job == 0 ? t.n_sampled : vmax;
    const float* src = (job == 0 ? w.pd_s : job == 1 ? w.pd_f : w.gt_f) + (long long)b * ld * 3;
    const float* dst = (job == 0 ? w.gt_s : job == 1 ? w.gt_f : w.pd_f) + (long long)b * ld * 3;
    float* out = (job == 0 ? w.d_s : job == 1 ? w.d_p2g : w.d_g2p) + (long long)b * ld;
    if (blockIdx.z * 256 >= n) return;
    const int i = blockIdx.z * 256 + threadIdx.x;
    const bool live = i < n;
    const float x = live ? src[i * 3] : 0.f, y = live ? src[i * 3 + 1] : 0.f, z = live ? src[i * 3 + 2] : 0.f;
    float best = INFINITY;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int m = min(256, n - j0);
        __syncthreads();
        for (int q = threadIdx.x; q < m * 3; q += 256) tile[q] = dst[(long long)j0 * 3 + q];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const float dx = x - tile[j * 3], dy = y - tile[j * 3 + 1], dz = z - tile[j * 3 + 2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            best = d2 < best ? d2 : best;
        }
    }
    if (live) out[i] = sqrtf(best);
}

__device__ inline float block_minmax(float v, bool is_max, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = is_max ? fmaxf(red[tid], red[tid + o]) : fminf(red[tid], red[tid + o]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void obj_metrics_kernel(const vpho_obj_metric_tables t, const double* __restrict__ pd_rt,
                                                          const double* __restrict__ gt_rt, const double* __restrict__ cam,
                                                          const int* __restrict__ obj_id, int vmax, ObjWs w, double* __restrict__ out) {
    __shared__ double red[256];
    __shared__ float redf[256];
    __shared__ double corner[2][8][3];
    const int b = blockIdx.x, tid = threadIdx.x, o = obj_id[b];
    const int ns = t.n_sampled, nf = t.vert_offset[o + 1] - t.vert_offset[o];
    const double* prt = pd_rt + (long long)b * 12;
    const double* grt = gt_rt + (long long)b * 12;
    const double* K = cam + (long long)b * 9;
    if (tid < 8) {
        rt_apply(prt, t.bbox3d + ((long long)o * 8 + tid) * 3, corner[0][tid]);
        rt_apply(grt, t.bbox3d + ((long long)o * 8 + tid) * 3, corner[1][tid]);
    }
    __syncthreads();
    double mce = 0, oce = 0;
    if (tid == 0) {
        double cp[3] = {0, 0, 0}, cg[3] = {0, 0, 0};
        for (int k = 0; k < 8; ++k) {
            double d2 = 0;
            for (int c = 0; c < 3; ++c) { const double d = corner[0][k][c] - corner[1][k][c]; d2 += d * d; cp[c] += corner[0][k][c]; cg[c] += corner[1][k][c]; }
            mce += sqrt(d2);
        }
        mce /= 8;
        double d2 = 0;
        for (int c = 0; c < 3; ++c) { const double d = cp[c] / 8 - cg[c] / 8; d2 += d * d; }
        oce = sqrt(d2);
    }
    // sampled vertices: ADD (fp32 points), REP (fp64 points re-derived from the table), ADD-S, boxes for MCE2
    const float* ps = w.pd_s + (long long)b * ns * 3;
    const float* gs = w.gt_s + (long long)b * ns * 3;
    double s_add = 0, s_rep = 0, s_adds = 0;
    float mn[2][3], mx[2][3];
    for (int c = 0; c < 3; ++c) { mn[0][c] = mn[1][c] = INFINITY; mx[0][c] = mx[1][c] = -INFINITY; }
    for (int i = tid; i < ns; i += 256) {
        const float dx = ps[i * 3] - gs[i * 3], dy = ps[i * 3 + 1] - gs[i * 3 + 1], dz = ps[i * 3 + 2] - gs[i * 3 + 2];
        s_add += (double)sqrtf((dx * dx + dy * dy) + dz * dz);
        s_adds += (double)w.d_s[(long long)b * ns + i];
        for (int c = 0; c < 3; ++c) {
            mn[0][c] = fminf(mn[0][c], ps[i * 3 + c]); mx[0][c] = fmaxf(mx[0][c], ps[i * 3 + c]);
            mn[1][c] = fminf(mn[1][c], gs[i * 3 + c]); mx[1][c] = fmaxf(mx[1][c], gs[i * 3 + c]);
        }
        double p[3], g[3], pp[2], gp[2];
        const double* v = t.verts_sampled + ((long long)o * ns + i) * 3;
        rt_apply(prt, v, p);
        rt_apply(grt, v, g);
        for (int r = 0; r < 2; ++r) {
            pp[r] = (p[0] * K[r * 3] + p[1] * K[r * 3 + 1] + p[2] * K[r * 3 + 2]) / (p[2] + 1e-7);
            gp[r] = (g[0] * K[r * 3] + g[1] * K[r * 3 + 1] + g[2] * K[r * 3 + 2]) / (g[2] + 1e-7);
        }
        s_rep += sqrt((pp[0] - gp[0]) * (pp[0] - gp[0]) + (pp[1] - gp[1]) * (pp[1] - gp[1]));
    }
    const double add = block_sum(s_add, red) / ns, rep = block_sum(s_rep, red) / ns, adds = block_sum(s_adds, red) / ns;
    float bmn[2][3], bmx[2][3];
    for (int k = 0; k < 2; ++k)
        for (int c = 0; c < 3; ++c) { bmn[k][c] = block_minmax(mn[k][c], false, redf); bmx[k][c] = block_minmax(mx[k][c], true, redf); }
    // full vertices: Chamfer distance and F-scores
    const float th[6] = {0.002f, 0.005f, 0.010f, 0.020f, 0.050f, 0.100f};
    double s_p = 0, s_g = 0, cp[6] = {0, 0, 0, 0, 0, 0}, cg[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < nf; i += 256) {
        const float dp = w.d_p2g[(long long)b * vmax + i], dg = w.d_g2p[(long long)b * vmax + i];
        s_p += (double)dp; s_g += (double)dg;
        for (int k = 0; k < 6; ++k) { cp[k] += dp < th[k] ? 1.0 : 0.0; cg[k] += dg < th[k] ? 1.0 : 0.0; }
    }
    const double mp = block_sum(s_p, red) / nf, mg = block_sum(s_g, red) / nf;
    double fs[6];
    for (int k = 0; k < 6; ++k) {
        const float prec = (float)(block_sum(cp[k], red) / nf), rec = (float)(block_sum(cg[k], red) / nf);
        fs[k] = (double)((2.f * prec * rec) / ((prec + rec) + 1e-6f));
    }
    if (tid == 0) {
        // corners of the two axis-aligned boxes in the reference's order (test.py:163-187)
        const int sel[3][8] = {{0, 1, 0, 0, 1, 0, 1, 1}, {0, 0, 1, 0, 1, 1, 0, 1}, {0, 0, 0, 1, 0, 1, 1, 1}};
        float s2 = 0.f;
        for (int k = 0; k < 8; ++k) {
            float d2 = 0.f;
            for (int c = 0; c < 3; ++c) {
                const float a = sel[c][k] ? bmx[0][c] : bmn[0][c], g = sel[c][k] ? bmx[1][c] : bmn[1][c];
                d2 += (a - g) * (a - g);
            }
            s2 += sqrtf(d2);
        }
        const double diam = t.diameter[o];
        double* r = out + (long long)b * 16;
        r[0] = mce; r[1] = oce; r[2] = (double)(s2 / 8.f); r[3] = add; r[4] = adds;
        r[5] = add <= diam * 0.1 ? 1.0 : 0.0; r[6] = adds <= diam * 0.1 ? 1.0 : 0.0; r[7] = rep; r[8] = rep < 5 ? 1.0 : 0.0;
        r[9] = 0.5 * (mp + mg);
        for (int k = 0; k < 6; ++k) r[10 + k] = fs[k];
    }
}

// ------------------------------------------------------------------------------------------------ multi-hypothesis evaluation
// Every sampled hypothesis scored (test_diff_hand / test_diff_object with is_eval_best, train_diff_hand_obj.py:454-523): the
// per-hypothesis TesterHand / TesterObject values and the per-image best-of-S (TesterObject.postprocess, test.py:522-567) and
// mean-of-S.  The ground truth is broadcast over the S candidates instead of being repeated S times in memory.

// One wave per (image, candidate): MJE and PA-MJE (TesterHand.criterion_MJE_PAMJE, test.py:657-679) of candidate s against the
// image's ground truth.  The reference's postprocess (train_diff_hand_obj.py:578-602: x un-flipped for left hands, root joint
// added, both in fp32) is applied as each point is loaded.  Reductions in fp64 by wave butterflies; no LDS, no barrier.
__global__ __launch_bounds__(64) void hand_metrics_multi_kernel(const float* __restrict__ pd, const float* __restrict__ gt,
                                                                const float* __restrict__ root, const unsigned char* __restrict__ is_right,
                                                                int S, int n, float* __restrict__ mean_err, float* __restrict__ pa_mean_err) {
    const long long bs = blockIdx.x;
    const int b = (int)(bs / S), l = threadIdx.x;
    const float* A = pd + bs * n * 3;
    const float* B = gt + (long long)b * n * 3;
    const float sg = is_right[b] ? 1.f : -1.f, r0 = root[b * 3], r1 = root[b * 3 + 1], r2 = root[b * 3 + 2];
    auto load = [&](int i, double a[3]) {
        a[0] = (double)(A[i * 3] * sg + r0); a[1] = (double)(A[i * 3 + 1] + r1); a[2] = (double)(A[i * 3 + 2] + r2);
    };
    double sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0}, se = 0;
    for (int i = l; i < n; i += 64) {
        double a[3], d2 = 0;
        load(i, a);
#pragma unroll
        for (int c = 0; c < 3; ++c) { sa[c] += a[c]; sb[c] += B[i * 3 + c]; const double d = (double)B[i * 3 + c] - a[c]; d2 += d * d; }
        se += sqrt(d2);
    }
    double cA[3], cB[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { cA[c] = wave_sum(sa[c]) / n; cB[c] = wave_sum(sb[c]) / n; }
    const double me = wave_sum(se) / n;
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, va = 0;
    for (int i = l; i < n; i += 64) {
        double a[3], bb[3];
        load(i, a);
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] -= cA[c]; bb[c] = B[i * 3 + c] - cB[c]; va += a[c] * a[c]; }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) h[r * 3 + c] += a[r] * bb[c];
    }
    double H[3][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k / 3][k % 3] = wave_sum(h[k]) / n;
    const double varA = wave_sum(va) / n;
    double T[12];
    similarity_from_cov(H, cA, cB, varA, T);           // every lane solves the same 3x3: identical results, no broadcast needed
    double sp = 0;
    for (int i = l; i < n; i += 64) {
        double a[3], d2 = 0;
        load(i, a);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double al = T[r * 3] * a[0] + T[r * 3 + 1] * a[1] + T[r * 3 + 2] * a[2] + T[9 + r];
            const double d = (double)B[i * 3 + r] - al;
            d2 += d * d;
        }
        sp += sqrt(d2);
    }
    const double pa = wave_sum(sp) / n;
    if (l == 0) { mean_err[bs] = (float)me; pa_mean_err[bs] = (float)pa; }
}

// Object: every nearest-neighbour search of TesterObject is done in an object frame, where the target set is the model point set
// itself and does not depend on the candidate.  For a model point x the pd->gt distance is the distance of R_g^-1 (R_s x + t_s - t_g)
// to the nearest point of M, the gt->pd one that of R_s^-1 (R_g y + t_g - t_s).  A workgroup stages M in LDS tiles (fp32, as the
// reference's .float() points) and streams MH_CHUNK queries of one candidate past them, MH_QPL per lane in packed-f32 pairs: 3 packed
// VALU operations and half a v_min3 per point pair in the direct form |q - y|^2 (a candidate equal to the ground truth gives 0, not a
// rounding residue of an expansion).  Distances never go to HBM; each workgroup leaves one row of partial sums.
constexpr int MH_QPL = 8;                          // queries per lane
constexpr int MH_CHUNK = 256 * MH_QPL;             // queries per workgroup
constexpr int MH_TILE = 2048;                      // targets per LDS tile: 32 KB of float4

struct MhWs { double* part; int chunks; long long bytes; };   // part [n_img*S][3 jobs][chunks][8]: sum of distances, 6 threshold counts

inline MhWs mh_carve(int n_img, int S, int ns, int vmax, char* base) {
    MhWs w;
    w.chunks = (std::max(ns, vmax) + MH_CHUNK - 1) / MH_CHUNK;
    w.part = (double*)base;
    w.bytes = ows_align((long long)n_img * S * 3 * w.chunks * 8 * sizeof(double));
    return w;
}

// x -> Rd^-1 (Rs x + ts - td) as one 3x4 map, fp64; the exact inverse (adjugate / det), so that Rs = Rd gives the identity
// to fp64 rounding even for a ground truth stored in fp32
__device__ inline void rel_transform(const double* src, const double* dst, double T[12]) {
    const double a = dst[0], b = dst[1], c = dst[2], d = dst[4], e = dst[5], f = dst[6], g = dst[8], h = dst[9], k = dst[10];
    const double det = a * (e * k - f * h) - b * (d * k - f * g) + c * (d * h - e * g);
    const double inv[9] = {(e * k - f * h) / det, (c * h - b * k) / det, (b * f - c * e) / det,
                           (f * g - d * k) / det, (a * k - c * g) / det, (c * d - a * f) / det,
                           (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int col = 0; col < 3; ++col)
            T[r * 4 + col] = inv[r * 3] * src[col] + inv[r * 3 + 1] * src[4 + col] + inv[r * 3 + 2] * src[8 + col];
        T[r * 4 + 3] = inv[r * 3] * (src[3] - dst[3]) + inv[r * 3 + 1] * (src[7] - dst[7]) + inv[r * 3 + 2] * (src[11] - dst[11]);
    }
}

// grid (image*S + candidate, job, chunk of MH_CHUNK queries): job 0 sampled pd->gt (ADD-S), 1 full pd->gt, 2 full gt->pd
__global__ __launch_bounds__(256) void obj_multi_nn_kernel(const vpho_obj_metric_tables t, const double* __restrict__ pd_rt,
                                                           const double* __restrict__ gt_rt, const int* __restrict__ obj_id, int S, MhWs w) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    __shared__ float4 tile[MH_TILE + 1];
    __shared__ double red[4][8];
    const int bs = blockIdx.x, job = blockIdx.y, chunk = blockIdx.z, tid = threadIdx.x, wave = tid >> 6;
    const int b = bs / S, o = obj_id[b];
    const int n = job == 0 ? t.n_sampled : t.vert_offset[o + 1] - t.vert_offset[o];
    const double* pts = job == 0 ? t.verts_sampled + (long long)o * t.n_sampled * 3 : t.verts + (long long)t.vert_offset[o] * 3;
    double* part = w.part + (((long long)bs * 3 + job) * w.chunks + chunk) * 8;
    const int q0 = chunk * MH_CHUNK;
    if (q0 >= n) {                                 // whole workgroup: this object has fewer points than the largest one
        if (tid < 8) part[tid] = 0.0;
        return;
    }
    double T[12];
    const double* prt = pd_rt + (long long)bs * 12;
    const double* grt = gt_rt + (long long)b * 12;
    if (job == 2) rel_transform(grt, prt, T); else rel_transform(prt, grt, T);
    const int qi = q0 + tid * MH_QPL;               // this lane's first query; its MH_QPL queries are consecutive points
    f32x2 qx[MH_QPL / 2], qy[MH_QPL / 2], qz[MH_QPL / 2];
#pragma unroll
    for (int k = 0; k < MH_QPL; ++k) {
        const int i = qi + k;
        float v[3] = {0.f, 0.f, 0.f};
        if (i < n) {
            const double* x = pts + (long long)i * 3;
#pragma unroll
            for (int r = 0; r < 3; ++r) v[r] = (float)(T[r * 4] * x[0] + T[r * 4 + 1] * x[1] + T[r * 4 + 2] * x[2] + T[r * 4 + 3]);
        }
        qx[k / 2][k % 2] = v[0]; qy[k / 2][k % 2] = v[1]; qz[k / 2][k % 2] = v[2];
    }
    float best[MH_QPL];
#pragma unroll
    for (int k = 0; k < MH_QPL; ++k) best[k] = INFINITY;
    const bool wave_live = q0 + wave * 64 * MH_QPL < n;      // wave-uniform: a wave with no live query only helps to stage
    for (int j0 = 0; j0 < n; j0 += MH_TILE) {
        const int m = min(MH_TILE, n - j0);
        __syncthreads();
        for (int j = tid; j < m; j += 256) {
            const double* y = pts + (long long)(j0 + j) * 3;
            tile[j] = make_float4((float)y[0], (float)y[1], (float)y[2], 0.f);
        }
        if (tid == 0 && (m & 1)) {                 // odd tile: the last point twice, so that the pair loop needs no tail
            const double* y = pts + (long long)(j0 + m - 1) * 3;
            tile[m] = make_float4((float)y[0], (float)y[1], (float)y[2], 0.f);
        }
        __syncthreads();
        if (wave_live) {
#pragma clang fp contract(fast)
            for (int j = 0; j < m; j += 2) {
                const float4 y0 = tile[j], y1 = tile[j + 1];
#pragma unroll
                for (int k = 0; k < MH_QPL / 2; ++k) {
                    const f32x2 ax = qx[k] - y0.x, ay = qy[k] - y0.y, az = qz[k] - y0.z;
                    const f32x2 bx = qx[k] - y1.x, by = qy[k] - y1.y, bz = qz[k] - y1.z;
                    const f32x2 da = az * az + (ay * ay + ax * ax), db = bz * bz + (by * by + bx * bx);
                    best[2 * k] = fminf(best[2 * k], fminf(da.x, db.x));
                    best[2 * k + 1] = fminf(best[2 * k + 1], fminf(da.y, db.y));
                }
            }
        }
    }
    const float th[6] = {0.002f, 0.005f, 0.010f, 0.020f, 0.050f, 0.100f};
    double sum = 0, cnt[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < MH_QPL; ++k) {
        if (qi + k < n) {
            const float d = sqrtf(best[k]);
            sum += (double)d;
#pragma unroll
            for (int c = 0; c < 6; ++c) cnt[c] += d < th[c] ? 1.0 : 0.0;
        }
    }
    sum = wave_sum(sum);
#pragma unroll
    for (int c = 0; c < 6; ++c) cnt[c] = wave_sum(cnt[c]);
    if ((tid & 63) == 0) {
        red[wave][0] = sum;
#pragma unroll
        for (int c = 0; c < 6; ++c) red[wave][1 + c] = cnt[c];
    }
    __syncthreads();
    if (tid < 7) part[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    else if (tid == 7) part[7] = 0.0;
}

// one workgroup per (image, candidate): the 16 TesterObject values from the corners, the sampled vertices and the NN partial sums
__global__ __launch_bounds__(256) void obj_multi_metrics_kernel(const vpho_obj_metric_tables t, const double* __restrict__ pd_rt,
                                                                const double* __restrict__ gt_rt, const double* __restrict__ cam,
                                                                const int* __restrict__ obj_id, int S, MhWs w, double* __restrict__ out) {
    __shared__ double red[256];
    __shared__ float redf[256];
    __shared__ double corner[2][8][3];
    const int bs = blockIdx.x, b = bs / S, tid = threadIdx.x, o = obj_id[b];
    const int ns = t.n_sampled, nf = t.vert_offset[o + 1] - t.vert_offset[o];
    const double* prt = pd_rt + (long long)bs * 12;
    const double* grt = gt_rt + (long long)b * 12;
    const double* K = cam + (long long)b * 9;
    if (tid < 8) {
        rt_apply(prt, t.bbox3d + ((long long)o * 8 + tid) * 3, corner[0][tid]);
        rt_apply(grt, t.bbox3d + ((long long)o * 8 + tid) * 3, corner[1][tid]);
    }
    __syncthreads();
    double mce = 0, oce = 0;
    if (tid == 0) {
        double cp[3] = {0, 0, 0}, cg[3] = {0, 0, 0};
        for (int k = 0; k < 8; ++k) {
            double d2 = 0;
            for (int c = 0; c < 3; ++c) { const double d = corner[0][k][c] - corner[1][k][c]; d2 += d * d; cp[c] += corner[0][k][c]; cg[c] += corner[1][k][c]; }
            mce += sqrt(d2);
        }
        mce /= 8;
        double d2 = 0;
        for (int c = 0; c < 3; ++c) { const double d = cp[c] / 8 - cg[c] / 8; d2 += d * d; }
        oce = sqrt(d2);
    }
    // sampled vertices, transformed here (fp64, rounded to fp32 where the reference calls .float()): ADD, REP, boxes for MCE2
    double s_add = 0, s_rep = 0;
    float mn[2][3], mx[2][3];
    for (int c = 0; c < 3; ++c) { mn[0][c] = mn[1][c] = INFINITY; mx[0][c] = mx[1][c] = -INFINITY; }
    for (int i = tid; i < ns; i += 256) {
        double p[3], g[3], pp[2], gp[2];
        const double* v = t.verts_sampled + ((long long)o * ns + i) * 3;
        rt_apply(prt, v, p);
        rt_apply(grt, v, g);
        float pf[3], gf[3];
        for (int c = 0; c < 3; ++c) { pf[c] = (float)p[c]; gf[c] = (float)g[c]; }
        const float dx = pf[0] - gf[0], dy = pf[1] - gf[1], dz = pf[2] - gf[2];
        s_add += (double)sqrtf((dx * dx + dy * dy) + dz * dz);
        for (int c = 0; c < 3; ++c) {
            mn[0][c] = fminf(mn[0][c], pf[c]); mx[0][c] = fmaxf(mx[0][c], pf[c]);
            mn[1][c] = fminf(mn[1][c], gf[c]); mx[1][c] = fmaxf(mx[1][c], gf[c]);
        }
        for (int r = 0; r < 2; ++r) {
            pp[r] = (p[0] * K[r * 3] + p[1] * K[r * 3 + 1] + p[2] * K[r * 3 + 2]) / (p[2] + 1e-7);
            gp[r] = (g[0] * K[r * 3] + g[1] * K[r * 3 + 1] + g[2] * K[r * 3 + 2]) / (g[2] + 1e-7);
        }
        s_rep += sqrt((pp[0] - gp[0]) * (pp[0] - gp[0]) + (pp[1] - gp[1]) * (pp[1] - gp[1]));
    }
    const double add = block_sum(s_add, red) / ns, rep = block_sum(s_rep, red) / ns;
    float bmn[2][3], bmx[2][3];
    for (int k = 0; k < 2; ++k)
        for (int c = 0; c < 3; ++c) { bmn[k][c] = block_minmax(mn[k][c], false, redf); bmx[k][c] = block_minmax(mx[k][c], true, redf); }
    if (tid == 0) {
        // partial sums of the NN workgroups, in chunk order
        double acc[3][7];
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 7; ++c) {
                double a = 0;
                for (int q = 0; q < w.chunks; ++q) a += w.part[(((long long)bs * 3 + j) * w.chunks + q) * 8 + c];
                acc[j][c] = a;
            }
        const double adds = acc[0][0] / ns, mp = acc[1][0] / nf, mg = acc[2][0] / nf;
        const int sel[3][8] = {{0, 1, 0, 0, 1, 0, 1, 1}, {0, 0, 1, 0, 1, 1, 0, 1}, {0, 0, 0, 1, 0, 1, 1, 1}};
        float s2 = 0.f;
        for (int k = 0; k < 8; ++k) {
            float d2 = 0.f;
            for (int c = 0; c < 3; ++c) {
                const float a = sel[c][k] ? bmx[0][c] : bmn[0][c], g = sel[c][k] ? bmx[1][c] : bmn[1][c];
                d2 += (a - g) * (a - g);
            }
            s2 += sqrtf(d2);
        }
        const double diam = t.diameter[o];
        double* r = out + (long long)bs * 16;
        r[0] = mce; r[1] = oce; r[2] = (double)(s2 / 8.f); r[3] = add; r[4] = adds;
        r[5] = add <= diam * 0.1 ? 1.0 : 0.0; r[6] = adds <= diam * 0.1 ? 1.0 : 0.0; r[7] = rep; r[8] = rep < 5 ? 1.0 : 0.0;
        r[9] = 0.5 * (mp + mg);
        for (int k = 0; k < 6; ++k) {
            const float prec = (float)(acc[1][1 + k] / nf), rec = (float)(acc[2][1 + k] / nf);
            r[10 + k] = (double)((2.f * prec * rec) / ((prec + rec) + 1e-6f));
        }
    }
}

// per image and column, in candidate order: best-of-S (TesterObject.postprocess, test.py:529-538: max for the hit rates and
// F-scores, min for the rest) and mean-of-S
__global__ void obj_multi_reduce_kernel(const double* __restrict__ per, int n_img, int S, double* __restrict__ best, double* __restrict__ mean) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img * 16) return;
    const int b = i / 16, c = i % 16;
    const bool is_max = c == 5 || c == 6 || c == 8 || c >= 10;
    const double* p = per + (long long)b * S * 16 + c;
    double bv = p[0], sv = p[0];
    for (int s = 1; s < S; ++s) {
        const double v = p[(long long)s * 16];
        bv = is_max ? (v > bv ? v : bv) : (v < bv ? v : bv);
        sv += v;
    }
    if (best) best[i] = bv;
    if (mean) mean[i] = sv / S;
}

}  // namespace

extern "C" int vpho_hand_metrics_f32(const float* pd, const float* gt, int n_img, int n_pts, float* mean_err, float* pa_mean_err,
                                     float* per_point, void* stream) {
    VPHO_REQUIRE(pd && gt && mean_err && pa_mean_err && n_img > 0 && n_pts >= 3, "vpho_hand_metrics_f32: bad argument");
    hipLaunchKernelGGL(hand_metrics_kernel, dim3(n_img), dim3(256), 0, (hipStream_t)stream, pd, gt, n_pts, mean_err, pa_mean_err, per_point);
    return vpho::check_launch("hand_metrics_kernel");
}

extern "C" long long vpho_obj_metrics_workspace_bytes(const vpho_obj_metric_tables* t, int n_img, int max_verts) {
    if (!t || n_img <= 0 || max_verts <= 0 || t->n_sampled <= 0) return -1;
    return obj_carve(n_img, t->n_sampled, max_verts, nullptr).bytes;
}

extern "C" int vpho_obj_metrics_f64(const vpho_obj_metric_tables* t, const double* pd_rt, const double* gt_rt, const double* cam_intr,
                                    const int* obj_id, int n_img, int max_verts, double* out, void* workspace, long long workspace_bytes,
                                    void* stream) {
    VPHO_REQUIRE(t && t->bbox3d && t->verts_sampled && t->verts && t->vert_offset && t->diameter && t->n_obj > 0 && t->n_sampled > 0,
                 "vpho_obj_metrics_f64: bad tables");
    VPHO_REQUIRE(pd_rt && gt_rt && cam_intr && obj_id && out && workspace && n_img > 0 && max_verts > 0, "vpho_obj_metrics_f64: bad argument");
    const ObjWs w = obj_carve(n_img, t->n_sampled, max_verts, (char*)workspace);
    VPHO_REQUIRE(workspace_bytes >= w.bytes, "vpho_obj_metrics_f64: workspace %lld < %lld bytes", workspace_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    const int pts = t->n_sampled + max_verts;
    hipLaunchKernelGGL(obj_transform_kernel, dim3(n_img, (pts + 255) / 256), dim3(256), 0, s, *t, pd_rt, gt_rt, obj_id, max_verts, w);
    const int chunks = (std::max(t->n_sampled, max_verts) + 255) / 256;
    hipLaunchKernelGGL(obj_nn_kernel, dim3(n_img, 3, chunks), dim3(256), 0, s, *t, obj_id, max_verts, w);
    hipLaunchKernelGGL(obj_metrics_kernel, dim3(n_img), dim3(256), 0, s, *t, pd_rt, gt_rt, cam_intr, obj_id, max_verts, w, out);
    return vpho::check_launch("obj_metrics kernels");
}

extern "C" int vpho_obj_9d_to_rt_f64(const double* pose9, const float* root_joint, int n, double* rt, void* stream) {
    VPHO_REQUIRE(pose9 && root_joint && rt && n > 0, "vpho_obj_9d_to_rt_f64: bad argument");
    hipLaunchKernelGGL(obj_9d_to_rt_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, pose9, root_joint, n, rt);
    return vpho::check_launch("obj_9d_to_rt_kernel");
}

extern "C" int vpho_hand_metrics_multi_f32(const float* pd, const float* gt, const float* root_joint, const unsigned char* is_right, int n_img,
                                           int n_hyp, int n_pts, float* mean_err, float* pa_mean_err, void* stream) {
    VPHO_REQUIRE(pd && gt && root_joint && is_right && mean_err && pa_mean_err && n_img > 0 && n_hyp > 0 && n_pts >= 3 &&
                 (long long)n_img * n_hyp <= 0x7fffffff, "vpho_hand_metrics_multi_f32: bad argument");
    hipLaunchKernelGGL(hand_metrics_multi_kernel, dim3(n_img * n_hyp), dim3(64), 0, (hipStream_t)stream, pd, gt, root_joint, is_right, n_hyp,
                       n_pts, mean_err, pa_mean_err);
    return vpho::check_launch("hand_metrics_multi_kernel");
}

extern "C" long long vpho_obj_metrics_multi_workspace_bytes(const vpho_obj_metric_tables* t, int n_img, int n_hyp, int max_verts) {
    if (!t || n_img <= 0 || n_hyp <= 0 || max_verts <= 0 || t->n_sampled <= 0 || (long long)n_img * n_hyp > 0x7fffffff) return -1;
    return mh_carve(n_img, n_hyp, t->n_sampled, max_verts, nullptr).bytes;
}

extern "C" int vpho_obj_metrics_multi_f64(const vpho_obj_metric_tables* t, const double* pd_rt, const double* gt_rt, const double* cam_intr,
                                          const int* obj_id, int n_img, int n_hyp, int max_verts, double* out, double* best, double* mean,
                                          void* workspace, long long workspace_bytes, void* stream) {
    VPHO_REQUIRE(t && t->bbox3d && t->verts_sampled && t->verts && t->vert_offset && t->diameter && t->n_obj > 0 && t->n_sampled > 0,
                 "vpho_obj_metrics_multi_f64: bad tables");
    VPHO_REQUIRE(pd_rt && gt_rt && cam_intr && obj_id && out && workspace && n_img > 0 && n_hyp > 0 && max_verts > 0 &&
                 (long long)n_img * n_hyp <= 0x7fffffff, "vpho_obj_metrics_multi_f64: bad argument");
    const MhWs w = mh_carve(n_img, n_hyp, t->n_sampled, max_verts, (char*)workspace);
    VPHO_REQUIRE(workspace_bytes >= w.bytes, "vpho_obj_metrics_multi_f64: workspace %lld < %lld bytes", workspace_bytes, w.bytes);
    VPHO_REQUIRE(w.chunks <= 65535, "vpho_obj_metrics_multi_f64: %d query chunks exceed the grid", w.chunks);
    hipStream_t s = (hipStream_t)stream;
    const int rows = n_img * n_hyp;
    hipLaunchKernelGGL(obj_multi_nn_kernel, dim3(rows, 3, w.chunks), dim3(256), 0, s, *t, pd_rt, gt_rt, obj_id, n_hyp, w);
    hipLaunchKernelGGL(obj_multi_metrics_kernel, dim3(rows), dim3(256), 0, s, *t, pd_rt, gt_rt, cam_intr, obj_id, n_hyp, w, out);
    if (best || mean)
        hipLaunchKernelGGL(obj_multi_reduce_kernel, dim3((n_img * 16 + 255) / 256), dim3(256), 0, s, out, n_img, n_hyp, best, mean);
    return vpho::check_launch("obj_metrics_multi kernels");
}
