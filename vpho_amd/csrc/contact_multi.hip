// Hand contact map of EVERY sampled hypothesis (--eval_best with --eval_grasp): the hand -> object half of
// detect_hand_and_object_contact (lib/utils/physics_fn.py:47-117) for the n x S (hand hypothesis s, object hypothesis s) pairs, in the
// object's MODEL frame, so no posed object vertex is ever written (contact.hip wants them all in memory: n S N 12 bytes), and without
// its scan of every object vertex by every hand vertex.  Then the agreement of such maps with the annotation's (contact_agreement_kernel).
//
// Definition (all fp64, -ffp-contract=off, sums left to right; tests/_contact_multi_fp64.py restates it operation for operation):
//   c = (sg h_x + root_x, h_y + root_y, h_z + root_z),  sg = +1 right / -1 left     the filled hand vertex h back in the camera frame
//   p = R^T (c - t),   m = R^T (sg n_x, n_y, n_z)                                   point and normal in the model frame
//   v* = argmin_v d2(v),  d2(v) = dx dx + dy dy + dz dz,  (dx, dy, dz) = p - v      smaller ORIGINAL vertex index on an exact tie
//   e = p - v*,  nd = e . m,  vd = |e - nd m|
//   contact = nd > lo && nd < hi && vd < vt;   weight = contact ? clamp(contact_weight(nd) / w0, 0, 1) : 0   (contact_common.h)
//
// Pruning (vpho_obj_vertex_accel, built on the host by vpho_amd/grasp_eval.py vertex_accel): the vertices of every object in Morton order
// with their original indices, in clusters (of 32) with a bounding sphere.  A hand vertex takes the cluster with the nearest centre
// first, then all clusters in order, skipping those whose sphere is out of reach; every vertex of every other cluster goes through d2
// above -- the same expression on bit copies of the same operands as a scan of all vertices -- and the walk keeps the lexicographic
// minimum of (d2, original index), which does not depend on the order of the visits.  So the walk returns the brute-force index as long
// as no skipped vertex could have been that minimum:
//     skip iff  D > reach + r,   D = |p - centre|,  reach = sqrt(best) (1 + 2^-20),  r = r0 (1 + 2^-30) + 2^-30 diag   (all fp64)
//   with r0 the largest distance of the cluster's vertices from the centre and diag the object's bounding-box diagonal (the inflations
//   of penetration_multi.hip).  best only falls, so a skip against an earlier best holds against the final one.  In exact arithmetic a
//   vertex v of the cluster has d_v >= D - r0.  Rounding: (i) D^2, (reach + r)^2 and r0 are each a handful of fp64 operations on
//   non-negative terms, relative error < 8 eps = 2^-50: covered 2^20-fold by the two inflations, so a skip means
//   d_v - d* > 2^-21 d* + 2^-31 diag for the vertex v* that set best; (ii) d2 squares three differences of exact operands and adds
//   non-negative terms: computed(v) = d_v^2 (1 + th), |th| < 4 eps.  For d* > 0: computed(v) > d*^2 (1 + 2^-21)^2 (1 - 4 eps) >
//   d*^2 (1 + 4 eps) >= best.  For d* = 0: best = 0 and d_v > 2^-31 diag > 0, so computed(v) > 0 (diag = 0 means all vertices equal:
//   r = 0, D^2 is d2 of those very vertices, sqrt(best)^2 (1 + 2^-20)^2 >= best, nothing is skipped).  The test is STRICT and a vertex
//   as near as v* has D <= d* + r0 < reach + r: its cluster is visited and the smaller index still wins.  A NaN fails the skip test.
//   The seed only tightens best early.
// A pair with a non-finite pose, root, hand vertex or normal, an obj_id outside the table or an object without vertices writes NaN
// weights (and nd, vd) and -1 indices for the whole pair; decided before anything is looked up, so nothing is read out of bounds.
// One workgroup per (image, hypothesis): the pose and the cluster spheres are wave-uniform (scalar loads), a wave holds 64 consecutive
// hand vertices, the rows of a cluster are scalar loads too (wave-uniform addresses, batched four rows at a time).  A wave visits every
// cluster that ANY of its 64 vertices cannot reject, so its time falls with the distance between them.  Vector stores only, plain C++.
// gfx950, -O3: contact_multi_kernel 53 VGPRs, no scratch, no vector-register spills, 256 B LDS (the vote of the finiteness check); 35 scalar
// registers -- loop-invariant pointers and gates -- are parked in the lanes of one VGPR and read back once per round of 64 vertices, outside
// the sphere and row loops: the pose alone fills 24 scalar registers.  contact_agreement_kernel
// 22 VGPRs, 6 KB LDS (its reduction arrays), no scratch; contact_agreement_table_kernel 18 VGPRs, no scratch, no LDS.
#include "common.h"
#include "../../include/vpho_hip.h"
#include "contact_common.h"

namespace {

constexpr int CM_THREADS = 256;
constexpr int CM_VALUES = 8;             // IoU, precision, recall, F1, MAE, anchor_agree, grasped, grasp_agree
constexpr int CM_MAE = 4;                // the one column whose best is the minimum

struct ContactMultiArgs {
    vpho_obj_vertex_accel acc;
    const float *hv, *hn;        // (n, S, Nh, 3)
    const double* root;          // (n, 3)
    const unsigned char* right;  // (n,)
    const double* rt;            // (n, S, 3, 4)
    const int* obj_id;           // (n,)
    int S, Nh;
    double lo, hi, vt, mid1, mid2, w0;
    float* weight;               // (n, S, Nh)
    int* nn;                     // (n, S, Nh) or NULL
    double *nd, *vd;             // (n, S, Nh) or NULL
};

__device__ inline double dot3(double ax, double ay, double az, double bx, double by, double bz) { return ax * bx + ay * by + az * bz; }

// Tables and poses are read through pointers into the CONSTANT address space: nothing writes them while the kernel runs, and that is what
// lets the compiler turn a read at a wave-uniform address (pose, spheres, cluster rows) into a scalar load and batch such loads -- through
// a plain pointer it has to assume that the stores to the outputs change them and reads them per lane, one wait per row
template <class T> using ro = const T __attribute__((address_space(4)))*;
template <class T> __device__ __forceinline__ ro<T> read_only(const T* p) { return (ro<T>)p; }

// the walk of one pair's hand vertices
__device__ __forceinline__ void contact_multi_pair(ro<double> vert, ro<int> index, ro<int> clu_start, ro<double> sphere, const float* __restrict__ V,
                                                   const float* __restrict__ N, ro<double> R, ro<double> root, float* __restrict__ weight,
                                                   int* __restrict__ nn, double* __restrict__ ndo, double* __restrict__ vdo, int kb, int ke, int Nh,
                                                   double sg, double lo, double hi, double vt, double mid1, double mid2, double w0);

__global__ __launch_bounds__(CM_THREADS) void contact_multi_kernel(const ContactMultiArgs a) {
    const long long hyp = blockIdx.x;                  // image * S + hypothesis
    const int img = (int)(hyp / a.S), tid = threadIdx.x;
    const int o = a.obj_id[img];
    const double* R = a.rt + hyp * 12;
    const double* root = a.root + (long long)img * 3;
    const float* V = a.hv + hyp * a.Nh * 3;
    const float* N = a.hn + hyp * a.Nh * 3;
    // ---- the whole pair is NaN unless everything it is made of is a finite number and the object has vertices (wave-uniform up to the vote)
    int bad = !(o >= 0 && o < a.acc.n_obj);
    int kb = 0, ke = 0;
    if (!bad) {
        kb = a.acc.clu_offset[o]; ke = a.acc.clu_offset[o + 1];
        bad = !(ke > kb && a.acc.clu_start[ke] > a.acc.clu_start[kb]);
    }
    for (int i = 0; i < 12; ++i) bad |= !isfinite(R[i]);
    for (int i = 0; i < 3; ++i) bad |= !isfinite(root[i]);
    if (!bad)
        for (int i = tid; i < a.Nh * 3; i += CM_THREADS) bad |= !(isfinite(V[i]) && isfinite(N[i]));
    bad = __syncthreads_or(bad);
    if (bad) {
        for (int vi = tid; vi < a.Nh; vi += CM_THREADS) {
            a.weight[hyp * a.Nh + vi] = NAN;
            if (a.nn) a.nn[hyp * a.Nh + vi] = -1;
            if (a.nd) a.nd[hyp * a.Nh + vi] = NAN;
            if (a.vd) a.vd[hyp * a.Nh + vi] = NAN;
        }
        return;
    }
    contact_multi_pair(read_only(a.acc.vert), read_only(a.acc.index), read_only(a.acc.clu_start), read_only(a.acc.clu_sphere), V, N, read_only(R),
                       read_only(root), a.weight + hyp * a.Nh, a.nn ? a.nn + hyp * a.Nh : nullptr,
                       a.nd ? a.nd + hyp * a.Nh : nullptr, a.vd ? a.vd + hyp * a.Nh : nullptr, kb, ke, a.Nh, a.right[img] ? 1.0 : -1.0, a.lo, a.hi, a.vt,
                       a.mid1, a.mid2, a.w0);
}

__device__ __forceinline__ void contact_multi_pair(ro<double> vert, ro<int> index, ro<int> clu_start, ro<double> sphere, const float* __restrict__ V,
                                                   const float* __restrict__ N, ro<double> R, ro<double> root, float* __restrict__ weight,
                                                   int* __restrict__ nn, double* __restrict__ ndo, double* __restrict__ vdo, int kb, int ke, int Nh,
                                                   double sg, double lo, double hi, double vt, double mid1, double mid2, double w0) {
    const int tid = threadIdx.x;
    const double grow = 1.0 + 0x1p-20;
    // a wave stops at its first round without a live vertex (wave-uniform; no barrier in this loop)
    for (int v0 = __builtin_amdgcn_readfirstlane(tid & ~63); v0 < Nh; v0 += CM_THREADS) {
        const int vi = v0 + (tid & 63);
        const bool live = vi < Nh;
        double px = 0.0, py = 0.0, pz = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
        if (live) {
            const float* h = V + (long long)vi * 3;
            const float* g = N + (long long)vi * 3;
            const double d0 = ((double)h[0] * sg + root[0]) - R[3], d1 = ((double)h[1] + root[1]) - R[7], d2 = ((double)h[2] + root[2]) - R[11];
            px = R[0] * d0 + R[4] * d1 + R[8] * d2;
            py = R[1] * d0 + R[5] * d1 + R[9] * d2;
            pz = R[2] * d0 + R[6] * d1 + R[10] * d2;
            const double n0 = (double)g[0] * sg, n1 = (double)g[1], n2 = (double)g[2];
            mx = R[0] * n0 + R[4] * n1 + R[8] * n2;
            my = R[1] * n0 + R[5] * n1 + R[9] * n2;
            mz = R[2] * n0 + R[6] * n1 + R[10] * n2;
        }
        // ---- nearest vertex: the cluster with the nearest centre first, then every cluster the bound cannot reject
        int seed = kb;
        double seed_d2 = INFINITY;
#pragma unroll 4
        for (int k = kb; k < ke; ++k) {
            ro<double> s = sphere + (long long)k * 4;
            const double dx = px - s[0], dy = py - s[1], dz = pz - s[2];
            const double D2 = dot3(dx, dy, dz, dx, dy, dz);
            if (D2 < seed_d2) { seed_d2 = D2; seed = k; }
        }
        double best = INFINITY;
        int bi = 0x7fffffff, bj = clu_start[kb];          // original index and table row of the nearest vertex so far
        {
            const int je = clu_start[seed + 1];
#pragma unroll 4
            for (int j = clu_start[seed]; j < je; ++j) {
                ro<double> v = vert + (long long)j * 3;
                const double dx = px - v[0], dy = py - v[1], dz = pz - v[2];
                const double q = dot3(dx, dy, dz, dx, dy, dz);
                const int idx = index[j];
                if (q < best || (q == best && idx < bi)) { best = q; bi = idx; bj = j; }
            }
        }
        double reach = sqrt(best) * grow;
        for (int k = kb; k < ke; ++k) {
            ro<double> s = sphere + (long long)k * 4;
            const double dx = px - s[0], dy = py - s[1], dz = pz - s[2];
            const double D2 = dot3(dx, dy, dz, dx, dy, dz);
            const double lim = reach + s[3];
            if (live && k != seed && !(D2 > lim * lim)) {
                const int je = clu_start[k + 1];
#pragma unroll 4
                for (int j = clu_start[k]; j < je; ++j) {
                    ro<double> v = vert + (long long)j * 3;
                    const double ex = px - v[0], ey = py - v[1], ez = pz - v[2];
                    const double q = dot3(ex, ey, ez, ex, ey, ez);
                    const int idx = index[j];
                    if (q < best || (q == best && idx < bi)) { best = q; bi = idx; bj = j; }
                }
                reach = sqrt(best) * grow;
            }
        }
        if (live) {
            ro<double> v = vert + (long long)bj * 3;
            const double ex = px - v[0], ey = py - v[1], ez = pz - v[2];
            const double nd = dot3(ex, ey, ez, mx, my, mz);
            const double rx = ex - nd * mx, ry = ey - nd * my, rz = ez - nd * mz;
            const double vd = sqrt(dot3(rx, ry, rz, rx, ry, rz));
            const bool in = nd > lo && nd < hi && vd < vt;
            const int at = vi;
            weight[at] = in ? (float)fmin(fmax(contact_weight(nd, mid1, mid2) / w0, 0.0), 1.0) : 0.f;
            if (nn) nn[at] = in ? bi : -1;
            if (ndo) ndo[at] = nd;
            if (vdo) vdo[at] = vd;
        }
    }
}

struct AgreeArgs {
    const float *w, *w_gt;               // (n, S, Nh), (n, Nh)
    const float *fc, *fc_gt;             // (n, S, 32), (n, 32)
    const unsigned char *gr, *gr_gt;     // (n, S), (n,)
    int n, S, Nh;
    int* counts;                         // (n, S, 3)   TP, P, G
    double* values;                      // (n, S, 8)
    double* table;                       // (n, 24)
};

// one workgroup per (image, hypothesis): TP / P / G, sum |w - w_gt| (per-thread strided partial sums, then a halving tree: a fixed order)
__global__ __launch_bounds__(CM_THREADS) void contact_agreement_kernel(const AgreeArgs a) {
    __shared__ double s_mae[CM_THREADS];
    __shared__ int s_tp[CM_THREADS], s_p[CM_THREADS], s_g[CM_THREADS], s_nan[CM_THREADS];
    const long long hyp = blockIdx.x;
    const int img = (int)(hyp / a.S), tid = threadIdx.x;
    const float* W = a.w + hyp * a.Nh;
    const float* G = a.w_gt + (long long)img * a.Nh;
    int tp = 0, p = 0, g = 0, nan = 0;
    double mae = 0.0;
    for (int i = tid; i < a.Nh; i += CM_THREADS) {
        const float w = W[i], t = G[i];
        nan |= (w != w) || (t != t);
        const int c = w > 0.f, d = t > 0.f;
        tp += c & d; p += c; g += d;
        mae += fabs((double)w - (double)t);
    }
    s_mae[tid] = mae; s_tp[tid] = tp; s_p[tid] = p; s_g[tid] = g; s_nan[tid] = nan;
    __syncthreads();
    for (int h = CM_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            s_mae[tid] += s_mae[tid + h]; s_tp[tid] += s_tp[tid + h]; s_p[tid] += s_p[tid + h]; s_g[tid] += s_g[tid + h];
            s_nan[tid] |= s_nan[tid + h];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    int* cnt = a.counts + hyp * 3;
    double* out = a.values + hyp * CM_VALUES;
    if (s_nan[0]) {
        cnt[0] = cnt[1] = cnt[2] = 0;
        for (int j = 0; j < CM_VALUES; ++j) out[j] = NAN;
        return;
    }
    const int TP = s_tp[0], P = s_p[0], Gn = s_g[0];
    cnt[0] = TP; cnt[1] = P; cnt[2] = Gn;
    int same = 0;
    for (int k = 0; k < 32; ++k) same += (a.fc[hyp * 32 + k] > 0.f) == (a.fc_gt[(long long)img * 32 + k] > 0.f);
    const int gr = a.gr[hyp] ? 1 : 0, gt = a.gr_gt[img] ? 1 : 0;
    out[0] = (P + Gn - TP) ? (double)TP / (double)(P + Gn - TP) : NAN;
    out[1] = P ? (double)TP / (double)P : NAN;
    out[2] = Gn ? (double)TP / (double)Gn : NAN;
    out[3] = (P + Gn) ? (double)(2 * TP) / (double)(P + Gn) : NAN;
    out[4] = s_mae[0] / (double)a.Nh;
    out[5] = (double)same / 32.0;
    out[6] = (double)gr;
    out[7] = gr == gt ? 1.0 : 0.0;
}

// one thread per (image, value): hypothesis 0 | best-of-S (max; min for MAE) | mean-of-S (sum in ascending s / how many), NaNs left out
__global__ __launch_bounds__(256) void contact_agreement_table_kernel(const AgreeArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.n * CM_VALUES) return;
    const long long img = i / CM_VALUES;
    const int j = (int)(i % CM_VALUES);
    const double* src = a.values + img * a.S * CM_VALUES + j;
    double best = NAN, sum = 0.0;
    int cnt = 0;
    for (int s = 0; s < a.S; ++s) {
        const double v = src[(long long)s * CM_VALUES];
        if (v != v) continue;
        best = cnt == 0 ? v : (j == CM_MAE ? fmin(best, v) : fmax(best, v));
        sum += v;
        ++cnt;
    }
    double* out = a.table + img * (3 * CM_VALUES) + j;
    out[0] = src[0];
    out[CM_VALUES] = best;
    out[2 * CM_VALUES] = cnt ? sum / (double)cnt : NAN;
}

}  // namespace

extern "C" int vpho_contact_multi_f32(const vpho_obj_vertex_accel* acc, const float* hand_verts, const float* hand_normals, int n, int S, int Nh,
                                      const double* root, const unsigned char* is_right, const double* obj_rt, const int* obj_id,
                                      float normal_lo, float normal_hi, float vertical_thresh, float decay_lo, float decay_hi,
                                      float* weight, int* nn_index, double* nd, double* vd, void* stream) {
    VPHO_REQUIRE(acc && acc->vert && acc->index && acc->clu_offset && acc->clu_start && acc->clu_sphere && acc->n_obj > 0,
                 "vpho_contact_multi_f32: bad vertex tables");
    VPHO_REQUIRE(n >= 0 && S > 0 && Nh > 0 && (long long)n * S <= 0x7fffffffLL && (long long)Nh * 3 <= 0x7fffffffLL,
                 "vpho_contact_multi_f32: bad shape (n=%d, S=%d, Nh=%d)", n, S, Nh);
    VPHO_REQUIRE(normal_lo < decay_lo && decay_lo < decay_hi && decay_hi < normal_hi && vertical_thresh > 0,
                 "vpho_contact_multi_f32: thresholds must satisfy normal_lo < decay_lo < decay_hi < normal_hi");
    if (n == 0) return 0;
    VPHO_REQUIRE(hand_verts && hand_normals && root && is_right && obj_rt && obj_id && weight, "vpho_contact_multi_f32: bad argument");
    ContactMultiArgs a;
    a.acc = *acc; a.hv = hand_verts; a.hn = hand_normals; a.root = root; a.right = is_right; a.rt = obj_rt; a.obj_id = obj_id;
    a.S = S; a.Nh = Nh;
    a.lo = normal_lo; a.hi = normal_hi; a.vt = vertical_thresh;
    a.mid1 = ((double)decay_lo + (double)normal_lo) / 2; a.mid2 = ((double)decay_hi + (double)normal_hi) / 2;
    {
        const double m1 = 1.0 + std::exp(-1600.0 * (0.0 - a.mid1)), m2 = 1.0 + std::exp(1600.0 * (0.0 - a.mid2));
        a.w0 = 1.0 / (m1 * m2 + 1e-10);
    }
    a.weight = weight; a.nn = nn_index; a.nd = nd; a.vd = vd;
    hipLaunchKernelGGL(contact_multi_kernel, dim3((unsigned)((long long)n * S)), dim3(CM_THREADS), 0, (hipStream_t)stream, a);
    return vpho::check_launch("contact_multi_kernel");
}

extern "C" int vpho_contact_agreement_f32(const float* weight, const float* weight_gt, const float* force_contact, const unsigned char* is_grasped,
                                          const float* force_contact_gt, const unsigned char* is_grasped_gt, int n, int S, int Nh,
                                          int* counts, double* values, double* table, void* stream) {
    VPHO_REQUIRE(n >= 0 && S > 0 && Nh > 0 && (long long)n * S <= 0x7fffffffLL, "vpho_contact_agreement_f32: bad shape (n=%d, S=%d, Nh=%d)", n, S, Nh);
    if (n == 0) return 0;
    VPHO_REQUIRE(weight && weight_gt && force_contact && is_grasped && force_contact_gt && is_grasped_gt && counts && values && table,
                 "vpho_contact_agreement_f32: bad argument");
    hipStream_t s = (hipStream_t)stream;
    AgreeArgs a;
    a.w = weight; a.w_gt = weight_gt; a.fc = force_contact; a.fc_gt = force_contact_gt; a.gr = is_grasped; a.gr_gt = is_grasped_gt;
    a.n = n; a.S = S; a.Nh = Nh; a.counts = counts; a.values = values; a.table = table;
    hipLaunchKernelGGL(contact_agreement_kernel, dim3((unsigned)((long long)n * S)), dim3(CM_THREADS), 0, s, a);
    int rc = vpho::check_launch("contact_agreement_kernel");
    if (!rc) {
        hipLaunchKernelGGL(contact_agreement_table_kernel, dim3((unsigned)(((long long)n * CM_VALUES + 255) / 256)), dim3(256), 0, s, a);
        rc = vpho::check_launch("contact_agreement_table_kernel");
    }
    return rc;
}
