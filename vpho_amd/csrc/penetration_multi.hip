// Hand-object penetration and contact of EVERY sampled hypothesis (--eval_best with --eval_physics): the metric of
// penetration.hip for the n x S (hand hypothesis s, object hypothesis s) pairs, bit for bit, without its visit of every triangle by every
// vertex.  Two conservative filters, built on the host (vpho_amd/physics_eval.py mesh_accel, include/vpho_hip.h vpho_obj_mesh_accel):
//   parity: a vertex walks the triangle list of the 8 x 8-cell column its own hash cell lies in (ascending triangle index) and applies
//     the cell test and the strict containment of penetration.hip to every entry.  A triangle is in the list of every column its cell
//     rectangle touches, so the list only lacks triangles the cell test rejects; the parities are XOR counts: the same bits.
//   nearest: the triangles in Morton order, in clusters of 16 with a bounding sphere.  A vertex first takes the cluster with the nearest
//     centre (its own gather), then all clusters in order, skipping those whose sphere is out of reach; every other triangle goes through
//     tri_dist2_geo (penetration_common.h), the arithmetic of penetration.hip on bit copies of its record fields and the same p.  fmin
//     over fp64 is exact and order-free, so best has the brute-force bits as long as no skipped triangle could have lowered it:
//       skip iff  D > reach + r,   D = |p - centre|,  reach = sqrt(best) (1 + 2^-20),  r = r0 (1 + 2^-30) + 2^-30 diag   (all fp64)
//     with r0 the exact-arithmetic radius about the centre and diag the mesh's bounding-box diagonal.  In exact arithmetic a triangle T
//     of the cluster has d_T >= D - r0.  Rounding: (i) D^2, (reach + r)^2 and r0 are each a handful of fp64 operations on
//     non-negative terms, relative error < 8 eps = 2^-50: covered 2^20-fold by the two inflations; (ii) tri_dist2 returns |e|^2 of
//     a vector e it forms with absolute error <= c eps L per component, L <= d_T + diag the size of the operands (point to corner, edges)
//     and c < 32, so computed(T) >= (d_T - c eps L)^2 and best <= (d* + c eps L*)^2 for the triangle T* that set it.  A skip means
//     d_T - d* > 2^-20 d* + 2^-30 diag.  What has to be covered is c eps (L + L*) <= 2^-48 (d_T + d* + 2 diag): for d_T <= 2 d* + diag
//     that is at most 2^-48 (3 d* + 3 diag), far below the gap; for a larger d_T the gap d_T - d* > d_T / 2 exceeds 2^-48 (3.5 d_T).
//     So computed(T) >= best and the minimum keeps its bits.
//     The seed only tightens best early; a NaN anywhere fails the skip test, so the cluster is visited.
// One workgroup per (image, hypothesis): the hypothesis' pose and the cluster spheres are wave-uniform (scalar loads), a wave holds 64
// consecutive vertices, and PD / count / min sd are reduced in the workgroup -- nothing per vertex is written unless sd / inside are
// asked for.  A second, tiny launch reduces the S hypotheses of an image to the one | best | mean table.
// No LDS staging: the lists are short and read through L2 (column lists per lane, cluster geometry per wave).
// gfx950, -O3: penetration_multi_kernel 78 VGPRs, no scratch, 5 KB LDS (the three reduction arrays); penetration_table_kernel 20 VGPRs.
#include "common.h"
#include "../../include/vpho_hip.h"
#include "penetration_common.h"

namespace {

constexpr int PM_THREADS = 256;
constexpr int TS = VPHO_PEN_TRI_STRIDE;
constexpr int CLU = VPHO_PEN_CLUSTER;
constexpr int COLS = VPHO_PEN_COLUMNS;
constexpr int CELLS = VPHO_PEN_RESOLUTION / COLS;      // hash cells per column side
static_assert(COLS * CELLS == VPHO_PEN_RESOLUTION, "columns tile the hash cells");

struct PenMultiArgs {
    vpho_obj_mesh_tables t;
    vpho_obj_mesh_accel acc;
    const float* verts;          // (n, S, V, 3)
    const double* rt;            // (n, S, 3, 4)
    const int* obj_id;           // (n,)
    int n, S, V;
    double thresh;
    double* per_hyp;             // (n, S, 4)
    double* sd;                  // (n, S, V) or NULL
    unsigned char* inside;       // (n, S, V) or NULL
    double* table;               // (n, 12)
};

__global__ __launch_bounds__(PM_THREADS) void penetration_multi_kernel(const PenMultiArgs a) {
    __shared__ double s_pd[PM_THREADS], s_min[PM_THREADS];
    __shared__ int s_cnt[PM_THREADS];
    const long long hyp = blockIdx.x;                  // image * S + hypothesis
    const int img = (int)(hyp / a.S), tid = threadIdx.x;
    const int o = a.obj_id[img];
    if (!(o >= 0 && o < a.t.n_obj)) {                  // the whole workgroup: NaN, as penetration.hip
        for (int vi = tid; vi < a.V; vi += PM_THREADS) {
            if (a.sd) a.sd[hyp * a.V + vi] = NAN;
            if (a.inside) a.inside[hyp * a.V + vi] = 0;
        }
        if (tid < 4) a.per_hyp[hyp * 4 + tid] = NAN;
        return;
    }
    const double* R = a.rt + hyp * 12;
    const double* sc = a.t.scale + 3 * o;
    const double* tr = a.t.translate + 3 * o;
    const int kb = a.acc.clu_offset[o], ke = a.acc.clu_offset[o + 1];
    const int* coff = a.acc.col_offset + (long long)o * (COLS * COLS);
    double pd = 0.0, mn = INFINITY;
    int cnt = 0;
    bool nan = false;
    // a wave stops at its first round without a live vertex (wave-uniform; no barrier in this loop)
    for (int v0 = __builtin_amdgcn_readfirstlane(tid & ~63); v0 < a.V; v0 += PM_THREADS) {
        const int vi = v0 + (tid & 63);
        const bool live = vi < a.V;
        // p = R^T (v - t) in the model frame; q = scale * p + translate in the hash frame (the expressions of penetration.hip)
        double px = 0.0, py = 0.0, pz = 0.0, qx = 0.0, qy = 0.0, qz = 0.0;
        if (live) {
            pen_model_frame(R, a.verts + (hyp * a.V + vi) * 3, px, py, pz);
            pen_hash_frame(sc, tr, px, py, pz, qx, qy, qz);
        }
        // ---- nearest triangle: the cluster with the nearest centre first, then every cluster the bound cannot reject
        int seed = kb;
        double seed_d2 = INFINITY;
        for (int k = kb; k < ke; ++k) {
            const double* s = a.acc.clu_sphere + (long long)k * 4;
            const double dx = px - s[0], dy = py - s[1], dz = pz - s[2];
            const double D2 = dot3(dx, dy, dz, dx, dy, dz);
            if (D2 < seed_d2) { seed_d2 = D2; seed = k; }
        }
        double best = INFINITY;
        {
            const double* g = a.acc.clu_geo + (long long)seed * (CLU * 9);
#pragma unroll 1
            for (int j = 0; j < CLU; ++j) best = fmin(best, tri_dist2_geo(g + j * 9, px, py, pz));
        }
        const double grow = 1.0 + 0x1p-20;
        double reach = sqrt(best) * grow;
        for (int k = kb; k < ke; ++k) {
            const double* s = a.acc.clu_sphere + (long long)k * 4;
            const double dx = px - s[0], dy = py - s[1], dz = pz - s[2];
            const double D2 = dot3(dx, dy, dz, dx, dy, dz);
            const double lim = reach + s[3];
            if (live && k != seed && !(D2 > lim * lim)) {
                const double* g = a.acc.clu_geo + (long long)k * (CLU * 9);
#pragma unroll 1
                for (int j = 0; j < CLU; ++j) best = fmin(best, tri_dist2_geo(g + j * 9, px, py, pz));
                reach = sqrt(best) * grow;
            }
        }
        // ---- z-ray parity over the triangles of the vertex' own column
        double cx, cy;
        const bool has_cell = pen_cell(qx, qy, qz, cx, cy) && live;
        unsigned par0 = 0, par1 = 0;
        if (has_cell) {
            const int col = ((int)cy / CELLS) * COLS + (int)cx / CELLS;
            const int le = coff[col + 1];
            for (int i = coff[col]; i < le; ++i) {
                const double* r = a.t.tri + (long long)a.acc.col_tri[i] * TS;
                pen_parity_step(r, qx, qy, qz, cx, cy, par0, par1);
            }
        }
        if (live) {
            const bool ins = par0 && par1;
            const double d = sqrt(best);
            const double s = ins ? -d : d;
            if (a.sd) a.sd[hyp * a.V + vi] = s;
            if (a.inside) a.inside[hyp * a.V + vi] = ins ? 1 : 0;
            nan |= s != s;
            if (ins) { pd = fmax(pd, -s); ++cnt; }
            mn = fmin(mn, s);
        }
    }
    // PD = max d over the inside vertices (0 if none), n_inside, min sd, contact = (min sd <= thresh): penetration_reduce_kernel's rule
    s_pd[tid] = pd; s_min[tid] = nan ? NAN : mn; s_cnt[tid] = cnt;
    __syncthreads();
    for (int h = PM_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            s_pd[tid] = fmax(s_pd[tid], s_pd[tid + h]);
            const double m0 = s_min[tid], m1 = s_min[tid + h];
            s_min[tid] = (m0 != m0 || m1 != m1) ? NAN : fmin(m0, m1);
            s_cnt[tid] += s_cnt[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool bad = s_min[0] != s_min[0];
        double* out = a.per_hyp + hyp * 4;
        out[0] = bad ? NAN : s_pd[0];
        out[1] = bad ? NAN : (double)s_cnt[0];
        out[2] = bad ? NAN : s_min[0];
        out[3] = bad ? NAN : (s_min[0] <= a.thresh ? 1.0 : 0.0);
    }
}

// one thread per (image, metric): one = hypothesis 0, best = min PD / min n_inside / max min-sd / max contact, mean = sum in ascending s / S
__global__ __launch_bounds__(256) void penetration_table_kernel(const PenMultiArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.n * 4) return;
    const long long img = i >> 2;
    const int j = (int)(i & 3);
    const double* src = a.per_hyp + img * a.S * 4 + j;
    double lo = INFINITY, hi = -INFINITY, sum = 0.0;
    bool nan = false;
    for (int s = 0; s < a.S; ++s) {
        const double v = src[(long long)s * 4];
        nan |= v != v;
        lo = fmin(lo, v);
        hi = fmax(hi, v);
        sum += v;
    }
    double* out = a.table + img * 12 + j;
    out[0] = src[0];
    out[4] = nan ? NAN : (j < 2 ? lo : hi);
    out[8] = sum / (double)a.S;
}

}  // namespace

extern "C" int vpho_hand_obj_penetration_multi_f64(const vpho_obj_mesh_tables* t, const vpho_obj_mesh_accel* acc, const float* verts, int n, int S,
                                                   int V, const double* obj_rt, const int* obj_id, double contact_thresh, double* per_hyp,
                                                   double* sd, unsigned char* inside, double* table, void* stream) {
    VPHO_REQUIRE(t && t->tri && t->tri_offset && t->scale && t->translate && t->n_obj > 0, "vpho_hand_obj_penetration_multi_f64: bad mesh tables");
    VPHO_REQUIRE(acc && acc->col_offset && acc->col_tri && acc->clu_offset && acc->clu_sphere && acc->clu_geo,
                 "vpho_hand_obj_penetration_multi_f64: bad acceleration tables");
    VPHO_REQUIRE(n >= 0 && S > 0 && V > 0 && (long long)n * S <= 0x7fffffffLL, "vpho_hand_obj_penetration_multi_f64: bad shape (n=%d, S=%d, V=%d)", n, S, V);
    if (n == 0) return 0;
    VPHO_REQUIRE(verts && obj_rt && obj_id && per_hyp && table, "vpho_hand_obj_penetration_multi_f64: bad argument");
    hipStream_t s = (hipStream_t)stream;
    PenMultiArgs a;
    a.t = *t; a.acc = *acc; a.verts = verts; a.rt = obj_rt; a.obj_id = obj_id; a.n = n; a.S = S; a.V = V; a.thresh = contact_thresh;
    a.per_hyp = per_hyp; a.sd = sd; a.inside = inside; a.table = table;
    hipLaunchKernelGGL(penetration_multi_kernel, dim3((unsigned)((long long)n * S)), dim3(PM_THREADS), 0, s, a);
    int rc = vpho::check_launch("penetration_multi_kernel");
    if (!rc) {
        hipLaunchKernelGGL(penetration_table_kernel, dim3((unsigned)(((long long)n * 4 + 255) / 256)), dim3(256), 0, s, a);
        rc = vpho::check_launch("penetration_table_kernel");
    }
    return rc;
}
