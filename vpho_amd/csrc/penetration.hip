// Hand-object penetration and contact (--eval_physics).  For every hand vertex of an image, in the object's model
// frame p = R^T (v - t) (fp64):
//   inside(p): the z-ray parity rule of the occupancy-networks MeshIntersector at resolution 512 -- rescale p into the object's
//     [0.5, 511.5]^3 box, cull to [0, 512]^3, count the triangles whose rescaled xy projection STRICTLY contains p (a triangle only
//     counts when p's own 512x512 cell lies in the triangle's integer-truncated xy bounding cells, as the triangle hash of that test
//     does), split them by the plane depth at p against p_z |n_z|, inside iff both counts are odd.  Triangles with det A == 0 or
//     n_z == 0 never count (their depth is NaN: in neither bucket).
//   d(p): exact unsigned distance to the nearest triangle (closest point by Voronoi regions, Ericson, "Real-Time Collision
//     Detection" 5.1.5), metres.   sd = -d if inside else d.
// The point-independent terms of every triangle come from the host (vpho_amd/physics_eval.py, numpy, in the order of operations of
// that test); the point-dependent ones below keep its order too, and the library is built with -ffp-contract=off: the inside flags
// are bit-for-bit those of the host test.  Max / min / count reductions: exact, so every result is deterministic.
#include "common.h"
#include "../../include/vpho_hip.h"
#include "penetration_common.h"

namespace {

constexpr int PEN_THREADS = 256;
constexpr int PEN_TILE = 256;                          // triangles staged per LDS tile: 256 x 28 doubles = 56 KB
constexpr int TS = VPHO_PEN_TRI_STRIDE;

struct PenArgs {
    vpho_obj_mesh_tables t;
    const float* verts;          // (n, V, 3)
    const double* rt;            // (n, 3, 4)
    const int* obj_id;           // (n,)
    int n, V;
    double thresh;
    double* sd;                  // (n, V)
    unsigned char* inside;       // (n, V)
    double* per_image;           // (n, 4)
};

__global__ __launch_bounds__(PEN_THREADS) void penetration_kernel(const PenArgs a) {
    __shared__ double tile[PEN_TILE * TS];
    const int img = blockIdx.y, vi = blockIdx.x * PEN_THREADS + threadIdx.x;
    const int o = a.obj_id[img];
    const bool ok_obj = o >= 0 && o < a.t.n_obj;
    const bool live = vi < a.V;
    // p = R^T (v - t) in the model frame; q = scale * p + translate in the hash frame
    double px = 0.0, py = 0.0, pz = 0.0, qx = 0.0, qy = 0.0, qz = 0.0;
    int tb = 0, te = 0;
    if (ok_obj) {
        tb = a.t.tri_offset[o];
        te = a.t.tri_offset[o + 1];
        if (live) {
            pen_model_frame(a.rt + (long long)img * 12, a.verts + ((long long)img * a.V + vi) * 3, px, py, pz);
            pen_hash_frame(a.t.scale + 3 * o, a.t.translate + 3 * o, px, py, pz, qx, qy, qz);
        }
    }
    double cx, cy;
    const bool has_cell = pen_cell(qx, qy, qz, cx, cy);
    unsigned par0 = 0, par1 = 0;
    double best = INFINITY;
    for (int t0 = tb; t0 < te; t0 += PEN_TILE) {
        const int cnt = min(PEN_TILE, te - t0);
        __syncthreads();
        const double* src = a.t.tri + (long long)t0 * TS;
        for (int i = threadIdx.x; i < cnt * TS; i += PEN_THREADS) tile[i] = src[i];
        __syncthreads();
        if (!live) continue;
        for (int k = 0; k < cnt; ++k) {
            const double* r = tile + k * TS;
            best = fmin(best, tri_dist2(r, px, py, pz));
            if (has_cell) pen_parity_step(r, qx, qy, qz, cx, cy, par0, par1);
        }
    }
    if (!live) return;
    const long long idx = (long long)img * a.V + vi;
    const bool ins = ok_obj && par0 && par1;
    const double d = sqrt(best);
    if (a.sd) a.sd[idx] = ok_obj ? (ins ? -d : d) : NAN;
    if (a.inside) a.inside[idx] = ins ? 1 : 0;
}

// one workgroup per image: PD = max d over the inside vertices (0 if none), n_inside, min sd, contact = (min sd <= thresh)
__global__ __launch_bounds__(256) void penetration_reduce_kernel(const PenArgs a) {
    __shared__ double s_pd[256], s_min[256];
    __shared__ int s_cnt[256];
    const int img = blockIdx.x, tid = threadIdx.x;
    const double* sd = a.sd + (long long)img * a.V;
    const unsigned char* ins = a.inside + (long long)img * a.V;
    double pd = 0.0, mn = INFINITY;
    int cnt = 0;
    bool nan = false;
    for (int i = tid; i < a.V; i += 256) {
        const double s = sd[i];
        nan |= s != s;
        if (ins[i]) { pd = fmax(pd, -s); ++cnt; }
        mn = fmin(mn, s);
    }
    s_pd[tid] = pd; s_min[tid] = nan ? NAN : mn; s_cnt[tid] = cnt;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            s_pd[tid] = fmax(s_pd[tid], s_pd[tid + h]);
            const double m0 = s_min[tid], m1 = s_min[tid + h];
            s_min[tid] = (m0 != m0 || m1 != m1) ? NAN : fmin(m0, m1);
            s_cnt[tid] += s_cnt[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int o = a.obj_id[img];
        const bool bad = !(o >= 0 && o < a.t.n_obj) || s_min[0] != s_min[0];
        double* out = a.per_image + (long long)img * 4;
        out[0] = bad ? NAN : s_pd[0];
        out[1] = bad ? NAN : (double)s_cnt[0];
        out[2] = bad ? NAN : s_min[0];
        out[3] = bad ? NAN : (s_min[0] <= a.thresh ? 1.0 : 0.0);
    }
}

}  // namespace

extern "C" int vpho_hand_obj_penetration_f64(const vpho_obj_mesh_tables* t, const float* verts, int n, int V, const double* obj_rt,
                                             const int* obj_id, double contact_thresh, double* sd, unsigned char* inside, double* per_image,
                                             void* stream) {
    VPHO_REQUIRE(t && t->tri && t->tri_offset && t->scale && t->translate && t->n_obj > 0, "vpho_hand_obj_penetration_f64: bad mesh tables");
    VPHO_REQUIRE(n >= 0 && V > 0 && n <= 65535, "vpho_hand_obj_penetration_f64: bad shape (n=%d, V=%d)", n, V);
    if (n == 0) return 0;
    VPHO_REQUIRE(verts && obj_rt && obj_id && per_image, "vpho_hand_obj_penetration_f64: bad argument");
    hipStream_t s = (hipStream_t)stream;
    PenArgs a;
    a.t = *t; a.verts = verts; a.rt = obj_rt; a.obj_id = obj_id; a.n = n; a.V = V; a.thresh = contact_thresh;
    a.per_image = per_image;
    // sd / inside may be NULL: then they live in a stream-ordered temporary block
    void* tmp = nullptr;
    const size_t nv = (size_t)n * V;
    if (!sd || !inside) {
        VPHO_HIP(hipMallocAsync(&tmp, nv * (sizeof(double) + 1), s));
    }
    a.sd = sd ? sd : (double*)tmp;
    a.inside = inside ? inside : (unsigned char*)tmp + nv * sizeof(double);
    hipLaunchKernelGGL(penetration_kernel, dim3((V + PEN_THREADS - 1) / PEN_THREADS, n), dim3(PEN_THREADS), 0, s, a);
    int rc = vpho::check_launch("penetration_kernel");
    if (!rc) {
        hipLaunchKernelGGL(penetration_reduce_kernel, dim3(n), dim3(256), 0, s, a);
        rc = vpho::check_launch("penetration_reduce_kernel");
    }
    if (tmp) VPHO_HIP(hipFreeAsync(tmp, s));
    return rc;
}
