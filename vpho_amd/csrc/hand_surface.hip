// Hand surface for the contact labels: vertex normals of the posed hand mesh and the finger-gap fill.  Replaces, per sample,
// lib/dataset/base.py:887-891 (trimesh.Trimesh(hand_verts, hand_faces).vertex_normals, n / (|n| + 1e-20), fill, n / (|n| + 1e-20))
// and lib/utils/hand_fn.py:294-384 (fill_finger_gaps_in_mano: 778 -> 1080 rows).  The reference does this on the CPU for one
// frame at a time; here one 256-thread workgroup takes one sample and nothing leaves the device between the hand vertices
// and vpho_contact_detect_f32.
//
// Normal rule (a restatement of trimesh's angle-weighted vertex normals, not a comparison with trimesh):
//   face normal  = cross(v1 - v0, v2 - v0) / |.|; a face whose cross product is EXACTLY zero contributes nothing
//   corner angle = acos(clamp(u . w, -1, 1)) of the two unit edge vectors that leave the corner
//   vertex sum   = sum over the incident (face, corner) pairs, in the table's fixed CSR order, of angle * face normal
//   normal       = sum / |sum| (the zero vector when |sum| is zero: an unreferenced vertex, cancelling faces), then n / (|n| + 1e-20)
// Fill rule: row V + l = alpha[l] * x[links[l][0]] + (1 - alpha[l]) * x[links[l][1]] for the vertices and for the normals,
// then every normal row once more n / (|n| + 1e-20).
// fp64 from the fp32 vertices throughout, never contracted (-ffp-contract=off), each output rounded to fp32 once; no atomics, so
// two runs give the same bits.  A NaN coordinate reaches its faces (the comparisons below are written so that a NaN is not taken
// for a degenerate face), through them the normals of their vertices, and the links that read either; nothing else.
// LDS per workgroup: face records F x 6 doubles (unit normal, three corner angles), normals V x 3 doubles, vertices V x 3 floats:
// 96 KB + 24 KB + 12 KB at the limits V = 1024, F = 2048 (the large-LDS opt-in of vpho::dynamic_lds).
#include "common.h"
#include "../../include/vpho_hip.h"

namespace {

constexpr int HS_MAX_V = 1024, HS_MAX_F = 2048, HS_MAX_L = 1024;

struct HandSurfaceArgs {
    const float* verts;
    vpho_hand_surface_table t;
    float *verts_filled, *normals_filled;
};

__device__ inline double hs_clamp1(double c) { return c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c); }   // keeps a NaN (fmin / fmax would drop it)

// angle at p between the edges to q and r
__device__ inline double hs_corner(const double* p, const double* q, const double* r) {
    const double ux = q[0] - p[0], uy = q[1] - p[1], uz = q[2] - p[2];
    const double wx = r[0] - p[0], wy = r[1] - p[1], wz = r[2] - p[2];
    const double lu = sqrt(ux * ux + uy * uy + uz * uz), lw = sqrt(wx * wx + wy * wy + wz * wz);
    return acos(hs_clamp1((ux / lu) * (wx / lw) + (uy / lu) * (wy / lw) + (uz / lu) * (wz / lw)));
}

__global__ __launch_bounds__(256) void hand_surface_kernel(const HandSurfaceArgs a) {
    extern __shared__ __attribute__((aligned(16))) double hs_sm[];
    const int V = a.t.V, F = a.t.F, L = a.t.L, tid = threadIdx.x;
    double* s_rec = hs_sm;                                   // [F][6]: unit face normal, angles at corners 0, 1, 2
    double* s_n = s_rec + F * 6;                             // [V][3]
    float* s_v = reinterpret_cast<float*>(s_n + V * 3);      // [V][3]
    const long long sample = blockIdx.x;
    const float* X = a.verts + sample * V * 3;
    float* VO = a.verts_filled + sample * (V + L) * 3;
    float* NO = a.normals_filled + sample * (V + L) * 3;
    for (int i = tid; i < V * 3; i += 256) {
        const float x = X[i];
        s_v[i] = x;
        VO[i] = x;
    }
    __syncthreads();
    for (int f = tid; f < F; f += 256) {
        double p[3][3];
        for (int k = 0; k < 3; ++k) {
            const int vi = a.t.faces[f * 3 + k];
            for (int c = 0; c < 3; ++c) p[k][c] = (double)s_v[vi * 3 + c];
        }
        const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
        const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const double len = sqrt(cx * cx + cy * cy + cz * cz);
        double* r = s_rec + f * 6;
        if (len == 0.0) {                                    // zero area (a NaN length is not zero: it goes on and poisons the face)
            for (int k = 0; k < 6; ++k) r[k] = 0.0;
        } else {
            r[0] = cx / len; r[1] = cy / len; r[2] = cz / len;
            r[3] = hs_corner(p[0], p[1], p[2]);
            r[4] = hs_corner(p[1], p[2], p[0]);
            r[5] = hs_corner(p[2], p[0], p[1]);
        }
    }
    __syncthreads();
    for (int v = tid; v < V; v += 256) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        const int e1 = a.t.csr_offset[v + 1];
        for (int e = a.t.csr_offset[v]; e < e1; ++e) {
            const int ent = a.t.csr_entry[e];
            const double* r = s_rec + (ent >> 2) * 6;
            const double w = r[3 + (ent & 3)];
            sx += w * r[0]; sy += w * r[1]; sz += w * r[2];
        }
        const double len = sqrt(sx * sx + sy * sy + sz * sz);
        if (len == 0.0) { sx = 0.0; sy = 0.0; sz = 0.0; }
        else { sx /= len; sy /= len; sz /= len; }
        const double l2 = sqrt(sx * sx + sy * sy + sz * sz) + 1e-20;          // base.py:889
        s_n[v * 3] = sx / l2; s_n[v * 3 + 1] = sy / l2; s_n[v * 3 + 2] = sz / l2;
    }
    __syncthreads();
    for (int row = tid; row < V + L; row += 256) {
        double nx, ny, nz;
        if (row < V) {
            nx = s_n[row * 3]; ny = s_n[row * 3 + 1]; nz = s_n[row * 3 + 2];
        } else {
            const int l = row - V, i0 = a.t.links[l * 2], i1 = a.t.links[l * 2 + 1];
            const double al = a.t.alpha[l], be = 1.0 - al;                    // hand_fn.py:362-364,376
            for (int c = 0; c < 3; ++c) VO[row * 3 + c] = (float)(al * (double)s_v[i0 * 3 + c] + be * (double)s_v[i1 * 3 + c]);
            nx = al * s_n[i0 * 3] + be * s_n[i1 * 3];
            ny = al * s_n[i0 * 3 + 1] + be * s_n[i1 * 3 + 1];
            nz = al * s_n[i0 * 3 + 2] + be * s_n[i1 * 3 + 2];
        }
        const double l2 = sqrt(nx * nx + ny * ny + nz * nz) + 1e-20;          // base.py:891
        NO[row * 3] = (float)(nx / l2); NO[row * 3 + 1] = (float)(ny / l2); NO[row * 3 + 2] = (float)(nz / l2);
    }
}

}  // namespace

extern "C" int vpho_hand_surface_f32(const vpho_hand_surface_table* t, const float* verts, int n, float* verts_filled, float* normals_filled,
                                     void* stream) {
    VPHO_REQUIRE(t && n >= 0, "vpho_hand_surface_f32: bad argument");
    VPHO_REQUIRE(t->V >= 1 && t->V <= HS_MAX_V, "vpho_hand_surface_f32: %d vertices, the kernel takes 1 .. %d", t->V, HS_MAX_V);
    VPHO_REQUIRE(t->F >= 0 && t->F <= HS_MAX_F, "vpho_hand_surface_f32: %d faces, the kernel takes at most %d", t->F, HS_MAX_F);
    VPHO_REQUIRE(t->L >= 0 && t->L <= HS_MAX_L, "vpho_hand_surface_f32: %d links, the kernel takes at most %d", t->L, HS_MAX_L);
    VPHO_REQUIRE(t->csr_offset && (t->F == 0 || (t->faces && t->csr_entry)) && (t->L == 0 || (t->links && t->alpha)),
                 "vpho_hand_surface_f32: the table lacks an array");
    if (n == 0) return 0;
    VPHO_REQUIRE(verts && verts_filled && normals_filled, "vpho_hand_surface_f32: bad argument");
    const size_t lds = (size_t)t->F * 6 * sizeof(double) + (size_t)t->V * 3 * sizeof(double) + (size_t)t->V * 3 * sizeof(float);
    VPHO_DYN_LDS(hand_surface_kernel, (HS_MAX_F * 6 + HS_MAX_V * 3) * sizeof(double) + HS_MAX_V * 3 * sizeof(float));
    HandSurfaceArgs a;
    a.verts = verts; a.t = *t; a.verts_filled = verts_filled; a.normals_filled = normals_filled;
    hipLaunchKernelGGL(hand_surface_kernel, dim3(n), dim3(256), lds, (hipStream_t)stream, a);
    return vpho::check_launch("hand_surface_kernel");
}
